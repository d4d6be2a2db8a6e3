"""One BERT layer with dropout ON (both probabilities 0.1, the trained configuration), forward and backward, on the GPU against the project's own
float64 oracle with the numpy dropout masks of tests/dropout_ref.py (tests/bert_dropout_ref.py): the executor of clip_lite_amd/bert.py is called
directly, the four (p, seed, site) tuples are taken out of the context it returns, and the gradients are read from the arena as _BertFn leaves
them. 6 captions of 30 tokens with ragged lengths and one caption mostly padding: 180 rows.

Exact-f32 mode (deterministic reductions): pooled output within 1e-4, every gradient within 2e-3 of max|ref| (the suite's f32 bounds).

bf16 mode, under every tile policy: the bound is measured against the reference's own rounding noise. R64 = the float64 oracle on the bf16-rounded
weight copies, Rbf = the same with bf16 rounding where the product stores bf16 (every Linear output, the GELU output, LayerNorm inputs and
outputs, the attention context; gradients at the same points), floor_t = |Rbf - R64| / |R64|. Asserted: |GPU - R64| / |R64| <= 3 * floor_t for the
pooled output and every gradient tensor of more than 4096 elements, and <= 3 * the largest floor for the smaller ones. The factor 3 covers the
rounding points the emulation leaves out, each of the same 2^-9 size: the attention probabilities and dS held in bf16, dqkv stored in bf16, the
order of atomic sums. tests/test_dropout_ref_host.py shows that a mask applied at the wrong site moves these tensors by 0.4 - 0.65, against floors
of about 1e-2.
The key projection's bias has a gradient of exactly zero (softmax ignores a shift of a row's scores): it is held to the same bound relative to the
query bias's gradient instead of its own."""
import pytest
import torch

import bert_dropout_ref as T
from detfill import det_fill

pytestmark = pytest.mark.gpu
_cache = {}


class _Holder(torch.nn.Module):
    """Gives a lone TextEncoder the `text_encoder` slot model.attach_runtime looks for (as in tests/test_gpu_mpnet.py)."""

    def __init__(self, te):
        super().__init__()
        self.text_encoder = te


def _tower(lowp):
    """(TextEncoder, its runtime, the state dict of its BertModel on the host) — built once per mode."""
    if ("tower", lowp) not in _cache:
        from clip_lite_amd.encoder import TextEncoder
        from clip_lite_amd.model import attach_runtime
        te = TextEncoder(mode="train_sbert", num_hidden_layers=1)
        assert te.strans.hidden_dropout_prob == 0.1 and te.strans.attention_probs_dropout_prob == 0.1
        det_fill(te)
        sd = {k: v.detach().clone() for k, v in te.strans.state_dict().items()}
        holder = _Holder(te).to("cuda").train()
        rt = attach_runtime(holder, torch.device("cuda", torch.cuda.current_device()), lowp, seed=5000)          # step seeds 5000 * 1000003 + k: above 2^32, both key words in use
        _cache["tower", lowp] = (holder, rt, sd)
    return _cache["tower", lowp]


def _run_gpu(lowp):
    """Forward + backward of the executor with the first step's seed; returns (pooled, {name: gradient}, the four dropout tuples)."""
    from clip_lite_amd.bert import bert_backward, bert_forward
    holder, rt, _ = _tower(lowp)
    te = holder.text_encoder
    ids, mask, dpooled = T.problem()
    rt.steps = 0          # every run draws the masks of step 1, so the float64 references are computed once
    rt.arena.flat_g.zero_()
    ids_d, mask_d, dp_d = ids.cuda(), mask.cuda(), dpooled.to(rt.tdtype).cuda()
    pooled, ctx = bert_forward(rt, te.strans, ids_d, mask_d, rt.next_step(True))
    layer = ctx["layers"][0]
    drops = {"d0": ctx["d0"], "da": layer[4], "d1": layer[6], "d2": layer[12]}
    assert all(d[0] == 0.1 for d in drops.values()) and len({d[2] for d in drops.values()}) == 4 and drops["d0"][1] == 5000 * 1000003 + 1
    bert_backward(rt, te.strans, ctx, dp_d)
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().cpu().clone() for n, p in te.strans.named_parameters()}
    return pooled.detach().double().cpu(), grads, drops


def _reference(lowp, drops):
    """Float64 references for these dropout tuples, computed once: exact-f32 mode (pooled, grads); bf16 mode (pooled, grads, floors)."""
    key = ("ref", lowp, tuple(sorted(drops.items())))
    if key not in _cache:
        _, _, sd = _tower(lowp)
        ids, mask, dpooled = T.problem()
        mults = T.multipliers(drops, *ids.shape)
        if not lowp:
            _cache[key] = T.run(T.build(sd, mults, round_weights=False), ids, mask, dpooled)
        else:
            p64, g64 = T.run(T.build(sd, mults), ids, mask, dpooled)
            pbf, gbf = T.run(T.build(sd, mults, emulate=True), ids, mask, dpooled)
            floors = {n: T.rel_l2(gbf[n], g64[n]) for n in g64 if n != T.ZERO_GRAD}
            floors["pooled"] = T.rel_l2(pbf, p64)
            _cache[key] = (p64, g64, floors)
    return _cache[key]


@pytest.mark.usefixtures("deterministic_reductions")
def test_f32_layer_with_dropout_matches_float64_oracle():
    pooled, grads, drops = _run_gpu(False)
    p64, g64 = _reference(False, drops)
    err = (pooled - p64).abs().max().item()
    print(f"pooled: max |GPU - R64| {err:.3e}")
    assert err < 1e-4
    qb = g64[T.ZERO_GRAD.replace("key", "query")].abs().max().item()
    worst = ("", 0.0)
    for n, ref in g64.items():
        scale = qb if n == T.ZERO_GRAD else ref.abs().max().item()
        rel = (grads[n] - ref).abs().max().item() / scale
        worst = max(worst, (n, rel), key=lambda t: t[1])
        assert rel <= 2e-3, (n, rel)
    print("worst gradient error / max|ref|: %s %.3e" % worst)


@pytest.fixture(params=[0, 1, 2, 3, 4], ids=["auto", "w128", "w256x128", "w256", "narrow"])
def tile_policy(request):
    """As the fixture at the top of tests/test_gpu_igemm.py: the tile family every bf16 GEMM of the case is forced onto; restores the automatic one."""
    from clip_lite_amd import hip
    hip.set_tile_policy(request.param)
    yield request.param
    hip.set_tile_policy(0)


def test_bf16_layer_with_dropout_is_within_three_rounding_floors(tile_policy):
    """Observed on MI355X: the worst err_t / floor_t is 1.00 (automatic policy, 128 x 128 and 4-wave tiles) and 0.99 (256-wide tiles), on the key
    projection's weight gradient; floors run from 7.0e-3 (pooled output) to 1.11e-2 (query weight gradient); the key bias's gradient is 2.5e-3 of
    the query bias's. The table is printed on every run."""
    pooled, grads, drops = _run_gpu(True)
    p64, g64, floors = _reference(True, drops)
    top = max(floors.values())
    rows = [("pooled", T.rel_l2(pooled, p64), floors["pooled"])]
    for n, ref in g64.items():
        if n == T.ZERO_GRAD:
            rows.append((n + " (/ |query.bias grad|)", (grads[n].norm() / g64[n.replace("key", "query")].norm()).item(), top))
        else:
            rows.append((n, T.rel_l2(grads[n], ref), floors[n] if ref.numel() > 4096 else top))
    for n, err, floor in rows:
        print(f"{n}: err {err:.3e} floor {floor:.3e} ratio {err / floor:.2f}")
    print("worst ratio: %.2f" % max(err / floor for _, err, floor in rows))
    assert 1e-3 < top < 5e-2          # the floors are bf16 rounding noise
    bad = [(n, err, floor) for n, err, floor in rows if not err <= 3 * floor]
    assert not bad, bad
