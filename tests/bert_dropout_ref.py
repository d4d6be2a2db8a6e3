"""The float64 reference of one BERT layer with dropout ON (test infrastructure; shared by tests/test_dropout_ref_host.py and
tests/test_gpu_bert_dropout_tower.py): the project's own oracle.ref_model.OracleBert in float64 with each of its nn.Dropout modules replaced, at
test time, by a multiplication with keep / (1 - p), where `keep` is the numpy mask of tests/dropout_ref.py for that site's (p, seed, site).

R64 = the oracle on the bf16-rounded weight copies (what the bf16 kernels read); Rbf = the same with bf16_emulation.Round at the points where the
product stores bf16 (every Linear output, the GELU output, LayerNorm inputs and outputs, the attention context), and on the gradients at the
same points. floor_t = |Rbf - R64| / |R64| of tensor t is the rounding noise no bf16 implementation of this scheme can be below."""
import numpy as np
import torch
import torch.nn as nn

import dropout_ref as D
from bf16_emulation import Round
from detfill import det_tensor

HEADS, HIDDEN = 12, 768
# softmax is invariant to a shift of all scores of a row, so the key projection's bias has a gradient of exactly zero: no relative error exists for it
ZERO_GRAD = "encoder.layer.0.attention.self.key.bias"
SITES = ("d0", "da", "d1", "d2")      # embeddings, attention probabilities, attention output projection, FFN output projection: bert_forward's order


def problem(B=6, L=30, vocab=30522):
    """ids [B][L] (ragged lengths, the last caption padded to a few tokens), mask [B][L], dpooled [B][768] with bf16-representable values."""
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1000, vocab, (B, L), generator=g)
    lens = [L, L - 1, 17, L, 23, 6][:B]
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, 0], ids[b, n - 1] = 101, 102
        ids[b, n:] = 0
        mask[b, :n] = 1
    return ids, mask, det_tensor("dpooled", (B, HIDDEN), "normal").bfloat16().float()


class _Keep(nn.Module):
    """Stands in for an nn.Dropout: x * keep / (1 - p) with a fixed mask."""

    def __init__(self, mult):
        super().__init__()
        self.mult = mult

    def forward(self, x):
        return x * self.mult.view(x.shape)


def multipliers(drops, B, L):
    """{site name: float64 multiplier tensor} for drops = {site name: (p, seed, site)}."""
    out = {}
    for name in SITES:
        p, seed, site = drops[name]
        if name == "da":
            keep = D.attention_keep(seed, site, B, HEADS, L, p)
        else:
            keep = D.hidden_keep(seed, site, B * L, HIDDEN, p)
        out[name] = torch.from_numpy(keep.astype(np.float64)) / (1.0 - np.float64(np.float32(p)))
    return out


def _r(x):
    return Round.apply(x).to(x.dtype)


def build(state_dict, mults, emulate=False, vocab=30522, round_weights=True):
    """OracleBert(1) in float64 with the four dropouts replaced by `mults` (multipliers()). round_weights: Linear / Embedding weights rounded to
    bf16, the copies the bf16 kernels read (biases and LayerNorm parameters stay f32 there too); False for the exact-f32 mode."""
    from oracle.ref_model import OracleBert
    net = OracleBert(1, vocab=vocab)
    net.load_state_dict({k: v.detach().float().cpu() for k, v in state_dict.items()})
    for m in net.modules():
        if round_weights and isinstance(m, (nn.Linear, nn.Embedding)):
            m.weight.data = m.weight.data.bfloat16().float()
    net = net.double().train()
    layer = net.encoder.layer[0]
    owners = {"d0": net.embeddings, "da": layer.attention.self, "d1": layer.attention.output, "d2": layer.output}
    for name, owner in owners.items():
        assert isinstance(owner.dropout, nn.Dropout)
        owner.dropout = _Keep(mults[name])
    if emulate:
        for m in net.modules():
            if isinstance(m, nn.Linear):
                m.register_forward_hook(lambda mod, inp, out: _r(out))
            elif isinstance(m, nn.LayerNorm):
                m.register_forward_pre_hook(lambda mod, inp: (_r(inp[0]),))
                m.register_forward_hook(lambda mod, inp, out: _r(out))
        layer.attention.self.register_forward_hook(lambda mod, inp, out: _r(out))          # the attention context
        layer.output.dense.register_forward_pre_hook(lambda mod, inp: (_r(inp[0]),))       # the GELU output (F.gelu in the oracle: rounded where it is read)
    return net


def run(net, ids, mask, dpooled):
    """(pooled [B][768], {parameter name: gradient}) in float64."""
    net.zero_grad(set_to_none=True)
    pooled = net(ids, mask)
    pooled.backward(dpooled.double())
    return pooled.detach(), {n: p.grad.detach() for n, p in net.named_parameters()}


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300)).item()
