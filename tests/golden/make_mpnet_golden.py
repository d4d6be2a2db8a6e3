"""Golden fixtures of the MPNet text tower, made by running the REFERENCE itself (its encoder.TextEncoder / model.VLInfoModel on
transformers' MPNetModel) in the build container — the import recipe is make_golden.py's, imported from there. Only seeded inputs, key lists
and the reference's numeric outputs are stored; weights come from tests/detfill.py by name.

    python tests/golden/make_mpnet_golden.py

Writes into tests/golden/:
    mpnet_buckets.npz              MPNetEncoder.relative_position_bucket for the relative offsets -31 .. 31 (what pins the kernels' table)
    mpnet_l1_b3_len30.npz          TextEncoder(mode="train_sbert", model_name=<MPNet>) with 1 layer: inputs, mean-pooled output, gradient norms
    mpnet_l2_b4_len7_ragged.npz    2 layers, pad ids (1) at the tail with the correct mask — and the same inputs under the reference's all-ones mask
    model_rn18_mpnet2_b4.npz       the four loss scalars and per-tensor gradient norms of the reference VLInfoModel with that tower
    vocab_mock_mpnet.txt / tokens_mock_mpnet.npz    transformers.MPNetTokenizer over a mock vocabulary built like vocab_mock.txt

The reference hard-codes transformers.MPNetConfig() (12 layers); the generator substitutes a config with fewer layers while it builds the
reference encoder, nothing else."""
import json
import os

import numpy as np
import torch

import make_golden as MG                     # stubs the absent third-party modules and imports the reference
from make_golden import HERE, det_fill, det_tensor, grads, pin_noise, ref_encoder, ref_loss, ref_model, save

transformers = ref_encoder.transformers      # the module object the reference's encoder.py resolves `transformers.MPNetConfig` on
from make_tokens_golden import EXTRA, build_vocab

MPNET = "sentence-transformers/paraphrase-mpnet-base-v2"


def ref_text_encoder(layers):
    orig = transformers.MPNetConfig
    transformers.MPNetConfig = lambda *a, **k: orig(*a, num_hidden_layers=layers, **k)
    try:
        te = ref_encoder.TextEncoder(word_dict={}, mode="train_sbert", model_name=MPNET)
    finally:
        transformers.MPNetConfig = orig
    assert len(te.strans.encoder.layer) == layers
    for m in te.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return te


def mpnet_ids(B, Ls, seed, ragged):
    """<s> = 0 first, </s> = 2 last, words in [4, 30527), pad id 1 at the tail of the ragged rows"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(4, 30527, (B, Ls), generator=g)
    ids[:, 0] = 0
    mask = torch.ones(B, Ls, dtype=torch.long)
    for b in range(B):
        n = Ls - (b % 3) if ragged else Ls
        mask[b, n:] = 0
        ids[b, n:] = 1
        ids[b, n - 1] = 2
    return ids, mask


def g_buckets():
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    rel = torch.arange(-31, 32)
    save("mpnet_buckets", offsets=rel, buckets=MPNetEncoder.relative_position_bucket(rel, num_buckets=32))


def run_text(te, ids, mask, w):
    te.zero_grad()
    out = te({"input_ids": ids, "attention_mask": mask})
    (out * w.to(out.dtype)).sum().backward()
    return out.detach().clone(), grads(te)


def norms(gr):
    return np.array([gr[k].double().norm().item() for k in sorted(gr)])


def g_text(tag, B, Ls, layers, ragged):
    te = det_fill(ref_text_encoder(layers)).train()
    ids, mask = mpnet_ids(B, Ls, 1234, ragged)
    w = det_tensor(tag + "w", (B, 768), "normal")
    out, gr = run_text(te, ids, mask, w)
    # The same reference module once more in float64 (`*64` entries): its float32 backward is good to ~5e-5 relative on the large weight
    # gradients (measured here: 689.934 against 689.969 for layer 0's intermediate.dense.weight), which a 1e-5 comparison cannot resolve;
    # the float32 entries are what the float32 kernels are compared with.
    te64 = det_fill(ref_text_encoder(layers)).double().train()
    out64, gr64 = run_text(te64, ids, mask, w)
    arrs = dict(ids=ids, mask=mask, out=out, w=w, keys=np.array(list(te.state_dict().keys())), gnames=np.array(sorted(gr)),
                gnorms=norms(gr), out64=out64, gnorms64=norms(gr64), g_rel64=gr64["strans.encoder.relative_attention_bias.weight"],
                g_rel=gr["strans.encoder.relative_attention_bias.weight"], g_ln0_w=gr["strans.embeddings.LayerNorm.weight"],
                g_pos=gr["strans.embeddings.position_embeddings.weight"][:Ls + 2], g_q0_b=gr["strans.encoder.layer.0.attention.attn.q.bias"])
    if ragged:          # what the reference's collate feeds the tower: the mask padded with pad_token_id = 1, i.e. all ones
        out1, gr1 = run_text(te, ids, torch.ones_like(mask), w)
        out164, gr164 = run_text(te64, ids, torch.ones_like(mask), w)
        arrs.update(out_ones=out1, gnorms_ones=norms(gr1), g_rel_ones=gr1["strans.encoder.relative_attention_bias.weight"],
                    out64_ones=out164, gnorms64_ones=norms(gr164), g_rel64_ones=gr164["strans.encoder.relative_attention_bias.weight"])
        assert sorted(gr1) == sorted(gr)
    save(tag, **arrs)


def g_model(tag, B, S, Ls, layers):
    ids, mask = mpnet_ids(B, Ls, 77, False)
    batch = {"image": det_tensor(tag + "image", (B, 3, S, S), "normal"), "input_ids": ids, "attention_mask": mask}
    u_img, u_txt = det_tensor(tag + "u_img", (B, 512), "uniform"), det_tensor(tag + "u_txt", (B, 768), "uniform")

    def run(double):
        ie = MG.OracleImageEncoder("resnet18")
        te = ref_text_encoder(layers)
        L = ref_loss.JSDInfoMaxLoss(image_dim=512, text_dim=768, type="dot", prior_weight=0.1, image_prior=True, text_prior=True)
        M = det_fill(ref_model.VLInfoModel(te, ie, L, "train_sbert", is_amp=False))
        b = dict(batch)
        if double:
            M.double()
            b["image"] = b["image"].double()
        M.train()
        out = pin_noise(lambda: M(b), [u_img, u_txt])
        out["loss"].backward()
        return out, grads(M)

    out, gr = run(False)
    out64, gr64 = run(True)          # (see g_text: the float64 run of the same reference modules)
    comp = out["loss_components"]
    save(tag, **batch, u_img=u_img, u_txt=u_txt, total=out["loss"], cross=comp["cross_modal_loss"], visual=comp["visual_loss"],
         textual=comp["textual_loss"], gnames=np.array(sorted(gr)), gnorms=norms(gr), total64=out64["loss"], gnorms64=norms(gr64),
         g_conv1=gr["image_encoder.img_encoder.conv1.weight"], g_temperature=gr["loss.global_d.temperature"],
         g_rel=gr["text_encoder.strans.encoder.relative_attention_bias.weight"],
         g_rel64=gr64["text_encoder.strans.encoder.relative_attention_bias.weight"])


def g_tokens():
    from clip_lite_amd.data import normalize_caption
    with open(os.path.join(os.path.dirname(ref_encoder.__file__), "data", "mock_data.json")) as fh:
        captions = [r["caption"] if isinstance(r["caption"], str) else r["caption"][0] for r in json.load(fh)]
    bert = build_vocab(captions)
    # MPNet's layout: <s>, <pad>, </s>, <unk> at 0 .. 3 in place of BERT's specials, <mask> last
    vocab = ["<s>", "<pad>", "</s>", "<unk>"] + [t for t in bert if not (t.startswith("[") and t.endswith("]"))] + ["<mask>"]
    vp = os.path.join(HERE, "vocab_mock_mpnet.txt")
    with open(vp, "w", encoding="utf-8") as fh:
        fh.write("\n".join(vocab) + "\n")
    vdict = {t: i for i, t in enumerate(vocab)}
    tk = transformers.MPNetTokenizer(vocab=vdict, do_lower_case=True, unk_token="<unk>")
    assert (tk.cls_token_id, tk.pad_token_id, tk.sep_token_id, tk.unk_token_id) == (0, 1, 2, 3)
    cases = [(c, 30) for c in captions] + [(c, 12) for c in captions[:10]] + EXTRA
    ids = [list(tk(normalize_caption(cap, L), padding=False, truncation=True, max_length=L)["input_ids"]) for cap, L in cases]
    raw = [list(tk(cap, padding=False, truncation=True, max_length=L)["input_ids"]) for cap, L in EXTRA]
    width = max(len(r) for r in ids + raw)
    pad = lambda rows: np.array([r + [-1] * (width - len(r)) for r in rows], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "tokens_mock_mpnet.npz"), captions=np.array([c for c, _ in cases]),
                        max_length=np.array([L for _, L in cases], dtype=np.int32), input_ids=pad(ids), raw_captions=np.array([c for c, _ in EXTRA]),
                        raw_max_length=np.array([L for _, L in EXTRA], dtype=np.int32), raw_input_ids=pad(raw))
    print(f"{len(cases)} + {len(EXTRA)} cases, vocab {len(vocab)}, {sum(r.count(3) for r in ids + raw)} <unk>, longest {width}")


if __name__ == "__main__":
    g_buckets()
    g_text("mpnet_l2_b4_len7_ragged", 4, 7, 2, True)
    g_text("mpnet_l1_b3_len30", 3, 30, 1, False)
    g_model("model_rn18_mpnet2_b4", 4, 64, 9, 2)
    g_tokens()
