"""CPU-side tests of the MPNet text tower: the plain-torch restatement tests/mpnet_ref.py against the fixtures the reference itself produced
(tests/golden/make_mpnet_golden.py), the host-computed bucket table, the MPNet tokenizer framing, the module tree's state-dict keys, and the
loader's padding. No GPU, no transformers."""
import os

import numpy as np
import pytest
import torch

import mpnet_ref as R
from detfill import det_fill
from oracle import ref_model as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MPNET = "sentence-transformers/paraphrase-mpnet-base-v2"


def load(name):
    return dict(np.load(os.path.join(G, name + ".npz")))


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def ref_text(name, layers, mask_key="mask"):
    fx = load(name)
    te = det_fill(RefTextEncoder(layers)).double()
    ids = torch.tensor(fx["ids"])
    mask = torch.ones_like(ids) if mask_key == "ones" else torch.tensor(fx["mask"])
    out = te({"input_ids": ids, "attention_mask": mask})
    (out * torch.tensor(fx["w"]).double()).sum().backward()
    return fx, te, out


RefTextEncoder = R.RefTextEncoder


@pytest.mark.parametrize("name,layers,mask", [("mpnet_l2_b4_len7_ragged", 2, "mask"), ("mpnet_l2_b4_len7_ragged", 2, "ones"), ("mpnet_l1_b3_len30", 1, "mask")])
def test_ref_tower_matches_reference_fixture(name, layers, mask):
    """The float64 restatement within 1e-5 relative of the reference: its float32 pooled output, and every gradient norm and the bias table's
    gradient of the same reference module run in float64 (the generator's note: the reference's float32 backward is itself only good to ~5e-5
    on the large weight gradients). The all-ones mask is what the reference's collate feeds the tower: the fixture holds both."""
    fx, te, out = ref_text(name, layers, mask)
    sfx = "_ones" if mask == "ones" else ""
    assert rel_err(out.detach(), fx["out" + sfx]) < 1e-5 and rel_err(out.detach(), fx["out64" + sfx]) < 1e-5
    g = {k: p.grad for k, p in te.named_parameters() if p.grad is not None}
    names = [str(n) for n in fx["gnames"]]
    assert sorted(g) == names          # (the pooler gets no gradient in the reference either)
    gmax = float(fx["gnorms64" + sfx].max())          # (the key biases' gradient is zero in exact arithmetic - softmax ignores a per-row shift - hence the floor,
    for n, ref in zip(names, fx["gnorms64" + sfx]):          # the one tests/test_gpu_model.py uses)
        assert abs(g[n].norm().item() - ref) <= 1e-5 * max(ref, 1e-3 * gmax), (n, g[n].norm().item(), ref)
    assert rel_err(g["strans.encoder.relative_attention_bias.weight"], fx["g_rel64" + sfx]) < 1e-5


def test_ref_model_matches_reference_fixture():
    """The reference VLInfoModel with the 2-layer MPNet tower: the four loss scalars and the bias table's gradient from the oracle's image
    encoder and loss around the restated tower, all in float64."""
    fx = load("model_rn18_mpnet2_b4")
    M = O.OracleVLInfoModel(RefTextEncoder(2), O.OracleImageEncoder("resnet18"), O.OracleJSDInfoMaxLoss(512, 768, "dot", 0.1, True, True), "train_sbert")
    det_fill(M).double().train()
    M.loss.noise = (torch.tensor(fx["u_img"]).double(), torch.tensor(fx["u_txt"]).double())
    out = M({"image": torch.tensor(fx["image"]).double(), "input_ids": torch.tensor(fx["input_ids"]), "attention_mask": torch.tensor(fx["attention_mask"])})
    out["loss"].backward()
    assert rel_err(out["loss"].detach(), fx["total"]) < 1e-5 and rel_err(out["loss"].detach(), fx["total64"]) < 1e-5
    comp = out["loss_components"]
    for k, f in (("cross_modal_loss", "cross"), ("visual_loss", "visual"), ("textual_loss", "textual")):
        assert abs(float(comp[k]) - float(fx[f])) <= 1e-5 * max(abs(float(fx[f])), abs(float(fx["total"]))), k
    g = {k: p.grad for k, p in M.named_parameters() if p.grad is not None}
    names = [str(n) for n in fx["gnames"]]
    assert sorted(g) == names
    gmax = float(fx["gnorms64"].max())
    for n, ref in zip(names, fx["gnorms64"]):          # (against the float64 run of the reference modules)
        assert abs(g[n].norm().item() - ref) <= 1e-5 * max(ref, 1e-3 * gmax), (n, g[n].norm().item(), ref)
    assert rel_err(g["text_encoder.strans.encoder.relative_attention_bias.weight"], fx["g_rel64"]) < 1e-5


def test_bucket_table_matches_fixture():
    from clip_lite_amd import hip
    fx = load("mpnet_buckets")
    assert fx["offsets"].tolist() == list(range(-31, 32))
    want = fx["buckets"].tolist()
    assert hip.relative_position_buckets() == want == R.bucket_table()
    assert want[:31] == [R.bucket(r) for r in range(-31, 0)] and want[30] == 1 and want[0] == 11 and want[31] == 0 and min(want[32:]) == 17 and max(want) == 27


def test_position_ids():
    ids = torch.tensor([[0, 5, 1, 7, 2, 1, 1], [0, 2, 1, 1, 1, 1, 1]])
    assert R.position_ids(ids).tolist() == [[2, 3, 1, 4, 5, 1, 1], [2, 3, 1, 1, 1, 1, 1]]


def test_tokenizer_matches_transformers_mpnet_tokenizer_golden():
    from clip_lite_amd.data import WordPieceTokenizer, normalize_caption
    fx = np.load(os.path.join(G, "tokens_mock_mpnet.npz"))
    tok = WordPieceTokenizer(os.path.join(G, "vocab_mock_mpnet.txt"), framing="mpnet")
    assert (tok.cls_token_id, tok.pad_token_id, tok.sep_token_id, tok.unk_token_id) == (0, 1, 2, 3)
    for cap, L, want in zip(fx["captions"], fx["max_length"], fx["input_ids"]):
        assert tok(normalize_caption(str(cap), int(L)), int(L)) == [int(t) for t in want if t >= 0], cap
    for cap, L, want in zip(fx["raw_captions"], fx["raw_max_length"], fx["raw_input_ids"]):
        assert tok(str(cap), int(L)) == [int(t) for t in want if t >= 0], cap
    import pickle
    again = pickle.loads(pickle.dumps(tok))
    assert again.framing == "mpnet" and again("a cat", 8) == tok("a cat", 8)


def test_state_dict_keys_match_reference():
    from clip_lite_amd.encoder import TextEncoder
    fx = load("mpnet_l2_b4_len7_ragged")
    te = TextEncoder(mode="train_sbert", model_name=MPNET, num_hidden_layers=2)
    sd = te.state_dict()
    assert list(sd) == [str(k) for k in fx["keys"]]
    shapes = R.param_shapes(2)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"strans." + k: v for k, v in shapes.items()}
    frozen = sorted(k for k, p in te.named_parameters() if not p.requires_grad)
    assert frozen == ["strans.pooler.dense.bias", "strans.pooler.dense.weight"]
    te.dont_train_enc()
    te.train_enc()
    assert sorted(k for k, p in te.named_parameters() if not p.requires_grad) == frozen          # train_enc() leaves the unused pooler frozen
    assert sorted(k for k, p in te.named_parameters() if p.requires_grad) == [str(n) for n in fx["gnames"]]
    assert len(TextEncoder(mode="train_sbert", model_name=MPNET).strans.encoder.layer) == 12


def test_bert_name_builds_the_same_module_as_before():
    from clip_lite_amd.bert import BertModel
    from clip_lite_amd.encoder import TextEncoder
    te = TextEncoder(mode="train_sbert", model_name="bert-base-uncased", num_hidden_layers=2)
    assert type(te.strans) is BertModel and te.strans.kind == "bert"
    want = BertModel(num_hidden_layers=2)
    assert {k: tuple(v.shape) for k, v in te.strans.state_dict().items()} == {k: tuple(v.shape) for k, v in want.state_dict().items()}
    assert list(te.strans.state_dict()) == list(want.state_dict())
    assert all(p.requires_grad for p in te.parameters())
    fx = load("text_l2_b4_len7_ragged")          # the reference's own list of BERT parameters
    assert sorted(k for k, _ in te.named_parameters()) == [str(n) for n in fx["gnames"]]
    assert te.strans.embeddings.token_type_embeddings.weight.shape == (2, 768)


def test_pretrained_raises_with_the_real_reason():
    from clip_lite_amd.encoder import TextEncoder
    for name in ("bert-base-uncased", MPNET):
        with pytest.raises(RuntimeError, match="download"):
            TextEncoder(mode="train_sbert", model_name=name, pretrained=True)


def test_loader_pads_ids_with_one_and_mask_with_zero():
    from clip_lite_amd import data as D
    ds = D.RandomDataset(image_size=32, length=8, text_model=MPNET)
    items = [ds[i] for i in range(4)]
    batch = ds.collate_fn(items)
    ids, mask = batch["input_ids"], batch["attention_mask"]
    lens = [len(i["caption_tokens"]) for i in items]
    assert len(set(lens)) > 1
    for r, n in enumerate(lens):
        assert ids[r, 0] == 0 and ids[r, n - 1] == 2 and (ids[r, n:] == 1).all() and (mask[r, :n] == 1).all() and (mask[r, n:] == 0).all()
        assert (ids[r, 1:n - 1] >= 4).all() and (ids[r, 1:n - 1] < D.MPNET_VOCAB_SIZE).all()          # the hashed fallback never emits a special inside
    # with a vocabulary: the tokenizer's own pad id
    ds = D.RandomDataset(image_size=32, length=8, text_model=MPNET, tokenizer_vocab=os.path.join(G, "vocab_mock_mpnet.txt"))
    batch = ds.collate_fn([ds[i] for i in range(4)])
    assert ds.pad_token_id == 1 and ((batch["input_ids"] == 1) == (batch["attention_mask"] == 0)).all()
    # a BERT name is untouched: [CLS] ... [SEP], pad id 0
    ds = D.RandomDataset(image_size=32, length=8)
    batch = ds.collate_fn([ds[i] for i in range(4)])
    assert (batch["input_ids"][:, 0] == 101).all() and ((batch["input_ids"] == 0) == (batch["attention_mask"] == 0)).all()
    from clip_lite_amd.downstream import tokenize_texts
    ids, mask = tokenize_texts(["a photo of a cat", "dog"], 12, text_model=MPNET)
    assert (ids[mask == 0] == 1).all() and (ids[:, 0] == 0).all()


def test_factory_passes_the_text_model_name():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import PretrainingDatasetFactory
    c = Config(os.path.join(os.path.dirname(G), "..", "configs", "smoke_random_mpnet.yaml"))
    ds = PretrainingDatasetFactory.from_config(c)
    assert ds.framing == "mpnet" and ds.pad_token_id == 1
    assert c.MODEL.TEXTUAL.NETWORK_NAME == MPNET and c.MODEL.TEXTUAL.NUM_HIDDEN_LAYERS == 2
