"""Host-side checks of the SigLIP reference (tests/siglip_ref.py) and of SigLIPLoss's construction (no GPU).

(a) The float64 reference against central finite differences (step 1e-6, bound relative 1e-6, as tests/test_loss_ref_host.py) for C, temperature
and bias; against a literal restatement of the paper's pseudocode (Zhai et al. 2023, Algorithm 1: -sum(log_sigmoid(labels * logits)) / n); and
finite at t = 100, bias = +-10, cosines +-1, where |x| reaches 110.

(b) SigLIPLoss: its state-dict keys and initial values, the factory name, the smoke configuration, the refusal of another critic. The key lists
of JSDInfoMaxLoss and InfoNCELoss hold no `global_d.bias`."""
import os
import re

import numpy as np
import pytest
import torch

import siglip_ref as S
from test_loss_ref_host import H, _fd_check, _picks, _tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("t,b", [(S.T_INIT, S.B_INIT), (S.T100, -3.0), (1.3, 0.4)])
def test_gradients_match_finite_differences(t, b):
    rng = np.random.default_rng(5)
    B, g = 9, 1.17
    Cm = np.clip(rng.standard_normal((B, B)) * 0.3 + 0.5 * np.eye(B), -1, 1)
    ref = S.siglip_ref(Cm, t, b, gout=g)

    def loss(c, tt, bb):
        return g * S.siglip_loss(_tt(c), _tt(tt), _tt(bb))[0].item()

    _fd_check("dC", lambda c: loss(c, t, b), Cm, ref.dC, _picks(rng, Cm.shape) + [(4, 4)])
    fd = (loss(Cm, t + H, b) - loss(Cm, t - H, b)) / (2 * H)
    assert abs(ref.dtemp - fd) <= 1e-6 * abs(fd)
    fd = (loss(Cm, t, b + H) - loss(Cm, t, b - H)) / (2 * H)
    assert abs(ref.dbias - fd) <= 1e-6 * abs(fd)
    # the term tables sum to the gradients, and the row terms to the loss
    assert abs(ref.dtemp_terms.sum() - ref.dtemp) <= 1e-12 * np.abs(ref.dtemp_terms).sum()
    assert abs(ref.dbias_terms.sum() - ref.dbias) <= 1e-12 * np.abs(ref.dbias_terms).sum()
    assert abs(ref.row_terms.sum() - ref.loss) <= 1e-14 * ref.loss and ref.row_terms.shape == (B,)
    # the issue's closed forms: dL/dx = -z sigmoid(-z x) / B, dC = g t dL/dx
    z = 2 * np.eye(B) - 1
    x = np.exp(t) * Cm + b
    dx = -z / (1 + np.exp(z * x)) / B
    assert np.abs(ref.dbias_terms - g * dx).max() <= 1e-14 and np.abs(ref.dC - g * np.exp(t) * dx).max() <= 1e-13 * np.exp(t)
    # the plain-float32 evaluation is the same formula
    assert np.abs(S.siglip_dC_float32(Cm, t, b, g) - ref.dC).max() <= 1e-4 * np.abs(ref.dC).max()


def test_matches_the_papers_pseudocode():
    """Algorithm 1 of the paper on already-normalised embeddings: logits = dot(zimg, ztxt.T) * t + b; labels = 2 * eye(n) - ones(n);
    l = -sum(log_sigmoid(labels * logits)) / n."""
    rng = np.random.default_rng(6)
    n = 12
    zimg = torch.nn.functional.normalize(_tt(rng.standard_normal((n, 16))), dim=-1)
    ztxt = torch.nn.functional.normalize(_tt(rng.standard_normal((n, 16))) + 0.7 * zimg, dim=-1)
    for t_prime, b in ((S.T_INIT, S.B_INIT), (S.T100, -3.0)):
        t = np.exp(t_prime)
        logits = zimg @ ztxt.T * t + b
        labels = 2 * torch.eye(n, dtype=torch.float64) - torch.ones(n, n, dtype=torch.float64)
        want = -torch.sum(torch.nn.functional.logsigmoid(labels * logits)) / n
        got = S.siglip_ref((zimg @ ztxt.T).numpy(), t_prime, b).loss
        assert abs(got - want.item()) <= 1e-13 * want.item()


@pytest.mark.parametrize("b", [10.0, -10.0])
def test_finite_at_the_extremes(b):
    Cm = np.array([[1.0, -1.0, 1.0], [-1.0, -1.0, 1.0], [1.0, 1.0, 1.0]])
    ref = S.siglip_ref(Cm, S.T100, b)
    assert np.abs(np.exp(S.T100) * Cm + b).max() >= 109.9
    for v in ref:
        assert np.isfinite(np.asarray(v)).all()
    assert np.isfinite(S.siglip_dC_float32(Cm, S.T100, b, 1.0)).all()
    # x = 110 on a diagonal entry costs nothing, x = -110 there costs 110 / B: the softplus is linear, not inf
    want = sum(max(-(1 if i == j else -1) * (np.exp(S.T100) * Cm[i, j] + b), 0.0) for i in range(3) for j in range(3)) / 3
    assert abs(ref.loss - want) <= 1e-9 * want


# ------------------------------------------------------------------------------------------------ (b) the host class
def _keys(loss):
    return [k for k in loss.state_dict() if k.startswith("global_d.") and "_block." not in k]


def test_siglip_loss_construction():
    from clip_lite_amd.loss import InfoNCELoss, JSDInfoMaxLoss, SigLIPLoss
    ls = SigLIPLoss(512, 768, "dot", 0.1, True, True)
    assert ls.estimator == "siglip" and _keys(ls) == ["global_d.temperature", "global_d.bias"]
    assert ls.global_d.bias.shape == () and ls.global_d.bias.item() == -10.0 and ls.global_d.bias.requires_grad
    assert abs(ls.global_d.temperature.item() - np.log(10.0)) < 1e-6
    # the heads and priors are the inherited ones: every other key, shape for shape
    base = JSDInfoMaxLoss(512, 768, "dot", 0.1, True, True)
    assert [(k, tuple(v.shape)) for k, v in ls.state_dict().items() if k != "global_d.bias"] == [(k, tuple(v.shape)) for k, v in base.state_dict().items()]
    for other in (base, InfoNCELoss(512, 768, "dot", 0.1, True, True)):
        assert _keys(other) == ["global_d.temperature"] and not any(k.endswith("global_d.bias") for k in other.state_dict())
        assert abs(other.global_d.temperature.item() - np.log(1 / 0.07)) < 1e-6
    for kind in ("concat", "condot", "dotcon"):
        with pytest.raises(ValueError, match="SigLIPLoss needs the dot critic"):
            SigLIPLoss(512, 768, kind)


def test_factory_and_smoke_config():
    from clip_lite_amd.config import Config
    from clip_lite_amd.factories import LossFactory
    from clip_lite_amd.loss import InfoNCELoss, JSDInfoMaxLoss, SigLIPLoss
    assert LossFactory.PRODUCTS["siglip"] is SigLIPLoss and LossFactory.PRODUCTS["jsd"] is JSDInfoMaxLoss and LossFactory.PRODUCTS["infonce"] is InfoNCELoss
    c = Config(os.path.join(ROOT, "configs", "smoke_random_siglip.yaml"))
    assert c.MODEL.LOSS.NAME == "siglip" and c.MODEL.LOSS.TYPE == "dot" and c.OPTIM.BATCH_SIZE % 8 == 0
    loss = LossFactory.from_config(c)
    assert type(loss) is SigLIPLoss and loss.image_dim == 768 and loss.text_dim == 512
    # the smoke configuration differs from the CLIP one in the loss name only
    ref = Config(os.path.join(ROOT, "configs", "smoke_random_clip.yaml"), ["MODEL.LOSS.NAME", "siglip"])
    assert str(ref) == str(c)
    # both new scalars are exempt from weight decay
    assert re.match(c.OPTIM.NO_DECAY, "loss.global_d.bias") and re.match(c.OPTIM.NO_DECAY, "loss.global_d.temperature")
    with pytest.raises(ValueError, match="SigLIPLoss needs the dot critic"):
        LossFactory.from_config(Config(os.path.join(ROOT, "configs", "smoke_random_siglip.yaml"), ["MODEL.LOSS.TYPE", "concat"]))


def test_extra_views_are_refused_by_name():
    """Hard negatives / augmented views reach the refusal before any kernel; the runtime is a stub."""
    import types
    from clip_lite_amd.loss import SigLIPLoss
    ls = SigLIPLoss(16, 16, "dot", 0.1, False, False)
    ls._clite_rt = types.SimpleNamespace(next_step=lambda training: None)
    x = torch.zeros(8, 16)
    with pytest.raises(NotImplementedError, match="SigLIPLoss"):
        ls(x, x, aug_image_features=x)
    with pytest.raises(NotImplementedError, match="SigLIPLoss"):
        ls(x, x, neg_image_features=x, neg_text_features=x)
