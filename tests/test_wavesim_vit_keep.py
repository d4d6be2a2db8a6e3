"""Patch dropout of the ViT tower on the wave simulator: the four kernels of csrc/vit_ops.hip through the C ABI (the checks of
tests/vit_keep_checks.py, shared with tests/test_gpu_vit_keep.py), which kernels a tower launches with the option off, in eval mode and in
training, and the smallest tower case against float64. Runs without a GPU."""
import ctypes as C

import pytest
import torch

import simlib
import vit_keep_checks as K
from detfill import det_tensor
from loss_backends import BF16, F32


@pytest.fixture(scope="module")
def be():
    return K.Sim()


@pytest.mark.parametrize("B,P,Kk", K.INDEX_SHAPES)
def test_keep_indices_equal_the_reference(be, B, P, Kk):
    K.check_indices(be, B, P, Kk)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("H,W,p,Kk", K.PATCHIFY_SHAPES)
def test_patchify_keep_is_the_kept_rows_of_the_patch_matrix(be, dtype, H, W, p, Kk):
    K.check_patchify(be, dtype, H, W, p, Kk)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("Cc,B,P,Kk", K.TOKEN_SHAPES)
def test_tokens_keep_forward(be, dtype, Cc, B, P, Kk):
    K.check_tokens_fwd(be, dtype, Cc, B, P, Kk)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("Cc,B,P,Kk", K.TOKEN_SHAPES)
def test_tokens_keep_backward(be, dtype, Cc, B, P, Kk):
    K.check_tokens_bwd(be, dtype, Cc, B, P, Kk)


def test_refusals(be):
    K.check_refusals(be, null_pointers=True)


# ---------------------------------------------------------------------------------------------------- the executor on the simulator
@pytest.fixture
def sim_hip(monkeypatch):
    from clip_lite_amd import hip
    simlib.build_sim()
    monkeypatch.setattr(hip, "_lib", hip._bind(C.CDLL(simlib.SIM_SO)))
    monkeypatch.setattr(hip, "_allow_host_tensors", True)
    return hip


def _small(r, **kw):
    return K.build_tower("vit_b_32", (64, 96), 1, r, "cpu", False, hidden=64, heads=1, mlp_dim=128, **kw)


def _names(log):
    return [n for n, _, _ in log]


def _launches(holder, image, train, backward):
    """kernel instantiations one pass launches, in order (dry run: the launches are logged, the kernels not executed)"""
    holder.train(train)
    simlib.set_dry_run(True)
    simlib.clear_launch_log()
    try:
        if backward:
            holder.image_encoder(image).backward(torch.ones(image.shape[0], 64))
        else:
            with torch.no_grad():
                holder.image_encoder(image)
        return simlib.launch_log()
    finally:
        simlib.set_dry_run(False)
        simlib.clear_launch_log()


def test_dispatch(sim_hip):
    """Ratio 0, and ratio 0.5 in eval mode or frozen, launch exactly what the tower without the option launches - names, grids, blocks; a
    training pass with 0.5 launches the four keep kernels instead of the three full ones, and the attention of its own length: 192 x 192 pixels
    are 37 tokens (the four-key-tile f32 attention), of which 19 remain (the one-tile kernels)."""
    from clip_lite_amd.encoder import ImageEncoder
    size = 192
    image = det_tensor("dispatch-image", (2, 3, size, size), "normal")
    mk = lambda r, **kw: K.build_tower("vit_b_32", size, 1, r, "cpu", False, hidden=64, heads=1, mlp_dim=128, **kw)[0]
    plain, off, on, frozen = mk(0.0), mk(0.0), mk(0.5), mk(0.5, frozen=True)
    assert isinstance(plain.image_encoder, ImageEncoder) and on.image_encoder.img_encoder.patch_dropout == 0.5
    base_train, base_eval = _launches(plain, image, True, True), _launches(plain, image, False, False)
    assert any("vit_patchify_kernel<" in n for n in _names(base_train)) and any("attention_long_fwd_kernel<" in n for n in _names(base_eval))
    assert not any("keep" in n for n in _names(base_train))
    assert _launches(off, image, True, True) == base_train and _launches(off, image, False, False) == base_eval
    assert _launches(on, image, False, False) == base_eval
    steps = on.rt.steps
    assert _launches(frozen, image, True, False) == base_eval and on.rt.steps == steps          # (no seed drawn either)
    log = _names(_launches(on, image, True, True))
    for family in ("vit_keep_indices_kernel", "vit_patchify_keep_kernel<", "vit_tokens_keep_fwd_kernel<", "vit_tokens_keep_bwd_kernel<"):
        assert sum(family in n for n in log) == 1, (family, log)
    for family in ("vit_patchify_kernel<", "vit_tokens_fwd_kernel<", "vit_tokens_bwd_kernel<", "attention_long_"):
        assert not any(family in n for n in log), (family, log)
    assert sum("attention_fwd_kernel<" in n for n in log) == 1 and sum("attention_bwd_kernel<" in n for n in log) == 1
    # everything else is the same sequence of kernel families on fewer rows (the GEMM launchers pick their instantiation by the row count)
    strip = lambda names: [n.split("<")[0] for n in names if "vit_" not in n and "attention" not in n]
    assert strip(log) == strip(_names(base_train))
    assert on.rt.steps == steps + 1


def test_executor_matches_reference_in_exact_f32(sim_hip):
    """the smallest tower case: 64 x 96 pixels, 6 patches of which 3 are kept (4 tokens), one layer - here 64 wide with one head"""
    holder, sd = _small(0.5)
    image, dfeat = det_tensor("keep-image", (3, 3, 64, 96), "normal"), det_tensor("keep-dfeat", (3, 64), "normal")
    K.check_tower_f32(holder, sd, 1, 1, image, dfeat, 0.5)


def test_eval_features_do_not_depend_on_the_ratio(sim_hip):
    """the same weights with ratio 0 and 0.5: equal features in eval mode bit for bit, other features in training"""
    image = det_tensor("keep-image", (3, 3, 64, 96), "normal")
    (h0, _), (h5, _) = _small(0.0), _small(0.5)
    with torch.no_grad():
        want = h0.eval().image_encoder(image)
        assert torch.equal(h5.eval().image_encoder(image), want)
        got = h5.train().image_encoder(image)
        assert got.shape == want.shape and not torch.equal(got, want)
        assert torch.equal(h0.train().image_encoder(image), want)
