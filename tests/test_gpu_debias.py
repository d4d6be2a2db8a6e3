"""Bias evaluation on the MI355X (debias.py, csrc/debias_ops.hip): the principal directions and the streaming row pass against float64,
debias.evaluate on planted data against the float64 stable ranking, and bias_eval.py end to end.

Tolerances (debias_ref.pca_bars / rows_bars / cosine_bar, computed from the inputs when the test runs): 8 x the deviation from float64 of a
float32 NumPy evaluation of the same formulas (Gram matrix + eigh; dot, subtract, normalise) at exactly the test's inputs - the summation
order differs (wave tree against NumPy's pairwise sums), the arithmetic does not. One exception: the eigenvalue of the single pair
(P, D, R) = (1, 8, 1) is one 8-term dot product that NumPy happens to hit within 0.2 ulp (1.3e-8), so 8 x that is 1.0e-7, below one ulp
(1.19e-7), which is what the kernel's sum in another order is off by; a result one ulp off cannot be held to a bar below one ulp, so that
one bar is max(8 x measured, one ulp). V V^T - I has a second bar at every shape, 8 x the largest float32 NumPy figure of the shapes up to
P = 10 (1.6e-6): NumPy's rows at (64, 2048, 8) have no Gram-Schmidt pass behind them and would let a kernel without one through.
Measured float32 NumPy deviations at the test inputs (CPU):

    directions (P, D, R)   projector   V V^T - I   eigenvalues / largest
    (1, 8, 1)              5.2e-08     1.4e-07     1.3e-08
    (2, 8, 2)              5.7e-08     9.3e-08     2.3e-08
    (3, 8, 3)              8.6e-08     1.3e-07     7.0e-08
    (7, 136, 2)            8.8e-09     1.1e-07     2.4e-08
    (10, 512, 3)           8.6e-09     1.9e-07     1.1e-07
    (64, 2048, 8)          4.3e-07     2.5e-05     2.9e-08
    rows (N, D, R)         xn          xd          coef / |x|
    (1, 8, 1)              2.0e-08     1.8e-08     1.0e-08
    (5, 136, 2)            1.8e-08     2.1e-08     1.4e-08
    (1027, 2048, 1)        1.1e-08     1.3e-08     2.4e-08
    (33, 4096, 8)          6.3e-09     8.5e-09     2.0e-08
    evaluate, planted N = 1000, D = 512: cosines 7.1e-08 (bar 5.7e-07); smallest float64 rank gap 1.4e-05, so no entry is skipped
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import debias_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _pca(d, R):
    from clip_lite_amd import hip
    P, D = d.shape
    dd = torch.from_numpy(d).cuda()
    lam, V = torch.full((P,), -7.0, device="cuda"), torch.full((R, D), -7.0, device="cuda")
    work, info = torch.zeros(P * P, device="cuda"), torch.full((2,), -7, device="cuda", dtype=torch.int32)
    hip.debias_pca(dd, P, D, R, lam, V, work, info)
    return lam.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy()


def _rows(x, V, want=(True, True, True)):
    from clip_lite_amd import hip
    N, D = x.shape
    R = V.shape[0]
    xd_, vd = torch.from_numpy(x).cuda(), torch.from_numpy(V).cuda()
    outs = [torch.full((N, D), -7.0, device="cuda") if want[0] else None, torch.full((N, D), -7.0, device="cuda") if want[1] else None,
            torch.full((N, R), -7.0, device="cuda") if want[2] else None]
    hip.debias_rows(xd_, vd, N, D, R, *outs)
    return [None if o is None else o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("P,D,R", ref.PCA_SHAPES)
def test_directions_match_float64(P, D, R):
    d = ref.pair_diffs(P, D)
    lam, V, info = _pca(d, R)
    assert info[0] == 0 and 0 <= info[1] <= 30
    bars, base = ref.pca_bars(d, R)
    got = ref.pca_errors(d, R, lam, V)
    print(f"projector / orthonormality / eigenvalue error: kernel {got}, float32 NumPy {base}, bars {bars}, sweeps {info[1]}")
    for g, b in zip(got, bars):
        assert g <= b
    assert got[1] <= ref.orthonormality_bar()                           # the Gram-Schmidt pass: orthonormal to rounding at every shape
    assert np.all(np.diff(lam) <= 0) and np.all(lam >= 0)
    np.testing.assert_array_equal(V, ref.sign_rule(V))                  # the entry of largest magnitude of every row is positive
    lam2, V2, info2 = _pca(d, R)
    assert lam2.tobytes() == lam.tobytes() and V2.tobytes() == V.tobytes() and np.array_equal(info, info2)


def test_directions_refuse_a_direction_that_is_noise():
    """Rank-one differences with two components asked for: the second eigenvalue is rounding noise of the Gram matrix."""
    from clip_lite_amd import debias
    rng = np.random.default_rng(3)
    d = (rng.standard_normal((6, 1)) * rng.standard_normal((1, 64))).astype(np.float32)
    base = rng.standard_normal((6, 64)).astype(np.float32)
    a, b = torch.from_numpy(base + d).cuda(), torch.from_numpy(base).cuda()
    with pytest.raises(ValueError, match="span fewer than 2 directions"):
        debias.directions(a, b, 2)
    V, ratio = debias.directions(a, b, 1)
    want = ref.directions_ref((base + d).astype(np.float64) - base, 1)[1]
    assert abs(abs(float(V.cpu().numpy()[0].astype(np.float64) @ want[0])) - 1) < 1e-5 and ratio.shape == (1,) and float(ratio[0]) > 0.999
    with pytest.raises(ValueError, match=r"\[1, 6\] for 6 pairs"):
        debias.directions(a, b, 7)
    with pytest.raises(ValueError, match="at most 64 pairs"):
        debias.directions(torch.zeros(65, 64, device="cuda"), torch.zeros(65, 64, device="cuda"), 1)
    with pytest.raises(ValueError, match="not finite in f32"):           # finite embeddings whose squared differences overflow
        debias.directions(1e20 * a, b, 2)


@pytest.mark.parametrize("N,D,R", ref.ROWS_SHAPES)
def test_rows_match_float64(N, D, R):
    x, V, special = ref.rows_inputs(N, D, R)
    xn, xd, coef = _rows(x, V)
    bars, base = ref.rows_bars(x, V)
    got = ref.rows_errors(x, V, xn, xd, coef)
    print(f"xn / xd / coef error: kernel {got}, float32 NumPy {base}, bars {bars}")
    for g, b in zip(got, bars):
        assert g <= b
    bar = bars[1]
    keep = np.ones(N, bool)
    if "zero" in special:
        z, o = special["zero"], special["orthogonal"]
        keep[z] = False
        assert not xn[z].any() and not xd[z].any() and not coef[z].any()
        assert np.abs(xd[o] - xn[o]).max() <= bar                   # both within the bar of the same float64 row
    # |<e, v>| <= |e| |v| <= bar sqrt(D) for an error vector e with entries within the bar; the same bound for | |row| - 1 |
    assert np.abs(xd.astype(np.float64) @ V.astype(np.float64).T).max() <= bar * np.sqrt(D)
    for out in (xn, xd):
        assert np.abs(np.linalg.norm(out[keep].astype(np.float64), axis=1) - 1).max() <= bar * np.sqrt(D)
    for want in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:      # any output may be NULL; the others keep their bits (reruns)
        for got_, full in zip(_rows(x, V, want), (xn, xd, coef)):
            assert got_ is None or got_.tobytes() == full.tobytes()


@pytest.mark.parametrize("N,D,R", ref.ROWS_SHAPES)
def test_row_equal_to_a_component_leaves_nothing(N, D, R):
    """Components without any rounding (Hadamard rows over a power of two): a multiple of a component has coef = |x| and y = 0 exactly in
    every summation order, so xd is zero."""
    V = ref.exact_components(R, D)
    x = np.stack([4.0 * V[R - 1], -0.5 * V[0], V.sum(0)]).astype(np.float32)
    xn, xd, coef = _rows(x, V)
    assert not xd.any()
    want = np.zeros((3, R), np.float32)
    want[0, R - 1], want[1, 0], want[2] = 4.0, -0.5, 1.0
    np.testing.assert_array_equal(coef, want)
    np.testing.assert_array_equal(np.abs(coef[:2]).sum(1), np.linalg.norm(x[:2].astype(np.float64), axis=1).astype(np.float32))
    np.testing.assert_allclose(xn[0], V[R - 1], atol=1e-7)


def test_evaluate_on_planted_bias():
    """N = 1000, D = 512, groups of 600 / 400 whose means differ along a direction that the ten pairs also span, 4 prompts, k = 10."""
    from clip_lite_amd import debias
    feats, groups, a, b, prompts, w = ref.planted()
    k, G = 10, 2
    comps, ratio = debias.directions(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 1)
    V = comps.cpu().numpy()
    assert abs(float(V[0].astype(np.float64) @ w)) > 0.99 and 0.5 < float(ratio[0]) <= 1
    res = debias.evaluate(torch.from_numpy(feats).cuda(), torch.from_numpy(groups), torch.from_numpy(prompts).cuda(), comps, k, ratio.tolist())
    want, want_prior = ref.evaluate_ref(feats, groups, prompts, V, k)                # float64 on the components the GPU found
    bar = ref.cosine_bar(feats, V, prompts)
    size_prior = np.bincount(groups) / len(groups)
    skipped = total = 0
    for mode in ref.MODES:
        gs, gi = np.array(res["top_scores"][mode]), np.array(res["top_indices"][mode])
        ws, wi, wbank, all_s = want[mode]
        err = np.abs(gs - ws).max()
        print(f"{mode}: cosine error {err:.2e} (bar {bar:.2e})")
        assert err <= bar
        sure = ref.rank_gaps(all_s, groups, wi) > 4 * bar
        skipped += int((~sure).sum())
        total += sure.size
        np.testing.assert_array_equal(gi[sure], wi[sure])
        np.testing.assert_allclose(res["mean_alignment"][mode], ws.mean(-1), atol=bar, rtol=0)
        # the shares: against the float64 reference's own values, wherever its whole-bank ranking is as sure
        bank_sure = ref.rank_gaps(all_s, np.zeros_like(groups), wbank[:, None, :]) > 4 * bar
        if bank_sure.all():
            np.testing.assert_array_equal(np.array(res["share"][mode]), ref.shares(wbank, groups, G))
    print(f"skipped {skipped} of {total} entries")
    assert skipped <= 0.02 * total
    sb, sd = np.array(res["share"]["biased"]), np.array(res["share"]["debiased"])
    wb, wd = ref.shares(want["biased"][2], groups, G), ref.shares(want["debiased"][2], groups, G)
    fav = int(np.argmax(wb.mean(0) - size_prior))                                    # the group the float64 reference finds favoured
    for s_b, s_d in ((wb, wd), (sb, sd)):
        assert np.all(s_b[:, fav] > size_prior[fav])
        assert np.all(np.abs(s_d[:, fav] - size_prior[fav]) < np.abs(s_b[:, fav] - size_prior[fav]))
    # a mean of coefficients is within the coefficients' own bar (relative to |x|) times the longest row
    coef_bar = ref.rows_bars(feats, V)[0][2] * np.linalg.norm(feats.astype(np.float64), axis=1).max()
    np.testing.assert_allclose(res["prior"], want_prior, rtol=0, atol=coef_bar)
    assert res["group_sizes"] == [600, 400] and res["k"] == k and res["explained_variance_ratio"] == pytest.approx(ratio.tolist())
    with pytest.raises(ValueError, match="exceeds the smallest group's 2 images"):
        debias.evaluate(torch.from_numpy(feats[:6]).cuda(), [0, 1, 1, 0, 1, 1], torch.from_numpy(prompts).cuda(), comps, 3)
    with pytest.raises(ValueError, match="8 features, the images 512"):
        debias.evaluate(torch.from_numpy(feats).cuda(), groups, torch.zeros(1, 8, device="cuda"), comps, k)


def test_bias_eval_cli_end_to_end(tmp_path):
    """bias_eval.py in a fresh process: random weights, the synthetic two-group source, two prompts."""
    out = os.path.join(str(tmp_path), "bias.json")
    cmd = [sys.executable, os.path.join(ROOT, "bias_eval.py"), "--config", os.path.join(ROOT, "configs", "smoke_random.yaml"),
           "--config-override", "MODEL.VISUAL.NETWORK_NAME", "resnet18", "MODEL.VISUAL.FEATURE_SIZE", "512", "MODEL.TEXTUAL.NUM_HIDDEN_LAYERS", "2",
           "--down-config", os.path.join(ROOT, "configs", "downstream_bias.yaml"), "--weight-init", "random", "--split", "val",
           "--query", "a doctor", "a person cooking", "--num-results", "5", "--cpu-workers", "0", "--output", out,
           "--checkpoints-dir", os.path.join(str(tmp_path), "logs") + "/"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(out) as fh:
        res = json.load(fh)
    printed = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert printed and json.loads(printed[-1]) == res
    assert set(res) == {"k", "num_groups", "num_images", "group_sizes", "prior", "explained_variance_ratio", "mean_alignment", "share", "top_scores",
                        "top_indices", "prompts", "groups", "pairs"}
    assert res["k"] == 5 and res["num_groups"] == 2 and res["num_images"] == 500 and sum(res["group_sizes"]) == 500
    assert res["prompts"] == ["a doctor", "a person cooking"] and res["groups"] == ["class_0", "class_1"] and len(res["pairs"]) == 10
    assert len(res["prior"]) == 2 and len(res["explained_variance_ratio"]) == 1 and 0 < res["explained_variance_ratio"][0] <= 1
    for key in ("mean_alignment", "share"):
        for mode in ref.MODES:
            m = np.array(res[key][mode])
            assert m.shape == (2, 2) and np.all(np.isfinite(m))
    for mode in ref.MODES:
        assert np.allclose(np.array(res["share"][mode]).sum(1), 1) and np.array(res["top_indices"][mode]).shape == (2, 2, 5)
        assert np.all(np.abs(np.array(res["top_scores"][mode])) <= 1 + 1e-5)
    assert "Mean Alignment | class_0 | Biased:" in r.stdout and "prompt 'a doctor'" in r.stdout
