"""The float64 references of the bias evaluation (tests/debias_ref.py) against the reference's own utils/we.py, recorded in
tests/golden/debias_small.npz (tests/golden/make_debias_golden.py: doPCA's sklearn components and explained-variance ratios, drop), and the
reference module's own invariants. Runs without a GPU."""
import os

import numpy as np
import pytest

import debias_ref as ref

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debias_small.npz"))


@pytest.mark.parametrize("P,D", [(10, 512), (3, 8)])
def test_directions_are_the_reference_pca(P, D):
    """we.doPCA fits sklearn's PCA to the 2 P pair-centred rows; their column mean is zero, so its components are the right singular vectors of
    the pair differences. The projector onto the first R of them (the span is what the evaluation uses) agrees within 1e-12."""
    key = f"p{P}_d{D}"
    diffs = G[f"{key}_a"] - G[f"{key}_b"]
    want_v, want_ratio = G[f"{key}_components"], G[f"{key}_ratio"]
    for R in range(1, min(P, 8) + 1):
        lam, V, ratio = ref.directions_ref(diffs, R)
        assert np.abs(ref.projector(V) - ref.projector(want_v[:R])).max() <= 1e-12
        assert np.abs(ratio - want_ratio[:R]).max() <= 1e-12
        np.testing.assert_array_equal(V, ref.sign_rule(V))
        assert np.abs(np.abs((V * want_v[:R]).sum(1)) - 1).max() <= 1e-12          # row by row, up to the sign


@pytest.mark.parametrize("P,D", [(10, 512), (3, 8)])
def test_drop_and_the_row_pass_are_the_reference_drop(P, D):
    key = f"p{P}_d{D}"
    u, v, want = G[f"{key}_u"], G[f"{key}_v"], G[f"{key}_drop"]
    assert np.abs(ref.drop(u, v) - want).max() <= 1e-12
    unit = (v / np.linalg.norm(v))[None, :]
    xn, xd, coef = ref.rows_ref(u[None, :], unit)
    assert np.abs(xd[0] - want / np.linalg.norm(want)).max() <= 1e-12              # the row pass: drop, then F.normalize
    assert np.abs(xn[0] - u / np.linalg.norm(u)).max() <= 1e-12 and abs(coef[0, 0] - u @ unit[0]) <= 1e-12


def test_row_pass_edge_cases_in_float64():
    V = ref.exact_components(2, 16).astype(np.float64)
    x = np.stack([np.zeros(16), 3 * V[1], np.eye(16)[9]])
    xn, xd, coef = ref.rows_ref(x, V)
    assert not xn[0].any() and not xd[0].any()                                      # F.normalize's max(|x|, 1e-12): 0 / 1e-12
    assert not xd[1].any() and coef[1, 1] == 3.0                                    # a row along a component leaves nothing
    np.testing.assert_array_equal(xd[2], xn[2])                                     # an orthogonal row is untouched


def test_exact_components_are_orthonormal_without_rounding():
    for R, D in ((1, 8), (2, 136), (4, 8), (8, 4096)):
        V = ref.exact_components(R, D)
        assert V.dtype == np.float32
        np.testing.assert_array_equal(V @ V.T, np.eye(R, dtype=np.float32))


def test_planted_reference_stays_under_the_skip_cap_and_shows_the_bias():
    """The planted data of tests/test_gpu_debias.py, in float64 alone: at most 2 % of the (mode, prompt, group, rank) entries have a
    neighbour within 4 x the cosine bar, the favoured group's biased share exceeds its prior, and the debiased share is closer to it."""
    feats, groups, a, b, prompts, w = ref.planted()
    _, V, _ = ref.directions_ref(a.astype(np.float64) - b.astype(np.float64), 1)
    assert abs(float(V[0] @ w)) > 0.99                                              # the pairs span the planted direction
    out, prior = ref.evaluate_ref(feats, groups, prompts, V, 10)
    bar = ref.cosine_bar(feats, V.astype(np.float32), prompts)
    skipped = total = 0
    for mode in ref.MODES:
        gaps = ref.rank_gaps(out[mode][3], groups, out[mode][1])
        skipped += int((gaps <= 4 * bar).sum())
        total += gaps.size
    assert total == 2 * 4 * 2 * 10 and skipped <= 0.02 * total
    size_prior = np.bincount(groups) / len(groups)
    sb, sd = ref.shares(out["biased"][2], groups, 2), ref.shares(out["debiased"][2], groups, 2)
    assert np.all(sb[:, 0] > size_prior[0])
    assert np.all(np.abs(sd[:, 0] - size_prior[0]) < np.abs(sb[:, 0] - size_prior[0]))
    assert prior[0] > 0 > prior[1] or prior[0] < 0 < prior[1]                       # the groups sit on opposite sides of the direction
