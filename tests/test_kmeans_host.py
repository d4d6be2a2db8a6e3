"""CPU-side checks of the k-means driver's host logic: tests/kmeans_ref.py (the float64 reference every GPU test compares against) pinned to
scikit-learn's Lloyd iteration, the empty-cluster rule of the driver and of the reference on the same inputs, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import kmeans_ref as R


def test_reference_matches_sklearn_lloyd_on_separated_blobs():
    sk = pytest.importorskip("sklearn.cluster")
    N, D, K = 3000, 32, 6
    X, _ = R.blobs(N, D, K, 1.5, seed=0)
    X = X.astype(np.float64)
    C0 = X[R.init_rows(N, K, seed=1)]
    want = sk.KMeans(n_clusters=K, init=C0, n_init=1, algorithm="lloyd", tol=0, max_iter=200).fit(X)
    got = R.lloyd(X, C0, niter=200)
    assert got["iterations"] < 200
    np.testing.assert_array_equal(got["assign"], want.labels_)
    np.testing.assert_allclose(got["centroids"], want.cluster_centers_, rtol=0, atol=1e-12)
    assert abs(got["inertia"] - want.inertia_) <= 1e-9 * want.inertia_
    assert all(b <= a * (1 + 1e-12) for a, b in zip(got["history"], got["history"][1:]))


def test_assign_step_ties_go_to_the_lower_centroid():
    X = np.eye(4, 8)
    C = np.stack([X[1], X[1], X[0], X[0]])                  # duplicated centroids
    a, dist, gap = R.assign_step(X, C)
    assert list(a[:2]) == [2, 0] and dist[0] == 0 and gap[0] == 1.0          # the gap is to the best DISTINCT centroid


def test_relocation_rule_driver_and_reference_agree():
    from clip_lite_amd.kmeans import relocate
    rng = np.random.default_rng(0)
    for _ in range(20):
        N, K = 50, 7
        assign = rng.integers(0, K, N)
        assign[np.isin(assign, [1, 4, 5])] = 0
        dist = rng.integers(0, 6, N).astype(np.float32)          # many ties: the lower row wins
        counts = np.bincount(assign, minlength=K)
        a1 = relocate(assign.astype(np.int32), dist, counts)
        a2 = R.relocate(assign, dist, counts)
        np.testing.assert_array_equal(a1, a2)
        moved = np.flatnonzero(a1 != assign)
        assert len(moved) == 3 and sorted(a1[moved]) == [1, 4, 5]
        far = sorted(range(N), key=lambda n: (-dist[n], n))[:3]
        assert [int(a1[n]) for n in far] == [1, 4, 5]            # ascending k takes descending distance
    a = np.array([0, 0, 1], np.int32)
    np.testing.assert_array_equal(relocate(a, np.zeros(3, np.float32), np.array([2, 1])), a)       # nothing empty: untouched


def test_reference_refills_an_emptied_cluster():
    """K identical rows among the initial centroids: every tie goes to the lowest k, the others start empty and are relocated"""
    X, _ = R.blobs(400, 16, 4, 2.0, seed=3)
    C0 = np.repeat(X[:1], 4, axis=0)
    out = R.lloyd(X, C0)
    assert out["counts"].min() > 0 and out["iterations"] < 200


def test_init_rows_are_distinct_and_seeded():
    from clip_lite_amd.kmeans import init_rows
    a, b, c = init_rows(1000, 64, 7), init_rows(1000, 64, 7), init_rows(1000, 64, 8)
    assert torch.equal(a, b) and not torch.equal(a, c) and len(set(a.tolist())) == 64


def test_fit_refuses_cpu_tensors_and_bad_shapes():
    from clip_lite_amd import kmeans
    with pytest.raises(RuntimeError, match="GPU"):
        kmeans.fit(torch.zeros(16, 8), 2)
    with pytest.raises(ValueError):
        kmeans.fit(torch.zeros(16, 12), 2)
    with pytest.raises(ValueError):
        kmeans.fit(torch.zeros(16, 8), 1)
    with pytest.raises(ValueError):
        kmeans.fit(torch.zeros(4, 8), 5)
    with pytest.raises(ValueError):
        kmeans.fit(torch.zeros(16, 8, dtype=torch.float64), 2)
