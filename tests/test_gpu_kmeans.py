"""GPU checks of clip_lite_amd/kmeans.py against the float64 reference tests/kmeans_ref.py. Where an f32 assignment may differ from float64
is derived there (tau_n); every comparison exempts exactly the rows under tau_n, prints their share and caps it at 1 % of N."""
import time

import numpy as np
import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu


def _exempt(X, C, gap=None):
    ex = R.exempt_rows(X, C, gap)
    share = float(ex.mean())
    print(f"rows under tau_n: {100 * share:.4f} % of {len(ex)}")
    assert share <= R.EXEMPT_CAP
    return ex


def _check_means(X, assign, K, C_got, C_old):
    want = R.means(X, assign, C_old)
    err = np.abs(np.asarray(C_got, np.float64) - want)
    bound = R.centroid_bound(X, assign, K)
    assert np.all(err <= bound), float((err - bound).max())


@pytest.mark.parametrize("K,nblobs,sep", [(10, 10, 0.15), (64, 40, 0.1)])
def test_one_lloyd_step_matches_float64(K, nblobs, sep):
    from clip_lite_amd import kmeans
    N, D = 20000, 768
    X, _ = R.blobs(N, D, nblobs, sep, seed=0)
    rows = X[R.init_rows(N, K, seed=1)]
    # the given centroids: the means after one float64 step from the seeded rows (raw unit rows as centroids put tau_n, which grows with
    # max |c|, above the gap of 1.28 % of the rows at K = 64: over the cap before any kernel has run)
    C0 = R.means(X, R.assign_step(X, rows)[0], rows).astype(np.float32)
    st = kmeans._State(torch.from_numpy(X).cuda(), K)
    st.set_centroids(torch.from_numpy(C0).cuda())
    st.assign_step()
    st.accumulate()
    st.update()
    a = st.assign.cpu().numpy()
    a64, d64, gap = R.assign_step(X, C0)
    ex = _exempt(X, C0, gap)
    np.testing.assert_array_equal(a[~ex], a64[~ex])
    assert int(st.stat[K]) == N                                                   # every row moved from "unassigned"
    np.testing.assert_array_equal(st.stat[:K].cpu().numpy(), np.bincount(a, minlength=K))
    _check_means(X, a, K, st.C[:K].cpu().numpy(), C0)                             # the mean of the member set the GPU chose
    np.testing.assert_allclose(st.dist.cpu().numpy()[~ex], d64[~ex], rtol=0, atol=8 * R.gamma(D))       # unit rows, see tests/test_wavesim_kmeans.py
    assert abs(float(st.inertia.item()) - float(st.dist.double().sum().item())) <= R.gamma(256) * float(d64.sum())


def test_full_fit_on_a_separated_problem_equals_the_reference():
    from clip_lite_amd import kmeans
    N, D, K = 3000, 32, 6                          # settled with kmeans_ref on the CPU: 5 iterations, no row under tau_n at any of them
    X, _ = R.blobs(N, D, 6, 2.0, seed=2)
    C0 = X[R.init_rows(N, K, seed=102)]
    ref = R.lloyd(X, C0)
    print(f"reference: {ref['iterations']} iterations, largest share under tau_n at any step {100 * ref['max_exempt_share']:.4f} %")
    assert ref["max_exempt_share"] == 0.0          # precondition: no boundary row at any iteration, so labels must be equal
    out = kmeans.fit(torch.from_numpy(X).cuda(), K, init=torch.from_numpy(C0))
    np.testing.assert_array_equal(out["assign"].cpu().numpy(), ref["assign"])
    assert out["iterations"] == ref["iterations"]
    _check_means(X, ref["assign"], K, out["centroids"].cpu().numpy(), C0)
    assert abs(out["inertia"] - ref["inertia"]) <= 8 * R.gamma(D) * N


def test_full_fit_on_a_hard_problem_is_a_fixed_point():
    from clip_lite_amd import kmeans
    N, D, K = 20000, 768, 10
    X, _ = R.blobs(N, D, 1, 0.0, seed=0)
    C0 = X[R.init_rows(N, K, seed=1)]
    out = kmeans.fit(torch.from_numpy(X).cuda(), K, init=torch.from_numpy(C0))
    C, a = out["centroids"].cpu().numpy(), out["assign"].cpu().numpy()
    print(f"iterations {out['iterations']}, inertia {out['inertia']:.6f}, smallest cluster {int(out['counts'].min())}")
    assert out["iterations"] < 200
    a64, d64, gap = R.assign_step(X, C)
    ex = _exempt(X, C, gap)
    np.testing.assert_array_equal(a[~ex], a64[~ex])
    _check_means(X, a, K, C, C0)
    assert int(out["counts"].min()) > 0
    h = out["history"]
    assert all(b <= a_ + R.gamma(D) * a_ for a_, b in zip(h, h[1:]))
    ref = R.lloyd(X, C0)
    print(f"float64 reference: {ref['iterations']} iterations, inertia {ref['inertia']:.6f} (not asserted: two runs that part at one boundary "
          f"row end in different local minima)")


def test_emptied_clusters_are_relocated_like_the_reference():
    from clip_lite_amd import kmeans
    N, D, K = 3000, 32, 6                          # settled with kmeans_ref on the CPU: 15 iterations, no row under tau_n at any of them
    X, _ = R.blobs(N, D, 6, 2.0, seed=2)
    C0 = np.repeat(X[:1], K, axis=0)               # K identical rows: every tie goes to k = 0, five clusters start empty
    ref = R.lloyd(X, C0)
    print(f"reference: {ref['iterations']} iterations, largest share under tau_n {100 * ref['max_exempt_share']:.4f} %")
    assert ref["max_exempt_share"] == 0.0 and ref["counts"].min() > 0
    out = kmeans.fit(torch.from_numpy(X).cuda(), K, init=torch.from_numpy(C0))
    np.testing.assert_array_equal(out["assign"].cpu().numpy(), ref["assign"])
    assert out["iterations"] == ref["iterations"]
    _check_means(X, ref["assign"], K, out["centroids"].cpu().numpy(), C0)


@pytest.mark.parametrize("K", [10, 256])
def test_coco_scale_runs_are_bit_identical(K):
    from clip_lite_amd import hip, kmeans
    N, D = 118287, 768
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(N, D, device="cuda", generator=g)
    X = X / X.norm(dim=1, keepdim=True)
    niter = 6
    runs = []
    for det in (False, False, True):
        hip.set_deterministic(det)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = kmeans.fit(X, K, niter=niter, seed=1234)
            dt = time.perf_counter() - t0
        finally:
            hip.set_deterministic(False)
        print(f"K = {K}, deterministic = {det}: {1e3 * dt / (out['iterations'] + 1):.2f} ms per iteration (wall, host loop included)")
        runs.append(out)
    for other in runs[1:]:
        assert torch.equal(other["assign"], runs[0]["assign"])
        assert torch.equal(other["centroids"].view(torch.int32), runs[0]["centroids"].view(torch.int32))
        assert other["history"] == runs[0]["history"]
    assert int(runs[0]["counts"].sum()) == N
