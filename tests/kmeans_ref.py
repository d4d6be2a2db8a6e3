"""float64 NumPy reference of clip-lite_amd/kmeans.py (Lloyd's algorithm with the same initial centroids, tie rule, empty-cluster rule and
stop rule), so GPU tests need no scikit-learn. tests/test_kmeans_host.py pins it to sklearn.cluster.KMeans.

Also the derived bound on where an f32 assignment may differ from this one: with u = 2^-24 and gamma_D = D u / (1 - D u), the f32 value of
0.5 |c|^2 - x.c is off by at most gamma_D (|x| |c| + |c|^2) whatever the summation order, so a row may land on another centroid only if its
float64 gap between the best and the second-best value is below tau_n = 2 gamma_D (|x_n| max_k |c_k| + max_k |c_k|^2)."""
import numpy as np

U = 2.0 ** -24
EXEMPT_CAP = 0.01          # the share of rows under tau_n that a comparison may exempt


def gamma(n):
    return n * U / (1.0 - n * U)


def blobs(N, D, nblobs, sep, seed=0):
    """Unit-normalised Gaussian blobs x = normalize(sep * proto[label] + N(0, I)) as f32, and their labels."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((nblobs, D))
    label = rng.integers(0, nblobs, N)
    x = sep * proto[label] + rng.standard_normal((N, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), label


def init_rows(N, K, seed=1):
    """K distinct rows of a seeded permutation."""
    return np.random.default_rng(seed).permutation(N)[:K]


def assign_step(X, C):
    """(assign, dist, gap) in float64: argmin_k 0.5 |c_k|^2 - x.c_k with ties to the lower k; dist = max(0, |x|^2 + 2 v_min); gap = second-best
    value minus the best, over the distinct centroids."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    v = 0.5 * np.sum(C * C, axis=1)[None, :] - X @ C.T
    a = np.argmin(v, axis=1)
    best = v[np.arange(len(a)), a]
    dist = np.maximum(0.0, np.sum(X * X, axis=1) + 2.0 * best)
    # identical centroids give identical values in any arithmetic (the tie rule decides, in f32 as here): the gap is to the best DISTINCT one
    first = np.unique(C, axis=0, return_index=True)[1]
    if len(first) < 2:
        return a.astype(np.int64), dist, np.full(len(a), np.inf)
    two = np.partition(v[:, np.sort(first)], 1, axis=1)[:, :2]
    return a.astype(np.int64), dist, two[:, 1] - two[:, 0]


def tau(X, C):
    """tau_n of the module docstring for every row."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    cmax = np.sqrt(np.max(np.sum(C * C, axis=1)))
    return 2.0 * gamma(X.shape[1]) * (np.sqrt(np.sum(X * X, axis=1)) * cmax + cmax * cmax)


def exempt_rows(X, C, gap=None):
    """Boolean mask of the rows whose float64 gap is below tau_n: the only rows an f32 assignment may legitimately place elsewhere."""
    if gap is None:
        gap = assign_step(X, C)[2]
    return gap < tau(X, C)


def relocate(assign, dist, counts):
    """Empty clusters in ascending k; the i-th takes the row with the i-th largest dist (ties to the lower row), which leaves its old cluster."""
    out = assign.copy()
    empty = [k for k in range(len(counts)) if counts[k] == 0]
    taken = sorted(range(len(dist)), key=lambda n: (-dist[n], n))[:len(empty)] if empty else []
    for k, n in zip(empty, taken):
        out[n] = k
    return out


def means(X, assign, C_old):
    """float64 mean of every cluster's members; an empty cluster keeps its old centroid."""
    X = np.asarray(X, np.float64)
    C = np.array(C_old, np.float64, copy=True)
    for k in range(C.shape[0]):
        m = assign == k
        if m.any():
            C[k] = X[m].mean(axis=0)
    return C


def centroid_bound(X, assign, K):
    """Per cluster and component: (gamma_{n_k} + u) * mean over the members of |x_d|, the recursive-sum bound plus the division."""
    X = np.abs(np.asarray(X, np.float64))
    out = np.zeros((K, X.shape[1]))
    for k in range(K):
        m = assign == k
        if m.any():
            out[k] = (gamma(int(m.sum())) + U) * X[m].mean(axis=0)
    return out


def lloyd(X, C0, niter=200):
    """The driver's loop in float64. Returns centroids, assign, counts, inertia, iterations, history and max_exempt_share (the largest share of
    rows under tau_n at any assignment step of the run)."""
    X = np.asarray(X, np.float64)
    C = np.array(C0, np.float64, copy=True)
    K = C.shape[0]
    prev = np.full(X.shape[0], -1, np.int64)
    history, share, converged = [], 0.0, False
    for _ in range(niter):
        a, dist, gap = assign_step(X, C)
        share = max(share, float(np.mean(gap < tau(X, C))))
        history.append(float(dist.sum()))
        if not np.any(a != prev):
            converged = True
            break
        counts = np.bincount(a, minlength=K)
        if np.any(counts == 0):
            a = relocate(a, dist, counts)
        C = means(X, a, C)
        prev = a
    if not converged:
        a, dist, gap = assign_step(X, C)
        share = max(share, float(np.mean(gap < tau(X, C))))
    else:
        a = prev
    return {"centroids": C, "assign": a, "counts": np.bincount(a, minlength=K), "inertia": float(dist.sum()), "iterations": len(history),
            "history": history, "max_exempt_share": share}
