"""NumPy references of the bias evaluation (clip-lite_amd/debias.py, csrc/debias_ops.hip), shared by the host, wave-simulator and GPU tests:
float64 for the truth, and a float32 evaluation of the same formulas whose distance from float64 sets the kernels' tolerances (8 x)."""
import functools

import numpy as np

PCA_SHAPES = [(1, 8, 1), (2, 8, 2), (3, 8, 3), (7, 136, 2), (10, 512, 3), (64, 2048, 8)]           # (P, D, R)
ROWS_SHAPES = [(1, 8, 1), (5, 136, 2), (1027, 2048, 1), (33, 4096, 8)]                              # (N, D, R)
FACTOR = 8                                  # kernel tolerance = FACTOR x the float32 NumPy evaluation's measured deviation from float64
ULP32 = 2.0 ** -23                          # one unit in the last place of a float32 result, relative
MODES = ("biased", "debiased")


# ------------------------------------------------------------------------------------------------ directions
def sign_rule(V):
    """Rows signed so that the entry of largest magnitude (lowest index among equal ones) is positive."""
    V = np.array(V, copy=True)
    for r in V:
        if r[np.argmax(np.abs(r))] < 0:
            r *= -1
    return V


def directions_ref(diffs, R):
    """(eigvals [P] descending, components [R][D], explained_variance_ratio [R]) in float64: the squared singular values and the right
    singular vectors of diffs, which are sklearn's PCA of the 2 P rows +-d_i / 2 (zero column mean)."""
    d = np.asarray(diffs, np.float64)
    _, s, vt = np.linalg.svd(d, full_matrices=False)
    lam = s * s
    return lam, sign_rule(vt[:R]), lam[:R] / lam.sum()


def directions_f32(diffs, R):
    """The kernel's formulas in float32 NumPy: Gram matrix, eigh, diffs^T u_j normalised. (eigvals, components)."""
    d = np.asarray(diffs, np.float32)
    lam, U = np.linalg.eigh(d @ d.T)
    order = np.argsort(-lam, kind="stable")
    lam, U = lam[order], U[:, order]
    V = (U[:, :R].T @ d).astype(np.float32)
    V /= np.linalg.norm(V, axis=1, keepdims=True).astype(np.float32)
    return np.maximum(lam, 0), sign_rule(V)


def projector(V):
    V = np.asarray(V, np.float64)
    return V.T @ V


def pair_diffs(P, D, seed=0, ratio=0.5):
    """f32 [P][D] with singular values ratio^0, ratio^1, ...: well-separated components."""
    rng = np.random.default_rng(1000 * P + D + seed)
    u, _ = np.linalg.qr(rng.standard_normal((P, P)))
    v, _ = np.linalg.qr(rng.standard_normal((D, P)))
    return ((u * ratio ** np.arange(P)) @ v.T * 3.0).astype(np.float32)


def pca_errors(diffs, R, lam, V):
    """(projector error, orthonormality error, eigenvalue error relative to the largest) of a result against float64."""
    lam64, V64, _ = directions_ref(diffs, R)
    V = np.asarray(V, np.float64)
    return (np.abs(projector(V) - projector(V64)).max(), np.abs(V @ V.T - np.eye(R)).max(),
            np.abs(np.asarray(lam, np.float64) - lam64).max() / lam64[0])


def pca_bars(diffs, R):
    """(bars, measured): the kernel's tolerances for pca_errors' three figures = FACTOR x the float32 NumPy evaluation's errors at the same
    input. One exception, the eigenvalue of a single pair (P = 1): it is one dot product, 8 terms at D = 8, which NumPy happens to hit within
    0.2 ulp (1.3e-8), so FACTOR x that is below one ulp, while a correct f32 sum in another order may be one ulp off; a result one ulp off
    cannot be held to a bar below one ulp, so that bar is max(FACTOR x measured, one ulp)."""
    measured = pca_errors(diffs, R, *directions_f32(diffs, R))
    bars = [FACTOR * m for m in measured]
    if np.asarray(diffs).shape[0] == 1:
        bars[2] = max(bars[2], ULP32)
    return tuple(bars), measured


@functools.lru_cache(maxsize=None)
def orthonormality_bar():
    """A second bar for V V^T - I at every shape. The float32 NumPy evaluation has no Gram-Schmidt pass, so at (64, 2048, 8) its rows are only
    orthogonal to 2.5e-5 and pca_bars' figure there would not notice a kernel without the pass; at the shapes up to P = 10 its rows are
    orthonormal to rounding (9e-8 .. 1.9e-7), which is what the kernel promises at every shape: FACTOR x the largest of those."""
    return FACTOR * max(pca_errors(pair_diffs(P, D), R, *directions_f32(pair_diffs(P, D), R))[1] for P, D, R in PCA_SHAPES if P <= 10)


# ------------------------------------------------------------------------------------------------ rows
def drop(u, v):
    """u with its part along v removed (v of any length)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return u - v * (u @ v) / (v @ v)


def _normalize(x, eps):
    n = np.sqrt((x * x).sum(1, keepdims=True))
    return x / np.maximum(n, eps)


def rows_ref(x, V, dtype=np.float64):
    """(xn, xd, coef) in `dtype` (float64: the truth; float32: the kernel's formulas in NumPy's summation order)."""
    x, V = np.asarray(x, dtype), np.asarray(V, dtype)
    eps = dtype(1e-12)
    coef = x @ V.T
    y = x - coef @ V
    return _normalize(x, eps), _normalize(y, eps), coef


def exact_components(R, D):
    """f32 [R][D], orthonormal with no rounding at all: rows of a Hadamard matrix of order 4 (x 1/2) or 16 (x 1/4) on the first entries, so
    that every product and every partial sum with a row whose entries are small integers over a power of two is exact in f32."""
    n = 4 if R <= 4 else 16
    assert R <= n <= D
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    V = np.zeros((R, D), np.float32)
    V[:, :n] = H[:R] / np.sqrt(n)
    return V


def random_components(R, D, rng):
    """f32 [R][D], orthonormal to f32 rounding."""
    q, _ = np.linalg.qr(rng.standard_normal((D, R)))
    return np.ascontiguousarray(q.T).astype(np.float32)


def rows_inputs(N, D, R):
    """(x f32 [N][D], V f32 [R][D], special: {name: row}): rows of norm about 3 sqrt(D); where N allows, a zero row and a row orthogonal to
    every component (to f32 rounding)."""
    rng = np.random.default_rng(77 * N + D + R)
    V = random_components(R, D, rng)
    x = (3.0 * rng.standard_normal((N, D))).astype(np.float32)
    special = {}
    if N >= 3:
        special["zero"] = N - 1
        x[N - 1] = 0
        y = x[N - 2].astype(np.float64)
        V64 = V.astype(np.float64)
        for _ in range(2):
            y = y - (y @ V64.T) @ np.linalg.inv(V64 @ V64.T) @ V64
        x[N - 2] = y.astype(np.float32)
        special["orthogonal"] = N - 2
    return x, V, special


def rows_errors(x, V, xn, xd, coef):
    """Largest deviations from float64: (xn, xd, coef relative to |x|)."""
    rn, rd, rc = rows_ref(x, V)
    norm = np.maximum(np.sqrt((np.asarray(x, np.float64) ** 2).sum(1, keepdims=True)), 1e-300)
    return np.abs(xn - rn).max(), np.abs(xd - rd).max(), (np.abs(coef - rc) / norm).max()


def rows_bars(x, V):
    """(bars, measured) for rows_errors' three figures: FACTOR x the float32 NumPy evaluation's errors at the same input."""
    measured = rows_errors(x, V, *rows_ref(x, V, np.float32))
    return tuple(FACTOR * m for m in measured), measured


# ------------------------------------------------------------------------------------------------ evaluate
def topk_ref(scores, k):
    """The first k of a stable argsort of every row, highest first (knn_ref.topk_ref)."""
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(scores, order, 1), order


def evaluate_ref(feats, groups, prompts, V, k):
    """float64 evaluation. {mode: (group_scores [Q][G][k], group_indices [Q][G][k], bank_indices [Q][k], all scores [Q][N])}, prior [G]."""
    groups = np.asarray(groups)
    G = int(groups.max()) + 1
    xn, xd, coef = rows_ref(feats, V)
    q = np.asarray(prompts, np.float64)
    out = {}
    for mode, bank in zip(MODES, (xn, xd)):
        s = q @ bank.T
        gs, gi = [], []
        for g in range(G):
            idx = np.flatnonzero(groups == g)
            ts, ti = topk_ref(s[:, idx], k)
            gs.append(ts)
            gi.append(idx[ti])
        out[mode] = (np.stack(gs, 1), np.stack(gi, 1), topk_ref(s, k)[1], s)
    return out, np.array([coef[groups == g, 0].mean() for g in range(G)])


def cosine_bar(feats, V, prompts):
    """The tolerance of evaluate's cosines: FACTOR x the deviation from float64 of the float32 NumPy evaluation (row pass, then the product
    with the prompts) at the same inputs."""
    q = np.asarray(prompts, np.float64)
    exact, single = rows_ref(feats, V), rows_ref(feats, V, np.float32)
    return FACTOR * max(np.abs(np.asarray(prompts, np.float32) @ single[m].T - q @ exact[m].T).max() for m in (0, 1))


def shares(bank_indices, groups, G):
    return np.array([[np.mean(np.asarray(groups)[row] == g) for g in range(G)] for row in bank_indices])


def planted(seed=0, N=1000, D=512, sizes=(600, 400), P=10, Q=4, offset=6.0):
    """Planted bias: (feats f32 [N][D], groups [N], pairs a, b f32 [P][D], prompts f32 [Q][D] unit rows, direction f64 [D]). The group means
    differ by `offset` along a unit direction that the pair differences also share (plus smaller independent parts); every prompt leans
    towards the direction's positive side, which is group 0's."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(D)
    w /= np.linalg.norm(w)
    groups = np.repeat(np.arange(len(sizes)), sizes)
    groups = groups[rng.permutation(N)]
    feats = rng.standard_normal((N, D)) + np.where(groups == 0, 0.5, -0.5)[:, None] * offset * w
    base = rng.standard_normal((P, D))
    a = base + (1.0 + 0.2 * rng.random((P, 1))) * w + 0.01 * rng.standard_normal((P, D))
    b = base - (1.0 + 0.2 * rng.random((P, 1))) * w + 0.01 * rng.standard_normal((P, D))
    prompts = rng.standard_normal((Q, D)) + 4.0 * w
    prompts /= np.linalg.norm(prompts, axis=1, keepdims=True)
    return feats.astype(np.float32), groups, a.astype(np.float32), b.astype(np.float32), prompts.astype(np.float32), w


def rank_gaps(all_scores, groups, group_indices):
    """For every (prompt, group, rank) entry of the float64 group lists: the float64 gap to both neighbours in the group's full ranking
    (inf at the top)."""
    groups = np.asarray(groups)
    Q, G, k = group_indices.shape
    gaps = np.empty((Q, G, k))
    for g in range(G):
        idx = np.flatnonzero(groups == g)
        s = -np.sort(-all_scores[:, idx], axis=1)[:, :k + 1]
        up = np.concatenate([np.full((Q, 1), np.inf), s[:, :k - 1] - s[:, 1:k]], 1)
        down = s[:, :k] - s[:, 1:k + 1] if s.shape[1] > k else np.concatenate([s[:, :k - 1] - s[:, 1:k], np.full((Q, 1), np.inf)], 1)
        gaps[:, g] = np.minimum(up, down)
    return gaps
