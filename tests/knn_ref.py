"""NumPy / float64 references of the k-NN evaluation (clip-lite_amd/knn.py, csrc/knn_ops.hip), shared by the wave-simulator and the GPU tests:
the selection is a stable argsort, the vote a float64 sum."""
import numpy as np

PRED = 5


def topk_ref(scores, k):
    """(top_s, top_i int32) [Q][min(k, N)]: the first k of np.argsort(-s, kind="stable") of every row (score descending, index ascending among
    equal scores, 0.0 == -0.0)."""
    scores = np.asarray(scores)
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(scores, order, 1), order.astype(np.int32)


def lattice(rng, rows, D=32, lo=-2, hi=2):
    """f32 [rows][D] with integer entries in [lo, hi]: every product and every sum of D of them is exact in f32."""
    return rng.integers(lo, hi + 1, (rows, D)).astype(np.float32)


def vote_ref(top_s, top_i, labels, C, ks, inv_T):
    """(scores float64 [nk][Q][C], pred int32 [nk][Q][5]): score[c] = sum over r < k with labels[top_i[r]] == c of exp((s_r - s_0) inv_T) in
    float64 on the given similarities and inv_T; pred = the best classes by (score descending, class ascending), -1 beyond C."""
    top_s = np.asarray(top_s, np.float64)
    top_i, labels = np.asarray(top_i), np.asarray(labels)
    Q = top_s.shape[0]
    w = np.exp((top_s - top_s[:, :1]) * float(inv_T))
    lab = labels[top_i]
    scores = np.zeros((len(ks), Q, C))
    pred = np.full((len(ks), Q, PRED), -1, np.int32)
    rows = np.arange(Q)
    for j, k in enumerate(ks):
        for r in range(k):
            np.add.at(scores[j], (rows, lab[:, r]), w[:, r])
        order = np.lexsort((np.broadcast_to(np.arange(C), (Q, C)), -scores[j]), axis=1)[:, :PRED]
        pred[j, :, :order.shape[1]] = order
    return scores, pred


def separated(scores, tol, ranks=PRED + 1):
    """bool [nk][Q]: the `ranks` highest class scores are pairwise more than tol relative apart, so a sum that is within tol / 2 of them ranks
    them the same way. Two classes that both score exactly 0 (no vote: exactly 0 in every precision, ranked by class) count as apart."""
    top = -np.sort(-scores, axis=-1)[..., :ranks]
    a, b = top[..., :-1], top[..., 1:]
    return np.all((a - b > tol * np.maximum(np.abs(a), np.abs(b))) | ((a == 0) & (b == 0)), axis=-1)


def clustered(seed, N, Q, D, C, noise):
    """Unit rows around C class centres: (bank f32 [N][D], bank labels int32 [N], queries f32 [Q][D], query labels int32 [Q])."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)

    def draw(n):
        y = rng.integers(0, C, n)
        x = centres[y] + noise / np.sqrt(D) * rng.standard_normal((n, D))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y.astype(np.int32)

    xb, yb = draw(N)
    xq, yq = draw(Q)
    return xb, yb, xq, yq


def knn_eval_ref(xb, yb, xq, yq, C, ks, temperature):
    """float64 k-NN evaluation: (scores [nk][Q][C], pred [nk][Q][5], {k: {"top1", "top5"}} in percent)."""
    s = np.asarray(xq, np.float64) @ np.asarray(xb, np.float64).T
    top_s, top_i = topk_ref(s, max(ks))
    scores, pred = vote_ref(top_s, top_i, yb, C, ks, 1.0 / temperature)
    acc = {}
    for j, k in enumerate(ks):
        acc[k] = {"top1": 100.0 * float(np.mean(pred[j, :, 0] == yq))}
        if C >= PRED:
            acc[k]["top5"] = 100.0 * float(np.mean((pred[j] == np.asarray(yq)[:, None]).any(1)))
    return scores, pred, acc


SELECTION_SHAPES = [(3, 700, 200), (2, 257, 256), (5, 33, 1), (1, 8, 8)]      # (Q, N, K)


def tie_scores(Q, N, D=32):
    """Integer-valued f32 scores [Q][N], the products of lattice vectors: a few dozen distinct values per row, so ties are everywhere."""
    rng = np.random.default_rng(1000 * Q + N)
    return lattice(rng, Q, D) @ lattice(rng, N, D).T


def feed(merge, s, K, chunk, pad=0, fill=1e30):
    """The running lists after feeding s [Q][N] to `merge(tile, lds, Q, Nc, base, K, have, top_s, top_i)` in chunks of `chunk` columns, each
    in a tile of row stride Nc + pad whose padding columns hold `fill`. Returns (top_s, top_i) [Q][min(K, N)]; the lists start as garbage."""
    Q, N = s.shape
    top_s = np.full((Q, K), -7.0, np.float32)
    top_i = np.full((Q, K), -7, np.int32)
    base = 0
    while base < N:
        nc = min(chunk, N - base)
        tile = np.full((Q, nc + pad), fill, np.float32)
        tile[:, :nc] = s[:, base:base + nc]
        merge(tile, nc + pad, Q, nc, base, K, min(K, base), top_s, top_i)
        base += nc
    return top_s[:, :min(K, N)], top_i[:, :min(K, N)]


def vote_inputs(seed, Q, K, N, C):
    """(top_s f32 [Q][K] descending in (0.2, 0.9), top_i int32 [Q][K] distinct rows of the bank, labels int32 [N])."""
    rng = np.random.default_rng(seed)
    top_s = -np.sort(-rng.uniform(0.2, 0.9, (Q, K)), axis=1)
    top_i = np.stack([rng.permutation(N)[:K] for _ in range(Q)])
    return top_s.astype(np.float32), top_i.astype(np.int32), rng.integers(0, C, N).astype(np.int32)
