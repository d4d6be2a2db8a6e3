"""Generate tests/golden/debias_small.npz by running the REFERENCE's utils/we.py (doPCA, drop) on seeded embeddings:

    python tests/golden/make_debias_golden.py <reference checkout>

Run where the reference and scikit-learn exist; the tests only read the committed .npz. Nothing of the reference's source is copied: the fixture
holds the seeded inputs (float64 embeddings of P word pairs whose differences have singular values 3, 3/2, 3/4, ...: well-separated
components) and the reference's numeric outputs (`doPCA(...).components_`, `.explained_variance_ratio_`, `drop(u, v)`)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import debias_ref  # noqa: E402

CASES = [(10, 512), (3, 8)]                 # (P, D)


class _Embedding:
    """What doPCA needs of the reference's WordEmbedding: v(word)."""

    def __init__(self, vectors):
        self.vectors = vectors

    def v(self, word):
        return self.vectors[word]


def main(reference):
    sys.path.insert(0, reference)
    from utils import we
    out = {}
    for P, D in CASES:
        rng = np.random.default_rng(5000 + P)
        d = debias_ref.pair_diffs(P, D).astype(np.float64)
        centre = rng.standard_normal((P, D))
        a, b = centre + d / 2, centre - d / 2
        vectors = {f"a{i}": a[i] for i in range(P)}
        vectors.update({f"b{i}": b[i] for i in range(P)})
        pca = we.doPCA([(f"a{i}", f"b{i}") for i in range(P)], _Embedding(vectors), num_components=P)
        u, v = rng.standard_normal(D), pca.components_[0] * 1.7        # drop() divides by v.v: a direction of any length
        key = f"p{P}_d{D}"
        out.update({f"{key}_a": a, f"{key}_b": b, f"{key}_components": pca.components_, f"{key}_ratio": pca.explained_variance_ratio_,
                    f"{key}_u": u, f"{key}_v": v, f"{key}_drop": we.drop(u, v)})
    path = os.path.join(HERE, "debias_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
