"""Writes tests/golden/ease_golden.npz from numpy alone: a 60 x 40 weighted matrix X, lambda, the float64 EASE weights B and
the float64 top-5 (liked items filtered) of ten users.

    python tests/golden/make_ease_golden.py

The fixture is chosen so that a float32 fit cannot reorder the top-5: for each of the ten users the float64 gap between
neighbouring scores down to the boundary (rank 5 against rank 6 included) exceeds 2 d_ref ||B|| ||x||, d_ref being the
relative distance of LAPACK-fp32's B from the float64 one.  The script asserts it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ease_reference as ref  # noqa: E402

USERS, ITEMS, REG, TOP, N_USERS = 60, 40, 5.0, 5, 10


def build(seed):
    rng = np.random.default_rng(seed)
    X = np.where(rng.random((USERS, ITEMS)) < 0.2, 1.0 + np.rint(8 * rng.random((USERS, ITEMS))) / 2, 0.0).astype(np.float32)
    B = ref.ease64(X, REG)
    B32 = ref.weights32(ref.lapack32_inverse(ref.gram64(X, REG).astype(np.float32)))
    d_ref = ref.rel_distance(B32, B)
    users = np.arange(N_USERS, dtype=np.int32)
    ids = np.empty((N_USERS, TOP), dtype=np.int32)
    scores = np.empty((N_USERS, TOP), dtype=np.float64)
    ok = True
    for r, u in enumerate(users):
        x = X[u].astype(np.float64)
        s = x @ B
        s[x != 0] = -np.inf
        order = np.argsort(-s, kind="stable")
        ids[r], scores[r] = order[:TOP], s[order[:TOP]]
        gaps = -np.diff(s[order[:TOP + 1]])
        ok &= bool(np.isfinite(gaps).all() and gaps.min() > 2 * d_ref * np.linalg.norm(B) * np.linalg.norm(x))
    return ok, dict(X=X, regularization=np.float64(REG), B=B, users=users, top_ids=ids, top_scores=scores)


def main():
    for seed in range(100):
        ok, data = build(seed)
        if ok:
            break
    assert ok, "no seed separates the top-5 of all ten users"
    np.savez_compressed(os.path.join(HERE, "ease_golden.npz"), seed=np.int64(seed), **data)
    print("seed", seed, os.path.getsize(os.path.join(HERE, "ease_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
