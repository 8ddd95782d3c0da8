"""Numpy restatement of AlternatingLeastSquares.explain / explain_batch, written from the arithmetic and pinned to
the reference's own output by tests/golden/explain_golden.npz (tests/test_explain_host.py).  Host arrays in, host arrays out;
nothing of the package under test is imported.

For one user with CSR row (j, c_j), `alpha` already applied, item factors Y and regularization reg:

    A = Y^T Y + reg I + sum_j (|c_j| - 1) y_j y_j^T        negative confidences enter A with their magnitude
    A = L L^T                                              L is the "user weights"
    w = A^-1 y_i                                           two triangular solves with L
    s_j = c_j (w . y_j)   for the entries with c_j > 0     the contributions
    total = sum_j s_j                                      = y_i . x_u, x_u what recalculate_user returns

and the answer is the N largest contributions, best first in the total order (score descending, item id descending): what the
reference's heap of (score, itemid) tuples yields.  `dtype` is the arithmetic of every step: float64 is the yardstick, float32
the plain single-precision twin that says what the 1e-4 bar leaves over fp32 rounding.
"""
import numpy as np
from scipy.linalg import solve_triangular

FLT_MAX = float(np.finfo(np.float32).max)


def normal_matrix(Y, indices, data, reg, dtype=np.float64, gram=None):
    Y = np.asarray(Y, dtype=dtype)
    f = Y.shape[1]
    A = (Y.T @ Y if gram is None else np.asarray(gram, dtype=dtype)) + dtype(reg) * np.eye(f, dtype=dtype)
    if len(indices):
        Yu = Y[np.asarray(indices)]
        A = A + (Yu * (np.abs(np.asarray(data, dtype=dtype)) - dtype(1))[:, None]).T @ Yu
    return A.astype(dtype)


def cholesky(A):
    """Lower factor in A's own dtype (LAPACK potrf of that precision); ValueError on a non-positive pivot."""
    try:
        return np.linalg.cholesky(A)
    except np.linalg.LinAlgError as e:
        raise ValueError("non-positive pivot") from e


def solve_lower(L, b):
    return solve_triangular(L, np.asarray(b, dtype=L.dtype), lower=True, check_finite=False)


def solve_upper_t(L, z):
    """L^T w = z"""
    return solve_triangular(L, np.asarray(z, dtype=L.dtype), lower=True, trans="T", check_finite=False)


def order(ids, scores):
    """positions sorted by (score descending, id descending)"""
    return np.lexsort((-np.asarray(ids, dtype=np.int64), -np.asarray(scores, dtype=np.float64)))


def explain(Y, indices, data, itemid, reg, dtype=np.float64, L=None, gram=None):
    """One (user, item) pair: (total, ids, scores, L) with EVERY positive entry's contribution, sorted; all in `dtype`."""
    Yd = np.asarray(Y, dtype=dtype)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=dtype)
    if L is None:
        L = cholesky(normal_matrix(Yd, indices, data, reg, dtype, gram))
    w = solve_upper_t(L, solve_lower(L, Yd[itemid]))
    liked = data > 0
    ids = indices[liked]
    scores = (data[liked] * (Yd[ids] @ w)).astype(dtype) if liked.any() else np.zeros(0, dtype=dtype)
    total = dtype(scores.sum()) if len(scores) else dtype(0)
    o = order(ids, scores)
    return total, ids[o], scores[o], L


def explain_batch(Y, user_items, itemids, reg, N, alpha=1.0, dtype=np.float64):
    """user_items: scipy CSR with one row per batch entry; itemids [B, M].  Returns (total [B, M], ids [B, M, N], scores
    [B, M, N], full) in `dtype`, padded with (-1, -FLT_MAX) as the package pads; `full[b][m]` = (ids, scores) of ALL the
    pair's contributions in order, for the near-tie rule of the GPU tests."""
    itemids = np.asarray(itemids)
    if itemids.ndim == 1:
        itemids = itemids[:, None]
    B, M = itemids.shape
    total = np.zeros((B, M), dtype=dtype)
    ids = np.full((B, M, N), -1, dtype=np.int64)
    scores = np.full((B, M, N), -FLT_MAX, dtype=dtype)
    full = []
    gram = np.asarray(Y, dtype=dtype).T @ np.asarray(Y, dtype=dtype)
    for b in range(B):
        lo, hi = user_items.indptr[b], user_items.indptr[b + 1]
        idx, dat = user_items.indices[lo:hi], np.asarray(user_items.data[lo:hi], dtype=dtype) * dtype(alpha)
        L, row = None, []
        for m in range(M):
            t, i, s, L = explain(Y, idx, dat, int(itemids[b, m]), reg, dtype, L, gram)
            total[b, m] = t
            k = min(N, len(i))
            ids[b, m, :k], scores[b, m, :k] = i[:k], s[:k]
            row.append((i, s))
        full.append(row)
    return total, ids, scores, full


def compare(total, ids, scores, ref_total, ref_ids, ref_scores, full, tie=2e-4):
    """The accuracy measures of the GPU tests against the float64 restatement.  Returns a dict: worst contribution error as a
    fraction of the pair's max |s|, worst total error as a fraction of its sum |s|, the number of compared id positions, the
    number that differ, and how many of those are NOT excused as near-ties (the two items' float64 contributions within
    `tie` x max |s| of each other).  Scores are compared per ITEM, so an excused swap does not count as a score error."""
    B, M, N = ids.shape
    worst_s = worst_t = 0.0
    positions = differing = unexcused = 0
    for b in range(B):
        for m in range(M):
            fi, fs = full[b][m]
            smax = float(np.abs(fs).max()) if len(fs) else 0.0
            ssum = float(np.abs(fs).sum()) if len(fs) else 0.0
            dt = abs(float(total[b, m]) - float(ref_total[b, m]))
            worst_t = max(worst_t, dt / ssum if ssum > 0 else (0.0 if dt == 0 else np.inf))
            exact = dict(zip(fi.tolist(), fs.tolist()))
            k = min(N, len(fi))
            assert (ids[b, m, k:] == -1).all() and (scores[b, m, k:] == np.float32(-FLT_MAX)).all(), (b, m)
            assert len(set(ids[b, m, :k].tolist())) == k, (b, m)  # no item twice
            for r in range(k):
                positions += 1
                got = int(ids[b, m, r])
                assert got in exact, (b, m, r, got)  # a liked item of this user with c > 0
                ds = abs(float(scores[b, m, r]) - exact[got])
                worst_s = max(worst_s, ds / smax if smax > 0 else (0.0 if ds == 0 else np.inf))
                if got != int(ref_ids[b, m, r]):
                    differing += 1
                    if not abs(exact[got] - float(ref_scores[b, m, r])) <= tie * smax:
                        unexcused += 1
    return dict(contribution=worst_s, total=worst_t, positions=positions, differing=differing, unexcused=unexcused)
