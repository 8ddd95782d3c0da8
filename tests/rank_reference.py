"""Float64 restatement of rank_items / score_items, written from the contract (include/implicit_hip.h on imp_knn_rank).
Numpy only: nothing of the package under test is imported here."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def scores(X, Y, users, lists, liked=None):
    """For each position r: the float64 scores of user users[r] against the items lists[r], in the list's own order.  liked: a
    scipy CSR with one row per position (any index order, stored zeros count); a liked candidate scores -FLT_MAX.
    Returns (scores, magnitudes): two lists of float64 arrays, magnitudes[r][j] = sum_k |x_k| |y_k| of that pair."""
    X64, Y64 = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    out, mags = [], []
    for r, (u, ids) in enumerate(zip(users, lists)):
        ids = np.asarray(ids, dtype=np.int64)
        s = Y64[ids] @ X64[u]
        m = np.abs(Y64[ids]) @ np.abs(X64[u])
        if liked is not None:
            row = liked.indices[liked.indptr[r]:liked.indptr[r + 1]]
            s = np.where(np.isin(ids, row), -float(FLT_MAX), s)
        out.append(s)
        mags.append(m)
    return out, mags


def rank(fp32_scores, ids, N):
    """The order of one list, given its fp32 scores: (score descending, id descending) with -0.0 == +0.0, the first N, padded
    with (-1, -FLT_MAX).  Returns (ids [N] int32, scores [N] float32)."""
    s = np.asarray(fp32_scores, dtype=np.float32) + np.float32(0.0)  # -0.0 + 0.0 = +0.0
    ids = np.asarray(ids, dtype=np.int64)
    order = np.lexsort((-ids, -s))[:N]  # last key first: score descending, then id descending
    out_ids = np.full(N, -1, dtype=np.int32)
    out_scores = np.full(N, -FLT_MAX, dtype=np.float32)
    out_ids[:len(order)] = ids[order]
    out_scores[:len(order)] = s[order]
    return out_ids, out_scores
