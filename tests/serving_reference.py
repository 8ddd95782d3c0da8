"""Float64 numpy restatement of the serving contract: what recommend / similar_items / similar_users return for given
factor matrices.  Written from the contract (include/implicit_hip.h on imp_knn_topk, the head of csrc/topk.hip) and pinned
to the reference's own output by tests/golden/serving_golden.npz (tests/test_serving_host.py).  Host arrays in, host arrays
out; nothing of the package under test is imported.

The selection
    A row of candidate scores is reduced to its k best and written best first in the total order (score descending, then
    column id descending).  Which entries are RETAINED when more of them tie with the k-th score than there are places
    left is not decided by that order: the contract is the bounded min-heap of the reference's select (csrc/topk.hip
    restates it in closed form).  A candidate enters while the heap holds fewer than k entries or when its score is
    strictly greater than the heap's lowest; it then displaces the lowest (score, column) pair.  So among equal scores at
    the boundary the earlier columns stay (two duplicated items at N = 1: the SMALLER id is returned), while inside the
    list equal scores appear larger id first.  `select` simulates the heap where the boundary ties and sorts otherwise.

The tail
    * A filtered candidate (already liked, filter_items / filter_users) is not removed: its score becomes -FLT_MAX and it
      takes part in the selection like any other.  A row with fewer live candidates than N therefore ends in filtered
      entries, score -FLT_MAX, their ids fixed by the rule above (a row with everything filtered: N - 1, N - 2 ... 0).
      A stored explicit zero in `user_items` filters like any stored entry, EXCEPT under `items=`, where the re-indexing
      of the liked pattern onto the subset drops stored zeros (the golden file shows both).
    * N larger than the number of candidates: only the first `candidates` positions of a row are written.  The rest keeps
      what the output buffers were created with: id 0 and score 0.0.  With `items=` / `users=` in similar_* the ids go
      through the subset map afterwards, so those positions read subset[0]; recommend(items=) caps N at len(items).
    * The cosine division comes last and covers the whole row in float32: a filtered entry becomes -FLT_MAX / |q|, which
      is -inf for every query norm below 1 (a zero-norm query has norm 1e-10) and a finite number otherwise; an unwritten
      0.0 stays 0.0.  `similar` returns -inf where the float32 quotient overflows.
    No tail id is unspecified: every position is compared, ids and scores.

Cosine similarity
    norms = calculate_norms(F): the 2-norm of every row, a zero norm replaced by 1e-10.  Candidate scores are divided by
    the candidate's norm before the selection and by the query's norm after it.  The model divides by the STORED norm of
    `queryid` even when the query row was recalculated (recalculate_item=True), as the reference's GPU model layer does;
    the reference's CPU model layer, which the golden file records, divides by the norm of the recalculated row
    (`recalculated_norm=True` restates that).  `subset` is taken in the caller's order, not sorted.
"""
import heapq

import numpy as np

from ivf_reference import audit  # noqa: F401  the project's one near-tie rule, re-exported for the serving tests

FLT_MAX = float(np.finfo(np.float32).max)
ZERO_NORM = 1e-10


def select(scores, k):
    """(ids[k] int64, scores[k] float64) of one row of candidate scores under the rule of the module docstring; positions
    past len(scores) hold id 0, score 0.0."""
    scores = np.asarray(scores, dtype=np.float64)
    n = len(scores)
    out_ids, out_scores = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.float64)
    if k >= n or (scores >= np.partition(scores, n - k)[n - k]).sum() == k:
        order = np.lexsort((-np.arange(n), -scores))[:k]
    else:  # more entries tie with the k-th score than fit: the bounded heap decides
        heap = []
        for col, s in enumerate(scores.tolist()):
            if len(heap) < k:
                heapq.heappush(heap, (s, col))
            elif s > heap[0][0]:
                heapq.heapreplace(heap, (s, col))
        order = np.array([col for _, col in sorted(heap, reverse=True)], dtype=np.int64)
    out_ids[:len(order)] = order
    out_scores[:len(order)] = scores[order]
    return out_ids, out_scores


def _select_rows(S, k):
    out = [select(row, k) for row in S]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _row(user_items, r):
    lo, hi = user_items.indptr[r], user_items.indptr[r + 1]
    return np.asarray(user_items.indices[lo:hi], dtype=np.int64), np.asarray(user_items.data[lo:hi])


def recommend(X, Y, userid, user_items, N=10, filter_already_liked_items=True, filter_items=None, items=None):
    """(ids, scores) of recommend(): X[userid] @ Y.T in float64.  `userid` scalar -> one row, else one row per id with
    row r of `user_items` belonging to userid[r].  `X` may already be the query rows of a fold-in: pass userid = arange."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    scalar = np.isscalar(userid)
    users = np.atleast_1d(np.asarray(userid)).astype(np.int64)
    cand = np.arange(len(Y))
    if items is not None:
        cand = np.sort(np.asarray(items, dtype=np.int64))
        N = min(N, len(cand))
    S = X[users] @ Y[cand].T
    if filter_already_liked_items:
        for r in range(len(users)):
            cols, data = _row(user_items, r)
            if items is not None:
                cols = cols[data != 0]  # the re-indexing drops stored zeros ...
                pos = np.clip(np.searchsorted(cand, cols), 0, len(cand) - 1)
                cols = pos[cand[pos] == cols]  # ... and entries outside the subset
            S[r, cols] = -FLT_MAX
    if filter_items is not None and len(filter_items):
        S[:, np.asarray(filter_items, dtype=np.int64)] = -FLT_MAX
    ids, scores = _select_rows(S, N)
    if items is not None:
        ids = cand[ids]
    return (ids[0], scores[0]) if scalar else (ids, scores)


def calculate_norms(F):
    F = np.asarray(F, dtype=np.float64)
    norms = np.sqrt((F * F).sum(axis=1))
    norms[norms == 0] = ZERO_NORM
    return norms


def similar(F, queryid, N=10, subset=None, filter_ids=None, query_factors=None, recalculated_norm=False):
    """(ids, scores) of similar_items / similar_users over the factor rows F.  query_factors: the recalculated rows that
    stand in for F[queryid]."""
    F = np.asarray(F, dtype=np.float64)
    norms = calculate_norms(F)
    scalar = np.isscalar(queryid)
    qids = np.atleast_1d(np.asarray(queryid)).astype(np.int64)
    q = F[qids] if query_factors is None else np.asarray(query_factors, dtype=np.float64).reshape(len(qids), F.shape[1])
    qnorm = calculate_norms(q) if recalculated_norm and query_factors is not None else norms[qids]
    cand = np.arange(len(F)) if subset is None else np.asarray(subset, dtype=np.int64)
    S = (q @ F[cand].T) / norms[cand]
    if filter_ids is not None and len(filter_ids):
        S[:, np.asarray(filter_ids, dtype=np.int64)] = -FLT_MAX
    ids, scores = _select_rows(S, N)
    if subset is not None:
        ids = cand[ids]
    scores = scores / qnorm[:, None]
    scores[scores < -FLT_MAX] = -np.inf  # the float32 quotient overflows
    return (ids[0], scores[0]) if scalar else (ids, scores)


def near_ties(ids, scores, f, planted=()):
    """The margin census of one result (ids, scores: rows x k, best first): (close, compared) where `compared` counts the
    neighbouring pairs of live scores and `close` those whose float64 gap is below the near-tie bound 4 f 2^-23 relative.
    A pair of bitwise equal scores whose ids both lie in `planted` (duplicated or zero rows) is left out: its order is
    fixed by the id rule, not by rounding."""
    ids, scores = np.atleast_2d(ids), np.atleast_2d(scores)
    tol = 4 * f * float(np.finfo(np.float32).eps)
    planted = np.asarray(sorted(planted), dtype=np.int64)
    a, b = scores[:, :-1], scores[:, 1:]
    live = (b > -FLT_MAX) & np.isfinite(a)
    fixed = (a == b) & np.isin(ids[:, :-1], planted) & np.isin(ids[:, 1:], planted)
    counted = live & ~fixed
    close = counted & (a - np.where(live, b, 0.0) < tol * np.maximum(np.abs(a), 1e-30))
    return int(close.sum()), int(counted.sum())
