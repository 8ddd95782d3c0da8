#!/usr/bin/env python3
"""Generates tests/golden/serving_golden.npz from the REFERENCE ITSELF: the CPU model layer (implicit.cpu.als, whose
recommend / similar_items / similar_users come from implicit.cpu.matrix_factorization_base) of the package assembled by
oracle/refsuite.py in build/refsuite.  Run in the build container only (the reference tree is not on the GPU box):

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_serving_golden.py

No model is trained: fixed float32 factor matrices are assigned (`model.user_factors = ...`) and the reference's own
(ids, scores) are recorded.  USERS x ITEMS x F = 60 x 150 x 8 with planted rows:

    items 20, 90, 140 identical and items 33, 34 identical (the tie order); item 77 all zero (the zero norm)
    user 11 = 3 x item row 20 (the duplicates lead its list); user 9 all zero
    user 3 likes every item, user 4 likes nothing; the liked rows are stored unsorted and hold explicit zeros

Arrays: X, Y; liked_indptr / liked_indices / liked_data (users x items) and likers_* (its transpose, items x users);
`cases`, one JSON string per case with the call and its options; c<i>_ids, c<i>_scores, the reference's result; and for a
fold-in case c<i>_query, what the reference's recalculate_user / recalculate_item returned for the same rows.  A batch call
gets rows `liked[userid]` (scipy row indexing), a scalar call the one row.  The file is written with fixed zip timestamps,
so the same reference reproduces it byte for byte.
"""
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SUITE = os.path.join(ROOT, "build", "refsuite")
sys.path.insert(0, SUITE)

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    from implicit.cpu.als import AlternatingLeastSquares  # noqa: E402

USERS, ITEMS, F = 60, 150, 8
REG = 0.05
rng = np.random.default_rng(2025)
X = (rng.standard_normal((USERS, F)) * 0.1).astype(np.float32)
Y = (rng.standard_normal((ITEMS, F)) * 0.1).astype(np.float32)
Y[90] = Y[140] = Y[20]
Y[34] = Y[33]
Y[77] = 0
X[11] = 3 * Y[20]
X[9] = 0


def liked_matrix(rows, cols, per_row, everything, nothing):
    """CSR straight from its three arrays: every row in shuffled (unsorted) order, every fifth stored value a zero."""
    indptr, indices = [0], []
    for r in range(rows):
        n = cols if r == everything else 0 if r == nothing else int(rng.integers(1, per_row))
        indices.append(rng.permutation(cols)[:n])
        indptr.append(indptr[-1] + n)
    indices = np.concatenate(indices).astype(np.int32)
    data = rng.integers(1, 5, len(indices)).astype(np.float32)
    data[::5] = 0
    return sp.csr_matrix((data, indices, np.array(indptr, dtype=np.int32)), shape=(rows, cols))


liked = liked_matrix(USERS, ITEMS, 30, everything=3, nothing=4)
likers = liked_matrix(ITEMS, USERS, 12, everything=-1, nothing=5)
assert not liked.has_sorted_indices and (liked.data == 0).any()

out = {"X": X, "Y": Y}
for prefix, m in (("liked", liked), ("likers", likers)):
    out[prefix + "_indptr"], out[prefix + "_indices"], out[prefix + "_data"] = m.indptr, m.indices, m.data
cases = []


def model(alpha=1.0):
    m = AlternatingLeastSquares(factors=F, regularization=REG, alpha=alpha, num_threads=1)
    m.user_factors, m.item_factors = X.copy(), Y.copy()
    return m


def rows_of(m, ids):
    return m[int(ids)] if np.isscalar(ids) else m[np.asarray(ids)]


def plain(v):
    return v if v is None or np.isscalar(v) else [int(x) for x in v]


def record(call, ids, scores, query=None, **opts):
    i = len(cases)
    cases.append(json.dumps(dict(call=call, **{k: plain(v) for k, v in opts.items()}), sort_keys=True))
    out[f"c{i}_ids"], out[f"c{i}_scores"] = np.asarray(ids), np.asarray(scores)
    if query is not None:
        out[f"c{i}_query"] = np.asarray(query)


def recommend(userid, N=10, filter_liked=True, filter_items=None, items=None, recalculate=False, alpha=1.0):
    m = model(alpha)
    uid = userid if np.isscalar(userid) else np.asarray(userid)
    rows = rows_of(liked, userid)
    query = m.recalculate_user(uid, rows) if recalculate else None
    ids, scores = m.recommend(uid, rows, N=N, filter_already_liked_items=filter_liked, filter_items=filter_items,
                              recalculate_user=recalculate, items=items)
    record("recommend", ids, scores, query, userid=userid, N=N, filter_liked=filter_liked, filter_items=filter_items,
           items=items, recalculate=recalculate, alpha=alpha)


def similar(call, qid, N=10, filter_ids=None, subset=None, recalculate=False, alpha=1.0):
    m = model(alpha)
    q = qid if np.isscalar(qid) else np.asarray(qid)
    query = None
    if call == "similar_users":
        ids, scores = m.similar_users(q, N=N, filter_users=filter_ids, users=subset)
    else:
        rows = rows_of(likers, qid) if recalculate else None
        query = m.recalculate_item(q, rows) if recalculate else None
        ids, scores = m.similar_items(q, N=N, recalculate_item=recalculate, item_users=rows, filter_items=filter_ids, items=subset)
    record(call, ids, scores, query, qid=qid, N=N, filter_ids=filter_ids, subset=subset, recalculate=recalculate, alpha=alpha)


everyone = list(range(USERS))
mixed = [int(u) for u in rng.permutation(USERS)[:25]] + [3, 4, 11, 11]
subset = [int(i) for i in rng.permutation(ITEMS)[:40]] + [20, 90, 77]
liked7 = [int(i) for i in rows_of(liked, 7).indices]
not_liked7 = [i for i in range(ITEMS) if i not in liked7][::-1]

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for userid in (7, 3, 4, 11, everyone, mixed):
        for N in ((1, 10, ITEMS + 50) if userid is everyone else (1, 2, 10, 37, ITEMS, ITEMS + 50)):
            for filter_liked in (True, False):
                recommend(userid, N=N, filter_liked=filter_liked)
    for filter_items in ([5, 20, 140], [5, 5, 20, 5], [], list(range(ITEMS))):
        recommend(7, N=10, filter_items=filter_items)
        recommend(mixed, N=12, filter_items=filter_items, filter_liked=False)
    for userid in (7, 11, mixed):
        for filter_liked in (True, False):
            for N in (1, 5, len(subset), len(subset) + 9):
                recommend(userid, N=N, items=subset, filter_liked=filter_liked)
    recommend(7, N=10, items=not_liked7)   # a subset that excludes every liked item
    recommend(7, N=10, items=liked7)       # a subset made only of liked items
    recommend(7, N=10, items=liked7, filter_liked=False)
    for alpha in (1.0, 2.0):
        for userid in (7, 4, mixed):
            recommend(userid, N=10, recalculate=True, alpha=alpha)
            recommend(userid, N=10, recalculate=True, alpha=alpha, filter_liked=False)

    for call, count, special in (("similar_items", ITEMS, [20, 33, 77, 140]), ("similar_users", USERS, [9, 11, 0])):
        batch = special + [int(i) for i in rng.permutation(count)[:20]]
        sub = [int(i) for i in rng.permutation(count)[:30]] + special[:3]
        for qid in special + [batch]:
            for N in (1, 2, 10, count, count + 7):
                similar(call, qid, N=N)
            similar(call, qid, N=10, filter_ids=special[:2] + [1])
            similar(call, qid, N=10, filter_ids=[])
            similar(call, qid, N=count, filter_ids=list(range(0, count, 2)))
            for N in (5, len(sub), len(sub) + 4):
                similar(call, qid, N=N, subset=sub)
    for alpha in (1.0, 2.0):
        for qid in (20, 5, [5, 77, 33, 101]):
            similar("similar_items", qid, N=10, recalculate=True, alpha=alpha)

out["cases"] = np.array(cases)
out["regularization"] = np.float64(REG)

# np.savez stamps every member with the current time: write the same container with a fixed date instead
path = os.path.join(HERE, "serving_golden.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
    for name in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[name]), allow_pickle=False)
        info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        z.writestr(info, buf.getvalue())
print("wrote", path, len(out), "arrays,", len(cases), "cases,", os.path.getsize(path), "bytes")
