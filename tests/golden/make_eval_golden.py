#!/usr/bin/env python3
"""Generates tests/golden/eval_golden.npz from the REFERENCE ITSELF: the compiled implicit.evaluation of the package
assembled by oracle/refsuite.py in build/refsuite.  Run in the build container only (the reference tree is not on the GPU
box):

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_eval_golden.py

No model is trained: the reference's ranking_metrics_at_k drives a stub whose recommend() returns rows of a prescribed
int32 array.  Every case <name> (one per K) stores the held-out pattern (<name>_indptr / _indices / _shape), the
prescribed ids (<name>_ids, users x K, -1 = padding), <name>_K and the reference's four results (<name>_result:
precision, map, ndcg, auc).  Row u of the pattern, for u % 3 != 2 (a third of the users holds nothing out), has a length
cycling through 1, K - 1, K, K + 1 and 200; users 0, 1, 3, 4 are the special rows described in the code.

split_* records train_test_split(m, 0.8, random_state=7) of a small matrix with negative values.
"""
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SUITE = os.path.join(ROOT, "build", "refsuite")
sys.path.insert(0, SUITE)

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    from implicit import evaluation as ref  # noqa: E402

USERS, ITEMS = 150, 257
KS = (1, 3, 10, 64, 65, 100)
out = {"names": []}
rng = np.random.default_rng(2024)


class Stub:
    """recommend() hands back the prescribed rows."""

    def __init__(self, ids):
        self.ids = ids

    def recommend(self, userid, user_items, N=10):
        assert N == self.ids.shape[1]
        return np.ascontiguousarray(self.ids[np.asarray(userid)]), None


def case(K):
    lengths = [1, max(K - 1, 1), K, K + 1, 200]
    rows = []
    for u in range(USERS):
        n = 0 if u % 3 == 2 else lengths[(u // 3 * 2 + u % 3) % len(lengths)]
        rows.append(np.sort(rng.choice(ITEMS, size=n, replace=False)).astype(np.int32))
    ids = np.stack([rng.permutation(ITEMS)[:K] for _ in range(USERS)]).astype(np.int32)
    # user 0: every position a hit (K + 50 held-out items, the ids a shuffle of K of them)
    rows[0] = np.sort(rng.choice(ITEMS, size=K + 50, replace=False)).astype(np.int32)
    ids[0] = rng.permutation(rows[0])[:K]
    # user 1: no hit at all
    rows[1] = np.sort(rng.choice(ITEMS, size=K + 1, replace=False)).astype(np.int32)
    ids[1] = rng.permutation(np.setdiff1d(np.arange(ITEMS), rows[1]))[:K]
    # user 3: the held-out row ends in item ITEMS - 1; its first and its last element are recommended (last position and,
    # for K > 1, position 0), nothing else hits
    rows[3] = np.unique(np.concatenate([rng.choice(ITEMS - 1, size=K + 1, replace=False), [ITEMS - 1]])).astype(np.int32)
    ids[3] = rng.permutation(np.setdiff1d(np.arange(ITEMS), rows[3]))[:K]
    ids[3, -1] = rows[3][-1]
    if K > 1:
        ids[3, 0] = rows[3][0]
    # user 4 and every 7th user: the tail of the row is -1 padding (user 4: from position 1 on, a hit in front)
    rows[4] = np.sort(rng.choice(ITEMS, size=5, replace=False)).astype(np.int32)
    ids[4, 0] = rows[4][2]
    ids[4, 1:] = -1
    for u in range(7, USERS, 7):
        ids[u, rng.integers(0, K):] = -1
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32)
    test = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(USERS, ITEMS))
    train = sp.csr_matrix((USERS, ITEMS))
    res = ref.ranking_metrics_at_k(Stub(ids), train, test, K=K, show_progress=False)
    name = f"K{K}"
    out["names"].append(name)
    out[name + "_indptr"], out[name + "_indices"] = indptr, indices
    out[name + "_shape"] = np.array([USERS, ITEMS], dtype=np.int64)
    out[name + "_ids"] = ids
    out[name + "_K"] = np.int64(K)
    out[name + "_result"] = np.array([res["precision"], res["map"], res["ndcg"], res["auc"]], dtype=np.float64)


for K in KS:
    case(K)

# train_test_split on a small matrix with some negative values
m = sp.random(30, 20, density=0.3, random_state=np.random.RandomState(5), format="csr", dtype=np.float64)
m.data = np.round(m.data * 10 - 3)
m.data[m.data == 0] = 1.0
assert (m.data < 0).any()
train, test = ref.train_test_split(m, 0.8, random_state=7)
for prefix, mat in (("split_in", m), ("split_train", train), ("split_test", test)):
    mat = mat.tocsr()
    out[prefix + "_indptr"] = mat.indptr.astype(np.int32)
    out[prefix + "_indices"] = mat.indices.astype(np.int32)
    out[prefix + "_data"] = mat.data.astype(np.float64)
    out[prefix + "_shape"] = np.array(mat.shape, dtype=np.int64)

out["names"] = np.array(out["names"])
np.savez_compressed(os.path.join(HERE, "eval_golden.npz"), **out)
print("wrote", os.path.join(HERE, "eval_golden.npz"), len(out), "arrays,", len(out["names"]), "cases")
