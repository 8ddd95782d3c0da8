#!/usr/bin/env python3
"""Generates tests/golden/knn_golden.npz from the REFERENCE ITSELF: implicit.nearest_neighbours (its weighting helpers, its
compiled all_pairs_knn and NearestNeighboursScorer), the package assembled by oracle/refsuite.py in build/refsuite.  Run
in the build container only (the reference tree is not on the GPU box):

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_knn_golden.py

Every case <name> stores its users x items counts (<name>_indptr / _indices / _data / _shape), the model kind
(<name>_kind: cosine, tfidf, bm25), K, the weighted users x items matrix the model passes to all_pairs_knn
(<name>_w_*), the fitted similarity CSR (<name>_sim_*), and recommend() output of every user for N = <name>_N with
remove_own_likes on (<name>_rec1_*) and off (<name>_rec0_*): ids / scores concatenated, <name>_recX_ptr the offsets.
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
    from implicit import nearest_neighbours as ref  # noqa: E402
    from implicit._nearest_neighbours import NearestNeighboursScorer  # noqa: E402

out = {"names": []}
rng = np.random.default_rng(77)


def put_csr(prefix, m):
    m = m.tocsr()
    out[prefix + "_indptr"] = m.indptr.astype(np.int32)
    out[prefix + "_indices"] = m.indices.astype(np.int32)
    out[prefix + "_data"] = m.data.astype(np.float64)
    out[prefix + "_shape"] = np.array(m.shape, dtype=np.int64)


def weighted(kind, counts, K1=1.2, B=0.75):
    if kind == "cosine":
        return ref.normalize(counts.T).T
    if kind == "tfidf":
        return ref.normalize(ref.tfidf_weight(counts.T)).T
    return ref.bm25_weight(counts.T, K1, B).T


def model(kind, K):
    return {"cosine": ref.CosineRecommender, "tfidf": ref.TFIDFRecommender, "bm25": ref.BM25Recommender}[kind](K=K)


def case(name, counts, kind, K, N=5):
    counts = sp.csr_matrix(counts, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = model(kind, K)
        m.fit(counts, show_progress=False)
        w = weighted(kind, counts).tocsr()
    out["names"].append(name)
    put_csr(name, counts)
    out[name + "_kind"] = np.array(kind)
    out[name + "_K"] = np.int64(K)
    out[name + "_N"] = np.int64(N)
    put_csr(name + "_w", w)
    put_csr(name + "_sim", m.similarity)
    scorer = NearestNeighboursScorer(m.similarity)
    for own in (0, 1):
        ids, scores, ptr = [], [], [0]
        for u in range(counts.shape[0]):
            row = counts[u]
            i, s = scorer.recommend(row.indptr, row.indices, row.data, K=N, remove_own_likes=bool(own))
            ids.append(i)
            scores.append(s)
            ptr.append(ptr[-1] + len(i))
        out[f"{name}_rec{own}_ids"] = np.concatenate(ids).astype(np.int32)
        out[f"{name}_rec{own}_scores"] = np.concatenate(scores).astype(np.float64)
        out[f"{name}_rec{own}_ptr"] = np.array(ptr, dtype=np.int64)


def random_counts(users, items, nnz, empty_items=(), binary=False):
    r = rng.integers(0, users, nnz)
    c = rng.integers(0, items, nnz)
    keep = ~np.isin(c, empty_items)
    v = np.ones(keep.sum()) if binary else rng.integers(1, 6, keep.sum()).astype(np.float64)
    m = sp.csr_matrix((v, (r[keep], c[keep])), shape=(users, items))
    m.sum_duplicates()
    if binary:
        m.data[:] = 1.0
    return m


base = random_counts(40, 30, 260)
no_item0 = random_counts(40, 30, 260, empty_items=(0, 17))
ties = random_counts(25, 20, 120, binary=True)
neg_idf = random_counts(30, 12, 90).tolil()
neg_idf[3, :] = 2.0  # user 3 likes every item: its idf (log N - log(1 + df)) is negative in the bm25 / tfidf weighting
neg_idf = neg_idf.tocsr()
for kind in ("cosine", "tfidf", "bm25"):
    for K in (1, 3, 50):
        case(f"base_{kind}_K{K}", base, kind, K)
    case(f"noitem0_{kind}_K3", no_item0, kind, 3)
    case(f"noitem0_{kind}_K50", no_item0, kind, 50)
    case(f"ties_{kind}_K3", ties, kind, 3)
    case(f"negidf_{kind}_K4", neg_idf, kind, 4)
case("issue_example_cosine_K3", sp.csr_matrix(np.array([[0, 1, 1, 0], [0, 1, 0, 1], [0, 0, 1, 1]], dtype=np.float64)),
     "cosine", 3)

out["names"] = np.array(out["names"])
np.savez_compressed(os.path.join(HERE, "knn_golden.npz"), **out)
print("wrote", os.path.join(HERE, "knn_golden.npz"), len(out), "arrays,", len(out["names"]), "cases")
