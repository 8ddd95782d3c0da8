"""Host-only checks of the item-item nearest-neighbour contract: the float64 restatement (tests/knn_reference.py) against
the reference's own output (tests/golden/knn_golden.npz) and scipy's A^T A, and the weighting helpers of
implicit_amd.nearest_neighbours against the reference's."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import knn_reference as kr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "knn_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def csr(g, prefix):
    return sp.csr_matrix((g[prefix + "_data"], g[prefix + "_indices"], g[prefix + "_indptr"]), shape=tuple(g[prefix + "_shape"]))


def rows_agree(ref, got):
    """Similarity CSRs agree row by row: equal entries, or a difference confined to items tied at the k-th score."""
    for r in range(ref.shape[0]):
        a, b = ref[r], got[r]
        if np.array_equal(a.indices, b.indices):
            scale = max(np.abs(a.data).max(initial=0), 1e-300)
            if not np.all(np.abs(a.data - b.data) <= 1e-12 * scale):
                return False
            continue
        oa, ob = np.argsort(-a.data, kind="stable"), np.argsort(-b.data, kind="stable")
        if not kr.tie_tolerant_equal(a.indices[oa], a.data[oa], b.indices[ob], b.data[ob]):
            return False
    return True


def test_golden_cases_cover_the_issue(golden):
    names = list(golden["names"])
    assert {str(golden[n + "_kind"]) for n in names} == {"cosine", "tfidf", "bm25"}
    assert {1, 3, 50} <= {int(golden[n + "_K"]) for n in names}
    assert any(n.startswith("noitem0") for n in names) and any(n.startswith("ties") for n in names)
    assert min(golden["negidf_bm25_K4_w_data"]) < 0


@pytest.mark.parametrize("kind", ["cosine", "tfidf", "bm25"])
def test_weighting_equals_reference(golden, kind):
    from implicit_amd import nearest_neighbours as nn

    for name in golden["names"]:
        if str(golden[name + "_kind"]) != kind:
            continue
        counts = csr(golden, name)
        if kind == "cosine":
            w = nn.normalize(counts.T).T
        elif kind == "tfidf":
            w = nn.normalize(nn.tfidf_weight(counts.T)).T
        else:
            w = nn.bm25_weight(counts.T, 1.2, 0.75).T
        ref = csr(golden, name + "_w")
        w = w.tocsr()
        np.testing.assert_array_equal(w.indptr, ref.indptr)
        np.testing.assert_array_equal(w.indices, ref.indices)
        np.testing.assert_array_equal(w.data, ref.data)  # the same float64 operations: bitwise


def test_restatement_matches_reference_similarity(golden):
    exact = 0
    for name in golden["names"]:
        K = int(golden[name + "_K"])
        ref = csr(golden, name + "_sim")
        got = kr.fit_similarity(csr(golden, name + "_w"), K)
        assert rows_agree(ref, got), name
        if np.array_equal(ref.indptr, got.indptr) and np.array_equal(ref.indices, got.indices):
            np.testing.assert_array_equal(ref.data, got.data, err_msg=name)  # same summation order: bitwise
            exact += 1
    assert exact >= len(golden["names"]) - 6  # only the tie cases may choose other tied items


def test_row0_fold_structure(golden):
    # 3 users x 4 items, item 0 without users, K = 3: short rows pad with (0, 0, 0.0), so row 0 is [0] / [0.0]
    ref = csr(golden, "issue_example_cosine_K3_sim")
    got = kr.fit_similarity(csr(golden, "issue_example_cosine_K3_w"), 3)
    np.testing.assert_array_equal(got.indptr, ref.indptr)
    np.testing.assert_array_equal(got.indices, ref.indices)
    np.testing.assert_array_equal(got.data, ref.data)
    assert list(ref[0].indices) == [0] and list(ref[0].data) == [0.0]


def test_restatement_matches_reference_recommend(golden):
    for name in golden["names"]:
        sim = csr(golden, name + "_sim")
        counts = csr(golden, name)
        N = int(golden[name + "_N"])
        for own in (0, 1):
            ids, scores, cnt = kr.product_topk(counts, sim, N, zero_own=bool(own))
            ptr = golden[f"{name}_rec{own}_ptr"]
            for u in range(counts.shape[0]):
                ri = golden[f"{name}_rec{own}_ids"][ptr[u]:ptr[u + 1]]
                rs = golden[f"{name}_rec{own}_scores"][ptr[u]:ptr[u + 1]]
                assert cnt[u] == len(ri), (name, own, u)
                assert kr.tie_tolerant_equal(ri, rs, ids[u, :cnt[u]], scores[u, :cnt[u]]), (name, own, u)


def test_restatement_against_scipy_product():
    rng = np.random.default_rng(3)
    A = sp.random(60, 80, density=0.08, random_state=rng, format="csr")
    B = sp.random(80, 70, density=0.1, random_state=rng, format="csr")
    full = (A @ B).toarray()
    pattern = ((A != 0).astype(np.int32) @ (B != 0).astype(np.int32)).toarray() > 0
    k = 7
    ids, scores, counts = kr.product_topk(A, B, k)
    for r in range(60):
        cand = np.flatnonzero(pattern[r])
        assert counts[r] == min(k, len(cand))
        order = np.lexsort((-cand, -full[r, cand]))[:k]
        np.testing.assert_array_equal(ids[r, :counts[r]], cand[order])
        np.testing.assert_allclose(scores[r, :counts[r]], full[r, cand[order]], rtol=1e-12, atol=1e-15)
        assert np.all(ids[r, counts[r]:] == -1) and np.all(np.isneginf(scores[r, counts[r]:]))


def test_zero_own_keeps_touched_columns():
    A = sp.csr_matrix(np.array([[1.0, 0, 2.0, 0]]))
    B = sp.csr_matrix(np.array([[0, 1.0, 3.0, 0], [0, 0, 0, 0], [0, 0, 1.0, 0], [9.0, 0, 0, 0]]))
    ids, scores, counts = kr.product_topk(A, B, 4, zero_own=True)
    # touched: 1 (1.0) and 2 (3 + 2 = 5, zeroed); column 0 is liked but untouched, so it is no candidate
    assert counts[0] == 2
    assert list(ids[0, :2]) == [1, 2] and list(scores[0, :2]) == [1.0, 0.0]
