"""The item-item nearest-neighbour models on the GPU (csrc/knn.hip, implicit_amd.nearest_neighbours): the primitive
imp_sparse_topk_product against the float64 restatement (tests/knn_reference.py), the models against the reference's own
output (tests/golden/knn_golden.npz), and the model surface."""
import io
import os
import pickle
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import knn_reference as kr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "knn_golden.npz")
KINDS = ("cosine", "tfidf", "bm25")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def nn(gpu):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from implicit_amd import nearest_neighbours

    return nearest_neighbours


def csr(g, prefix):
    return sp.csr_matrix((g[prefix + "_data"], g[prefix + "_indices"], g[prefix + "_indptr"]), shape=tuple(g[prefix + "_shape"]))


def make_model(nn, kind, K):
    return {"cosine": nn.CosineRecommender, "tfidf": nn.TFIDFRecommender, "bm25": nn.BM25Recommender}[kind](K=K)


def fit(model, counts):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit(counts, show_progress=False)
    return model


def weighted(nn, kind, counts):
    if kind == "cosine":
        return nn.normalize(counts.T).T.tocsr()
    if kind == "tfidf":
        return nn.normalize(nn.tfidf_weight(counts.T)).T.tocsr()
    return nn.bm25_weight(counts.T, 1.2, 0.75).T.tocsr()


def device_topk(A, B, k, zero_own=False):
    from implicit_amd import gpu

    return gpu.sparse_topk_product(gpu.SpMat(A), gpu.SpMat(B), k, zero_own)


def assert_topk_equal(got, want):
    """Against the restatement, which has the kernel's summation order and tie rule: counts, ids and score bits, padding
    included (tests/test_gpu_knn_edges.py does the same at the kernel's cuts)."""
    gi, gs, gc = got
    wi, ws, wc = want
    np.testing.assert_array_equal(gc, wc)
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(gs.view(np.int64), ws.view(np.int64))
    pad = np.arange(gi.shape[1])[None, :] >= gc[:, None]
    assert np.all(gi[pad] == -1) and np.all(np.isneginf(gs[pad]))


# ---- against the reference's own output --------------------------------------------------------------------------------
def test_golden_similarity(nn, golden):
    exact = 0
    for name in golden["names"]:
        kind, K = str(golden[name + "_kind"]), int(golden[name + "_K"])
        model = fit(make_model(nn, kind, K), csr(golden, name))
        ref, got = csr(golden, name + "_sim"), model.similarity
        assert got.dtype == np.float64
        if np.array_equal(ref.indptr, got.indptr) and np.array_equal(ref.indices, got.indices):
            scale = np.abs(ref.data).max(initial=1e-300)
            assert np.all(np.abs(ref.data - got.data) <= 1e-12 * scale), name
            exact += int(np.array_equal(ref.data, got.data))
            continue
        assert name.startswith("ties"), name  # only exact ties may keep other items than the reference
        for r in range(ref.shape[0]):
            a, b = ref[r], got[r]
            oa, ob = np.argsort(-a.data, kind="stable"), np.argsort(-b.data, kind="stable")
            assert kr.tie_tolerant_equal(a.indices[oa], a.data[oa], b.indices[ob], b.data[ob]), (name, r)
    assert exact >= len(golden["names"]) - 6


def test_golden_row0_fold(nn, golden):
    model = fit(nn.CosineRecommender(K=3), csr(golden, "issue_example_cosine_K3"))
    sim = model.similarity
    np.testing.assert_array_equal(sim.indptr, golden["issue_example_cosine_K3_sim_indptr"])
    np.testing.assert_array_equal(sim.indices, golden["issue_example_cosine_K3_sim_indices"])
    assert list(sim[0].indices) == [0] and list(sim[0].data) == [0.0]
    # users of item 0 touch item 0 through that stored entry, as in the reference
    ids, scores = model.recommend(0, sp.csr_matrix(np.array([[1.0, 0, 0, 0]])), N=4, filter_already_liked_items=False)
    assert list(ids) == [0] and list(scores) == [0.0]


def test_golden_recommend(nn, golden):
    for name in golden["names"]:
        kind, K, N = str(golden[name + "_kind"]), int(golden[name + "_K"]), int(golden[name + "_N"])
        model = make_model(nn, kind, K)
        model.similarity = csr(golden, name + "_sim")  # the reference's similarity: recommend alone is under test
        counts = csr(golden, name)
        for own in (0, 1):
            ptr = golden[f"{name}_rec{own}_ptr"]
            ids, scores = model.recommend(np.arange(counts.shape[0]), counts, N=N, filter_already_liked_items=bool(own))
            assert ids.shape == (counts.shape[0], N) and scores.dtype == np.float64
            for u in range(counts.shape[0]):
                ri = golden[f"{name}_rec{own}_ids"][ptr[u]:ptr[u + 1]]
                rs = golden[f"{name}_rec{own}_scores"][ptr[u]:ptr[u + 1]]
                n = len(ri)
                assert kr.tie_tolerant_equal(ri, rs, ids[u, :n], scores[u, :n]), (name, own, u)
                assert np.all(ids[u, n:] == -1) and np.all(scores[u, n:] == -np.finfo(np.float32).max)


# ---- against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset", ["ml100k", "lastfm360k@0.05"])
def test_fit_against_restatement(nn, dataset):
    from implicit_amd import synthetic

    name, _, scale = dataset.partition("@")
    counts = synthetic.named(name, scale=float(scale or 1.0)).astype(np.float64)
    for kind in KINDS:
        w = weighted(nn, kind, counts)
        items = w.T.tocsr()
        for K in (1, 20, 200):
            assert_topk_equal(device_topk(items, w, K), kr.product_topk(items, w, K))


def _class_matrix():
    """A users x items matrix whose item rows (A = items x users) fall in every class: an empty row, light rows that stay in
    the LDS table, rows past the table limit, a row heavier than many 64-column steps, and rows of ml20m density."""
    rng = np.random.default_rng(11)
    users, items = 3000, 5000
    rows, cols = [], []
    for i in range(1, items):
        deg = 1 if i < 2000 else 8 if i < 4000 else 60 if i < 4990 else 2500
        rows.append(rng.choice(users, deg, replace=False))
        cols.append(np.full(deg, i))
    heavy_users = rng.choice(users, 200, replace=False)  # users of 1000+ items make every one of their items heavy
    for u in heavy_users:
        its = rng.choice(np.arange(1, items), 1200, replace=False)
        rows.append(np.full(len(its), u))
        cols.append(its)
    r, c = np.concatenate(rows), np.concatenate(cols)
    m = sp.csr_matrix((rng.uniform(0.5, 4.0, len(r)), (r, c)), shape=(users, items))
    m.sum_duplicates()
    return m


def test_row_classes(nn):
    counts = _class_matrix()
    w = weighted(nn, "cosine", counts)
    items = w.T.tocsr()
    assert np.diff(items.indptr)[0] == 0  # an empty row
    for K in (20, 100):
        got = device_topk(items, w, K)
        assert got[2][0] == 0 and got[2].max() == K
        assert_topk_equal(got, kr.product_topk(items, w, K))


def test_recommend_against_restatement(nn):
    from implicit_amd import synthetic

    counts = synthetic.named("ml100k").astype(np.float64)
    model = fit(nn.BM25Recommender(K=50), counts)
    for own in (False, True):
        for N in (10, 300, 1500):
            assert_topk_equal(device_topk(counts, model.similarity, N, own), kr.product_topk(counts, model.similarity, N, own))


def test_bitwise_determinism(nn):
    from implicit_amd import synthetic

    counts = synthetic.named("lastfm360k", scale=0.03).astype(np.float64)
    a = fit(nn.CosineRecommender(K=20), counts).similarity
    b = fit(nn.CosineRecommender(K=20), counts).similarity
    for x, y in ((a.indptr, b.indptr), (a.indices, b.indices), (a.data.view(np.int64), b.data.view(np.int64))):
        np.testing.assert_array_equal(x, y)


# ---- model surface -----------------------------------------------------------------------------------------------------
def test_large_k_items_and_n(nn):
    from implicit_amd import synthetic

    counts = synthetic.named("ml100k").astype(np.float64)
    n_items = counts.shape[1]
    model = fit(nn.CosineRecommender(K=200), counts)
    users = np.arange(40)
    ids, scores, cnt = kr.product_topk(counts[users], model.similarity, n_items, zero_own=True)
    got_ids, got_scores = model.recommend(users, counts[users], N=1200)
    assert cnt.max() > 1024
    for u in users:
        n = min(1200, cnt[u])
        assert kr.tie_tolerant_equal(ids[u, :n], scores[u, :n], got_ids[u, :n], got_scores[u, :n])
    selected = np.arange(0, n_items, 3)
    one_ids, one_scores = model.recommend(5, counts[5], items=selected)
    assert set(one_ids.tolist()) == set(selected.tolist())
    touched = np.isin(one_ids, ids[5, :cnt[5]])
    assert np.all(one_scores[~touched] == -np.finfo(np.float64).max)
    assert np.all(np.diff(one_scores[touched]) <= 0)


def test_argument_errors(gpu):
    from implicit_amd import gpu as g

    A = g.SpMat(sp.csr_matrix(np.eye(3)))
    B = g.SpMat(sp.csr_matrix(np.ones((4, 5))))
    with pytest.raises(ValueError, match="A.cols"):
        g.sparse_topk_product(A, B, 3)
    with pytest.raises(ValueError, match="k must be"):
        g.sparse_topk_product(A, A, 0)
    B3 = g.SpMat(sp.csr_matrix(np.ones((3, 5))))
    with pytest.raises(ValueError, match="zero_own_columns"):
        g.sparse_topk_product(A, B3, 2, zero_own_columns=True)
    # nothing written on an argument error
    from implicit_amd.gpu import _hip

    import ctypes

    ids = np.full((3, 2), 7, np.int32)
    scores = np.full((3, 2), 7.0)
    counts = np.full(3, 7, np.int32)
    st = _hip.lib().imp_sparse_topk_product(A._h, B._h, 2, 0, ids.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    assert st == _hip.IMP_INVALID_ARGUMENT
    assert np.all(ids == 7) and np.all(scores == 7.0) and np.all(counts == 7)
    with pytest.raises(ValueError, match="column id"):
        _hip.check(_hip.lib().imp_spmat_create(1, 2, 1, np.array([0, 1], np.int64).ctypes.data,
                                               np.array([5], np.int32).ctypes.data, np.array([1.0]).ctypes.data,
                                               ctypes.byref(ctypes.c_void_p())))


def test_batch_equals_single(nn):
    from implicit_amd import synthetic

    counts = synthetic.named("ml100k").astype(np.float64)
    model = fit(nn.TFIDFRecommender(K=30), counts)
    users = np.arange(0, 900, 7)
    filt = np.arange(0, 200, 2)
    for kw in ({}, {"filter_already_liked_items": False}, {"filter_items": filt}, {"items": np.arange(50, 400)}):
        ids, scores = model.recommend(users, counts[users], N=15, **kw)
        for i, u in enumerate(users):
            si, ss = model.recommend(u, counts[u], N=15, **kw)
            si, ss = si[:15], ss[:15]
            np.testing.assert_array_equal(ids[i, :len(si)], si)
            np.testing.assert_array_equal(scores[i, :len(ss)], ss)
            assert np.all(ids[i, len(si):] == -1)


def test_similar_items_and_errors(nn):
    from implicit_amd import synthetic

    counts = synthetic.named("ml100k").astype(np.float64)
    model = fit(nn.CosineRecommender(K=10), counts)
    ids, scores = model.similar_items(np.arange(5), N=5)
    for i in range(5):
        si, ss = model.similar_items(i, N=5)
        np.testing.assert_array_equal(ids[i, :len(si)], si)
    with pytest.raises(NotImplementedError):
        model.similar_users(0)
    with pytest.raises(NotImplementedError):
        model.fit(counts, callback=lambda *a: None)


def test_persistence_round_trip(nn):
    from implicit_amd import synthetic

    counts = synthetic.named("ml100k").astype(np.float64)
    model = fit(nn.BM25Recommender(K=25), counts)
    buf = io.BytesIO()
    model.save(buf)
    buf.seek(0)
    with np.load(buf) as d:
        assert sorted(d.files) == ["K", "data", "indices", "indptr", "shape"]
    buf.seek(0)
    loaded = nn.BM25Recommender.load(buf)
    assert loaded.K == 25
    for x in ("indptr", "indices", "data"):
        np.testing.assert_array_equal(getattr(loaded.similarity, x), getattr(model.similarity, x))
    users = np.arange(20)
    np.testing.assert_array_equal(loaded.recommend(users, counts[users])[0], model.recommend(users, counts[users])[0])
    clone = pickle.loads(pickle.dumps(model))
    np.testing.assert_array_equal(clone.recommend(users, counts[users])[0], model.recommend(users, counts[users])[0])
