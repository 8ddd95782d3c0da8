"""EASE on the device (csrc/ease.hip, csrc/spd_inverse.hip, implicit_amd/ease.py) on the inputs of tests/ease_reference.py.

Gram matrix: zero tolerance on integer inputs, the fp32 summation bound on weighted ones.  Inverse: the yardstick is LAPACK's
own float32 Cholesky inverse of the same matrix, d_ref = ||P_lapack32 - P64||_F / ||P64||_F, and the assertion
d_gpu <= max(2 d_ref, 2^-23): two backward-stable orderings of the same sums differ by an O(1) factor (a numpy-fp32 blocked
scheme of the kernel's shape reads 0.75 - 1.16 d_ref on these inputs), and the n <= 2 cases sit at one ulp.  Weights and top-k
are bitwise defined and checked with zero tolerance against weights32 / scores32 / topk_order."""
import io
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_equal

import ease_reference as ref
from implicit_amd.synthetic import synthetic_csr
from implicit_amd.utils import transpose_csr

pytestmark = pytest.mark.gpu

FLOOR = 2.0**-23


def device_gram(gpu, X, reg):
    X = X.astype(np.float32)
    X.sum_duplicates()
    return gpu.ease_gram(gpu.CSRMatrix(transpose_csr(X)), gpu.CSRMatrix(X), reg).to_numpy()


# ---- Gram matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("items", ref.GRAM_EXACT_ITEMS)
def test_gram_exact(gpu, items):
    X = ref.gram_exact_case(items)
    G = device_gram(gpu, X, ref.GRAM_REG)
    assert G.dtype == np.float32 and G.shape == (items, items)
    assert_array_equal(G, G.T)
    assert_array_equal(G.astype(np.float64), ref.gram64(X, ref.GRAM_REG))
    held = np.bincount(X.indices, minlength=items)
    for i in np.flatnonzero(held == 0):  # an item nobody has: lambda e_i
        e = np.zeros(items, dtype=np.float32)
        e[i] = ref.GRAM_REG
        assert_array_equal(G[i], e)


def test_gram_weighted(gpu):
    X = synthetic_csr(300, 70, 3000, seed=7)
    reg = 2.5
    G = device_gram(gpu, X, reg)
    assert_array_equal(G, G.T)
    D = np.asarray(X.todense(), dtype=np.float64)
    count = (D != 0).T.astype(np.float64) @ (D != 0)
    bound = (count + 1) * 2.0**-24 * (np.abs(D).T @ np.abs(D))
    err = np.abs(G.astype(np.float64) - ref.gram64(X, reg))
    off = ~np.eye(70, dtype=bool)
    print("gram weighted: max err / bound off the diagonal", float((err[off] / np.maximum(bound[off], 1e-300)).max()))
    assert np.all(err <= bound)


def test_gram_rejects(gpu):
    X = synthetic_csr(30, 20, 100, seed=1)
    a, b = gpu.CSRMatrix(transpose_csr(X)), gpu.CSRMatrix(X)
    with pytest.raises(ValueError):
        gpu.ease_gram(b, b, 1.0)  # not the two orientations of one matrix
    with pytest.raises(ValueError):
        gpu.ease_gram(a, b, 1.0, gpu.Matrix.zeros(20, 19))
    with pytest.raises(ValueError):
        gpu.ease_gram(a, b, 1.0, gpu.Matrix(np.zeros((20, 20), dtype=np.float16)))


# ---- inverse --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.SPD_SIZES)
def test_spd_inverse_accuracy(gpu, n):
    G32, P64 = ref.spd_case(n)
    d_ref = ref.rel_distance(ref.lapack32_inverse(G32), P64)
    A = np.tril(G32).astype(np.float32)
    A[np.triu_indices(n, 1)] = np.nan  # only the lower triangle is read
    M = gpu.Matrix(A)
    assert gpu.spd_inverse(M) is M
    P = M.to_numpy()
    d_gpu = ref.rel_distance(P, P64)
    print(f"spd_inverse n={n}: d_ref={d_ref:.3e} d_gpu={d_gpu:.3e} ratio={d_gpu / d_ref:.3f}")
    assert_array_equal(P, P.T)
    assert d_gpu <= max(2 * d_ref, FLOOR)


@pytest.mark.parametrize("n,bad", [(70, 40), (300, 257)])
def test_spd_inverse_failed_pivot(gpu, n, bad):
    A = 2.0 * np.eye(n, dtype=np.float32)
    A[bad, bad] = -1.0
    with pytest.raises(ValueError) as e:
        gpu.spd_inverse(gpu.Matrix(A))
    assert e.value.failed_pivot == bad
    # the library works afterwards
    G32, P64 = ref.spd_case(65)
    P = gpu.spd_inverse(gpu.Matrix(G32.copy())).to_numpy()
    assert ref.rel_distance(P, P64) <= max(2 * ref.rel_distance(ref.lapack32_inverse(G32), P64), FLOOR)


def test_spd_inverse_rejects(gpu):
    with pytest.raises(ValueError):
        gpu.spd_inverse(gpu.Matrix.zeros(4, 5))
    with pytest.raises(ValueError):
        gpu.spd_inverse(gpu.Matrix(np.eye(4, dtype=np.float16)))
    nan = np.eye(5, dtype=np.float32)
    nan[2, 2] = np.nan
    with pytest.raises(ValueError) as e:
        gpu.spd_inverse(gpu.Matrix(nan))
    assert e.value.failed_pivot == 2


# ---- weights --------------------------------------------------------------------------------------------------------------
def test_weights_bitwise(gpu):
    P = ref.lapack32_inverse(ref.spd_case(257)[0]).astype(np.float32)
    M = gpu.Matrix(P.copy())
    B = gpu.ease_weights(M).to_numpy()
    assert_array_equal(B.view(np.uint32), ref.weights32(P).view(np.uint32))
    assert np.all(np.diag(B) == 0)


@pytest.mark.parametrize("value", [0.0, np.inf, np.nan])
def test_weights_refuse_a_bad_diagonal(gpu, value):
    P = ref.lapack32_inverse(ref.spd_case(65)[0]).astype(np.float32)
    P[17, 17] = value
    M = gpu.Matrix(P.copy())
    with pytest.raises(ValueError):
        gpu.ease_weights(M)
    assert_array_equal(M.to_numpy().view(np.uint32), P.view(np.uint32))  # untouched
    with pytest.raises(ValueError):
        gpu.ease_weights(gpu.Matrix.zeros(3, 4))


# ---- top-k ----------------------------------------------------------------------------------------------------------------
_topk = {}


def topk_setup(gpu, items):
    if items not in _topk:
        B, rows = ref.topk_case(items)
        _topk[items] = (B, rows, gpu.Matrix(B), {})
    return _topk[items]


def expected(items, k, liked, filt):
    B, rows, _, memo = _topk[items]
    key = (k, liked, None if filt is None else tuple(filt))
    if key not in memo:
        memo[key] = ref.recommend32(B, rows, k, liked, filt)
    return memo[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("items", ref.TOPK_ITEMS)
@pytest.mark.parametrize("k", [1, 10, 1024])
def test_topk_bitwise(gpu, items, k):
    B, rows, dB, _ = topk_setup(gpu, items)
    knn = gpu.KnnQuery()
    filt = np.unique(np.array([0, items // 3, items - 1], dtype=np.int32))
    for liked, f in ((False, None), (True, None), (False, filt), (True, filt)):
        ids, scores = gpu.ease_topk(knn, dB, rows, k, liked, f)
        want_ids, want_scores = expected(items, k, liked, f)
        assert_array_equal(ids, want_ids)
        assert_array_equal(bits(scores), bits(want_scores))
    if k > items:  # padding
        assert np.all(ids[:, items:] == -1) and np.all(scores[:, items:] == -ref.FLT_MAX)


@pytest.mark.parametrize("items", [257, 5000])
def test_topk_chunking_changes_nothing(gpu, items):
    B, rows, dB, _ = topk_setup(gpu, items)
    whole = gpu.ease_topk(gpu.KnnQuery(), dB, rows, 10, True)
    per_row = max(rows.getnnz(axis=1)) * 8 + 8 + ((items + 2047) // 2048) * 10 * 8 + 10 * 8
    small = gpu.ease_topk(gpu.KnnQuery(max_temp_memory=int(per_row) + 64), dB, rows, 10, True)  # one or two rows per chunk
    assert_array_equal(whole[0], small[0])
    assert_array_equal(bits(whole[1]), bits(small[1]))
    assert_array_equal(whole[0], expected(items, 10, True, None)[0])
    with pytest.raises(ValueError):
        gpu.ease_topk(gpu.KnnQuery(max_temp_memory=64), dB, rows, 10, True)  # a single row does not fit


def test_topk_rejects(gpu):
    B, rows, dB, _ = topk_setup(gpu, 70)
    knn = gpu.KnnQuery()
    ok = gpu.ease_topk(knn, dB, rows, 3)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError):
            gpu.ease_topk(knn, dB, rows, k)
    with pytest.raises(ValueError):
        gpu.ease_topk(knn, gpu.Matrix.zeros(70, 69), rows, 3)
    with pytest.raises(ValueError):
        gpu.ease_topk(knn, gpu.Matrix(np.zeros((70, 70), dtype=np.float16)), rows, 3)
    unsorted = sp.csr_matrix((np.ones(2, np.float32), np.array([5, 2], np.int32), np.array([0, 2])), shape=(1, 70))
    repeated = sp.csr_matrix((np.ones(2, np.float32), np.array([5, 5], np.int32), np.array([0, 2])), shape=(1, 70))
    outside = sp.csr_matrix((np.ones(1, np.float32), np.array([70], np.int32), np.array([0, 1])), shape=(1, 71))
    for bad in (unsorted, repeated, outside):
        with pytest.raises(ValueError):
            gpu.ease_topk(knn, dB, bad, 3)
    with pytest.raises(ValueError):
        gpu.ease_topk(knn, dB, rows, 3, item_filter=np.array([70], dtype=np.int32))
    again = gpu.ease_topk(knn, dB, rows, 3)
    assert_array_equal(ok[0], again[0])
    assert_array_equal(bits(ok[1]), bits(again[1]))


# ---- model ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return ref.golden()


@pytest.fixture(scope="module")
def fitted(gpu, gold):
    from implicit_amd.ease import EASE

    model = EASE(regularization=float(gold["regularization"]))
    X = sp.csr_matrix(gold["X"])
    model.fit(X, show_progress=False)
    return model, X, model.item_weights.to_numpy()


def test_fit_matches_the_golden_weights(gold, fitted):
    model, X, B = fitted
    B64 = gold["B"]
    B_ref = ref.weights32(ref.lapack32_inverse(ref.gram64(gold["X"], float(gold["regularization"])).astype(np.float32)))
    d_ref, d_gpu = ref.rel_distance(B_ref, B64), ref.rel_distance(B, B64)
    print(f"EASE.fit golden: d_ref={d_ref:.3e} d_gpu={d_gpu:.3e}")
    assert B.dtype == np.float32 and np.all(np.diag(B) == 0)
    assert d_gpu <= max(2 * d_ref, FLOOR)


def test_recommend_is_the_restatement_on_the_models_own_weights(gold, fitted):
    model, X, B = fitted
    users = np.arange(X.shape[0])
    ids, scores = model.recommend(users, X, N=7)
    want_ids, want_scores = ref.recommend32(B, X, 7, True)
    assert_array_equal(ids, want_ids)
    assert_array_equal(bits(scores), bits(want_scores))
    ids, scores = model.recommend(users, X, N=7, filter_already_liked_items=False)
    want_ids, want_scores = ref.recommend32(B, X, 7, False)
    assert_array_equal(ids, want_ids)
    assert_array_equal(bits(scores), bits(want_scores))
    # the float64 top-5 of the golden users
    got, _ = model.recommend(gold["users"], X[gold["users"]], N=5)
    assert_array_equal(got, gold["top_ids"])


def test_scalar_and_batch_forms_agree(fitted):
    model, X, _ = fitted
    ids, scores = model.recommend(np.arange(6), X[:6], N=4)
    for u in range(6):
        i, s = model.recommend(u, X[u], N=4)
        assert i.dtype == np.int32 and s.dtype == np.float32 and i.shape == (4,)
        assert_array_equal(i, ids[u])
        assert_array_equal(bits(s), bits(scores[u]))
    with pytest.raises(ValueError):
        model.recommend(np.arange(6), X[:5])
    with pytest.raises(ValueError):
        model.recommend(0, X[0].tocoo())
    assert_array_equal(model.recommend(3, X[3], N=4, recalculate_user=True)[0], ids[3])


def test_filter_items_and_items(fitted):
    model, X, B = fitted
    users = np.arange(8)
    filt = np.array([3, 11, 25], dtype=np.int32)
    ids, scores = model.recommend(users, X[:8], N=6, filter_items=filt)
    want = ref.recommend32(B, X[:8], 6, True, filt)
    assert_array_equal(ids, want[0])
    assert_array_equal(bits(scores), bits(want[1]))
    assert not np.isin(ids, filt).any()
    items = np.array([30, 2, 17, 9, 21, 38, 5, 12], dtype=np.int32)
    ids, scores = model.recommend(users, X[:8], N=5, items=items, filter_already_liked_items=False)
    other = np.setdiff1d(np.arange(40), items)
    want = ref.recommend32(B, X[:8], 5, False, other)
    assert_array_equal(ids, want[0])
    assert_array_equal(bits(scores), bits(want[1]))
    assert np.isin(ids, items).all()
    short = np.array([4, 19, 33], dtype=np.int32)  # fewer than N
    ids, scores = model.recommend(users, X[:8], N=5, items=short, filter_already_liked_items=False)
    assert ids.shape == (8, 5) and np.all(ids[:, 3:] == -1) and np.all(scores[:, 3:] == -ref.FLT_MAX)
    assert np.all(np.sort(ids[:, :3], axis=1) == short)
    assert model.recommend(0, X[0], N=5, items=short, filter_already_liked_items=False)[0].shape == (3,)
    with pytest.raises(ValueError):
        model.recommend(users, X[:8], filter_items=filt, items=items)
    with pytest.raises(IndexError):
        model.recommend(users, X[:8], items=np.array([40]))


def test_similar_items(fitted):
    model, _, B = fitted
    for item in (0, 13, 39):
        ids, scores = model.similar_items(item, N=6)
        row = B[item].copy()
        row[item] = -np.inf
        order = np.lexsort((-np.arange(40), -row.astype(np.float64)))[:6]
        assert item not in ids
        assert_array_equal(ids, order)
        assert_array_equal(bits(scores), bits(np.where(row[order] == 0, np.float32(0), row[order]).astype(np.float32)))
    batch_ids, _ = model.similar_items(np.array([0, 13, 39]), N=6)
    assert_array_equal(batch_ids[1], model.similar_items(13, N=6)[0])
    everything, _ = model.similar_items(5, N=40)  # the item itself is not returned even when everything else is
    assert len(everything) == 39 and 5 not in everything
    with pytest.raises(NotImplementedError):
        model.similar_users(0)
    with pytest.raises(NotImplementedError):
        model.similar_items(0, recalculate_item=True)


def test_save_load_and_pickle_round_trips(fitted, tmp_path):
    from implicit_amd.ease import EASE

    model, X, B = fitted
    want = model.recommend(np.arange(10), X[:10], N=5)
    path = str(tmp_path / "ease_model.npz")
    model.save(path)
    buf = io.BytesIO()
    model.save(buf)
    buf.seek(0)
    for other in (EASE.load(path), EASE.load(buf), pickle.loads(pickle.dumps(model))):
        assert other.regularization == model.regularization
        assert_array_equal(bits(other.item_weights.to_numpy()), bits(B))
        got = other.recommend(np.arange(10), X[:10], N=5)
        assert_array_equal(got[0], want[0])
        assert_array_equal(bits(got[1]), bits(want[1]))
    unfitted = pickle.loads(pickle.dumps(EASE(regularization=3.0)))
    assert unfitted.item_weights is None and unfitted.regularization == 3.0


def test_fit_errors(gpu, monkeypatch):
    from implicit_amd.ease import EASE

    D = ref.golden()["X"].copy()
    X = sp.csr_matrix(D)
    with pytest.raises(NotImplementedError):
        EASE().fit(X, callback=lambda *a: None)
    D[:, 5] = D[:, 4]  # a duplicated item column: X^T X is singular, and lambda = -1 makes a non-positive pivot certain
    with pytest.raises(ValueError, match="not positive definite at item"):
        EASE(regularization=-1.0).fit(sp.csr_matrix(D))
    import implicit_amd.gpu as g

    monkeypatch.setattr(g, "mem_get_info", lambda: (1000, 2000))
    with pytest.raises(MemoryError, match="12800.*1000"):
        EASE().fit(X)


def test_fit_sums_duplicates(gpu):
    from implicit_amd.ease import EASE

    X = sp.csr_matrix(ref.golden()["X"])
    # every entry stored twice with half its value (the values are multiples of 0.5: the halves add up exactly)
    dup = sp.csr_matrix((np.repeat(X.data / 2, 2), np.repeat(X.indices, 2), X.indptr * 2), shape=X.shape)
    assert not dup.has_canonical_format and dup.nnz == 2 * X.nnz
    a, b = EASE(regularization=5.0), EASE(regularization=5.0)
    a.fit(X)
    b.fit(dup)
    assert_array_equal(bits(a.item_weights.to_numpy()), bits(b.item_weights.to_numpy()))


def test_ranking_metrics_on_a_planted_block_problem(gpu):
    from implicit_amd.ease import EASE
    from implicit_amd.evaluation import leave_k_out_split, ranking_metrics_at_k

    rng = np.random.default_rng(11)
    groups, per_group, users = 8, 12, 400
    items = groups * per_group
    D = np.zeros((users, items), dtype=np.float32)
    for u in range(users):
        g = u % groups
        liked = rng.choice(per_group, size=7, replace=False) + g * per_group
        D[u, liked] = 1.0
    D[rng.random((users, items)) < 0.01] = 1.0  # noise
    D[:, :3] = np.maximum(D[:, :3], (rng.random((users, 3)) < 0.5).astype(np.float32))  # globally popular items
    train, test = leave_k_out_split(sp.csr_matrix(D), K=2, random_state=3)
    model = EASE(regularization=10.0)
    model.fit(train, show_progress=False)
    m = ranking_metrics_at_k(model, train, test, K=10, show_progress=False)
    assert set(m) == {"precision", "map", "ndcg", "auc"}
    # the most-popular-items ranking, liked items filtered
    pop = np.asarray(train.sum(axis=0)).ravel()
    hits = total = 0
    for u in np.flatnonzero(np.diff(test.indptr) > 0):
        s = pop.astype(np.float64).copy()
        s[train.indices[train.indptr[u]:train.indptr[u + 1]]] = -np.inf
        top = np.argsort(-s, kind="stable")[:10]
        held = test.indices[test.indptr[u]:test.indptr[u + 1]]
        hits += len(np.intersect1d(top, held))
        total += min(10, len(held))
    print("planted blocks: precision@10 EASE", m["precision"], "popularity", hits / total)
    assert m["precision"] > hits / total
