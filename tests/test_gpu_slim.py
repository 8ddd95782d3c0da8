"""SLIM on the device (csrc/slim.hip, implicit_amd/slim.py) on the inputs of tests/slim_reference.py.

imp_slim_solve is defined operation for operation: every comparison with solve32 is bit for bit, weights and sweep counts.  The
sizes straddle the two sizes at which the kernel changes path: the chunk width (1024 coordinates, one per thread: 1023, 1024, 1025)
and the grid, min(items, 2 x compute units) workgroups = 512 on MI355X, past which a workgroup draws a second column and zeroes r
and its row of W again (511, 512, 513; on a device with another CU count these are three more ordinary sizes).  The model is
held to scikit-learn's float64 optimum within the distance tests/test_slim_host.py measured for solve32, which the device equals."""
import io
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_equal

import ease_reference as eref
import slim_reference as ref

pytestmark = pytest.mark.gpu

bits = ref.bits
GRID = 512  # 2 workgroups per compute unit of MI355X: items above it share workgroups
SIZES = sorted(set(ref.SIZES) | {GRID - 1, GRID, GRID + 1})
_device = {}


def device_case(gpu, n):
    if n not in _device:
        _device[n] = gpu.Matrix(np.array(ref.case(n)[0]))
    return _device[n]


def solve(gpu, n, l1, positive, max_sweeps, tol, W=None):
    W, sweeps = gpu.slim_solve(device_case(gpu, n), l1, positive, max_sweeps, tol, W)
    return W.to_numpy(), sweeps


def check_shape_of_the_answer(W, sweeps, positive, empty, max_sweeps):
    assert W.dtype == np.float32 and sweeps.dtype == np.int32
    assert not bits(np.diag(W)).any()  # +0, not -0
    assert sweeps.min() >= 1 and sweeps.max() <= max_sweeps
    if positive:
        assert np.all(W >= 0)
    if empty is not None:
        assert not W[empty].any() and not W[:, empty].any() and sweeps[empty] == 1


# ---- bitwise against solve32 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ref.SETTINGS, ids=lambda s: f"sweeps{s[0]}-tol{s[1]:g}")
@pytest.mark.parametrize("positive", [True, False], ids=["positive", "signed"])
@pytest.mark.parametrize("n", SIZES)
def test_solve_bitwise(gpu, n, positive, setting):
    max_sweeps, tol = setting
    A, empty, twins = ref.case(n)
    W, sweeps = solve(gpu, n, ref.L1, positive, max_sweeps, tol)
    check_shape_of_the_answer(W, sweeps, positive, empty, max_sweeps)
    for j in ref.columns(n, A, empty, twins):
        w, s = ref.expected(n, j, ref.L1, positive, max_sweeps, tol)
        assert sweeps[j] == s, (j, int(sweeps[j]), s)
        assert_array_equal(bits(W[:, j]), bits(w), err_msg=f"column {j}")


# ---- edges of the skip logic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("positive", [True, False], ids=["positive", "signed"])
def test_no_l1_moves_every_coordinate(gpu, positive):
    n, max_sweeps = 65, 20
    A, empty, _ = ref.case(n)
    W, sweeps = solve(gpu, n, 0.0, positive, max_sweeps, 0.0)
    check_shape_of_the_answer(W, sweeps, positive, empty, max_sweeps)
    for j in range(n):
        w, s = ref.expected(n, j, 0.0, positive, max_sweeps, 0.0)
        assert sweeps[j] == s
        assert_array_equal(bits(W[:, j]), bits(w), err_msg=f"column {j}")
    if not positive:
        assert np.count_nonzero(W) > 0.8 * n * (n - 3)  # dense but for the diagonal and the empty item: the worst case of the loop


@pytest.mark.parametrize("n", [65, ref.CHUNK + 1])
def test_l1_above_every_entry_leaves_nothing(gpu, n):
    A = ref.case(n)[0]
    for positive in (True, False):
        W, sweeps = solve(gpu, n, float(np.abs(A).max()) * 2, positive, 100, 1e-4)
        assert not bits(W).any()
        assert_array_equal(sweeps, np.ones(n, dtype=np.int32))


def test_sweeps_may_be_null(gpu):
    from implicit_amd.gpu import _hip

    n = 65
    want, _ = solve(gpu, n, ref.L1, True, 100, 1e-4)
    W = gpu.Matrix(np.full((n, n), np.nan, dtype=np.float32))
    _hip.check(_hip.lib().imp_slim_solve(device_case(gpu, n)._h, ref.L1, 1, 100, 1e-4, W._h, None))
    assert_array_equal(bits(W.to_numpy()), bits(want))


# ---- independence from earlier calls ------------------------------------------------------------------------------------------
def test_answers_do_not_depend_on_earlier_calls(gpu):
    n = 257
    first_W, first_s = solve(gpu, n, ref.L1, False, 100, 1e-4)
    again_W, again_s = solve(gpu, n, ref.L1, False, 100, 1e-4)
    assert_array_equal(bits(again_W), bits(first_W))
    assert_array_equal(again_s, first_s)
    solve(gpu, ref.CHUNK + 1, ref.L1, True, 5, 0.0)  # another order: the workspace grows, the ticket and the counts move
    solve(gpu, 2, ref.L1, True, 5, 0.0)
    garbage = gpu.Matrix(np.full((n, n), np.nan, dtype=np.float32))
    W, s = solve(gpu, n, ref.L1, False, 100, 1e-4, garbage)
    assert_array_equal(bits(W), bits(first_W))
    assert_array_equal(s, first_s)
    gpu.release_workspaces()
    W, s = solve(gpu, n, ref.L1, False, 100, 1e-4)
    assert_array_equal(bits(W), bits(first_W))
    assert_array_equal(s, first_s)
    updates, longest = gpu.slim_stats()
    assert updates >= np.count_nonzero(first_W) and longest > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
SENTINEL = 7.5


def sentinel(gpu, n, dtype=np.float32):
    return gpu.Matrix(np.full((n, n), SENTINEL, dtype=dtype))


def refused(gpu, A, W, l1=1.0, positive=True, max_sweeps=10, tol=1e-4, match=None):
    with pytest.raises(ValueError, match=match):
        gpu.slim_solve(A, l1, positive, max_sweeps, tol, W)
    assert np.all(W.to_numpy() == SENTINEL)


def test_refusals_leave_W_untouched(gpu):
    from implicit_amd.gpu import _hip

    n = 65
    A, W = device_case(gpu, n), sentinel(gpu, n)
    for l1 in (-1.0, np.nan, np.inf):
        refused(gpu, A, W, l1=l1, match="l1")
    for tol in (-1e-4, np.nan, np.inf):
        refused(gpu, A, W, tol=tol, match="tol")
    for max_sweeps in (0, -3):
        refused(gpu, A, W, max_sweeps=max_sweeps, match="max_sweeps")
    refused(gpu, gpu.Matrix(np.ones((n, n + 1), dtype=np.float32)), W, match="square")
    refused(gpu, gpu.Matrix(np.ones((n + 1, n + 1), dtype=np.float32)), W, match="same order")
    refused(gpu, gpu.Matrix(np.ones((n, n), dtype=np.float16)), W, match="float32")
    with pytest.raises(ValueError, match="square"):
        gpu.slim_solve(A, 1.0, W=gpu.Matrix(np.ones((n, n - 1), dtype=np.float32)))
    with pytest.raises(ValueError, match="float32"):
        gpu.slim_solve(A, 1.0, W=sentinel(gpu, n, np.float16))
    # A and W sharing storage: the same matrix, and a view of it
    shared = sentinel(gpu, n)
    refused(gpu, shared, shared, match="share storage")
    refused(gpu, shared[0:n], shared, match="share storage")
    # NULL arguments reach the library only through the C-ABI
    for a, w in ((None, W._h), (A._h, None)):
        status = _hip.lib().imp_slim_solve(a, 1.0, 1, 10, 1e-4, w, None)
        assert status == _hip.IMP_INVALID_ARGUMENT
        with pytest.raises(ValueError, match="NULL"):
            _hip.check(status)
    assert np.all(W.to_numpy() == SENTINEL)
    # the library works afterwards
    got, _ = solve(gpu, n, ref.L1, True, 100, 1e-4)
    assert_array_equal(bits(got[:, 0]), bits(ref.expected(n, 0, ref.L1, True, 100, 1e-4)[0]))


@pytest.mark.parametrize("value", [0.0, -2.0, np.nan, np.inf])
def test_a_bad_diagonal_is_refused_and_named(gpu, value):
    n = 300
    A = np.array(ref.case(257)[0])
    A = np.pad(A, ((0, n - 257), (0, n - 257)))
    A[np.arange(257, n), np.arange(257, n)] = 3.0
    A[290, 290] = value
    A[41, 41] = value  # the smallest one is named
    W = sentinel(gpu, n)
    refused(gpu, gpu.Matrix(A), W, match="item 41 ")


def test_more_items_than_the_cap_are_refused(gpu):
    n = ref.MAX_ITEMS + 1
    A, W = gpu.Matrix.zeros(n, n), gpu.Matrix.zeros(n, n)
    edge = np.full((2, n), SENTINEL, dtype=np.float32)
    W[0:2].copy_from_numpy(edge)
    W[n - 2:n].copy_from_numpy(edge)
    with pytest.raises(ValueError, match=f"at most {ref.MAX_ITEMS}"):
        gpu.slim_solve(A, 1.0, W=W)
    assert np.all(W[0:2].to_numpy() == SENTINEL) and np.all(W[n - 2:n].to_numpy() == SENTINEL)
    with pytest.raises(ValueError, match=f"at most {ref.MAX_ITEMS}"):
        gpu.slim_solve(A, 1.0)  # the shim says the same before it allocates W


# ---- model --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return ref.golden()


def fit_golden(gold, setting, positive):
    from implicit_amd.slim import SLIM

    model = SLIM(l1_regularization=float(gold["l1"][setting]), l2_regularization=float(gold["l2"][setting]), positive=positive,
                 max_sweeps=ref.GOLDEN_MAX_SWEEPS, tol=ref.GOLDEN_TOL)
    model.fit(sp.csr_matrix(gold["X"]), show_progress=False)
    return model


@pytest.fixture(scope="module")
def fitted(gpu, gold):
    model = fit_golden(gold, 0, True)
    return model, sp.csr_matrix(gold["X"]), model.item_weights.to_numpy()


@pytest.mark.parametrize("setting", [0, 1])
@pytest.mark.parametrize("positive", [True, False], ids=["positive", "signed"])
def test_fit_matches_the_golden_weights(gpu, gold, setting, positive):
    model = fit_golden(gold, setting, positive)
    W = model.item_weights.to_numpy()
    distance, support = ref.column_distance(W, gold["W"][setting, int(positive)])
    print(f"SLIM.fit against scikit-learn, setting {setting} positive={positive}: distance {distance:.6e}, support difference {support}")
    assert distance <= 2 * ref.GOLDEN_DISTANCE[(setting, positive)] and support == 0
    assert model.sweeps_.dtype == np.int32 and model.sweeps_.shape == (40,) and model.sweeps_.max() < ref.GOLDEN_MAX_SWEEPS
    assert model.density == np.count_nonzero(W) / (40 * 39)
    S = model.sparse_weights()
    assert sp.isspmatrix_csr(S) and S.dtype == np.float32 and S.nnz == np.count_nonzero(W)
    assert_array_equal(bits(S.toarray()), bits(W))
    # the device is solve32: the exact Gram matrix of the integer X, the same rule
    A = eref.gram64(gold["X"], float(gold["l2"][setting])).astype(np.float32)
    for j in (0, 4, 5, 38, 39):
        w, s = ref.solve32(A, j, float(gold["l1"][setting]), positive, ref.GOLDEN_MAX_SWEEPS, ref.GOLDEN_TOL)
        assert_array_equal(bits(W[:, j]), bits(w))
        assert model.sweeps_[j] == s


def test_recommend_is_the_restatement_on_the_models_own_weights(fitted):
    model, X, W = fitted
    users = np.arange(X.shape[0])
    for liked in (True, False):
        ids, scores = model.recommend(users, X, N=7, filter_already_liked_items=liked)
        want_ids, want_scores = eref.recommend32(W, X, 7, liked)
        assert_array_equal(ids, want_ids)
        assert_array_equal(bits(scores), bits(want_scores))
    filt = np.array([3, 11, 25], dtype=np.int32)
    ids, scores = model.recommend(users[:8], X[:8], N=6, filter_items=filt)
    want = eref.recommend32(W, X[:8], 6, True, filt)
    assert_array_equal(ids, want[0])
    assert_array_equal(bits(scores), bits(want[1]))
    items = np.array([30, 2, 17, 9, 21, 37, 5, 12], dtype=np.int32)
    ids, scores = model.recommend(users[:8], X[:8], N=5, items=items, filter_already_liked_items=False)
    want = eref.recommend32(W, X[:8], 5, False, np.setdiff1d(np.arange(40), items))
    assert_array_equal(ids, want[0])
    assert_array_equal(bits(scores), bits(want[1]))
    assert np.isin(ids, items).all()
    with pytest.raises(ValueError):
        model.recommend(users[:8], X[:8], filter_items=filt, items=items)


def test_scalar_and_batch_forms_agree(fitted):
    model, X, _ = fitted
    ids, scores = model.recommend(np.arange(6), X[:6], N=4)
    for u in range(6):
        i, s = model.recommend(u, X[u], N=4)
        assert i.dtype == np.int32 and s.dtype == np.float32
        keep = ids[u] >= 0
        assert_array_equal(i, ids[u][keep])
        assert_array_equal(bits(s), bits(scores[u][keep]))


def test_similar_items_and_similar_users(fitted):
    from implicit_amd.slim import SLIM

    model, _, W = fitted
    for item in (0, 13, 38, 39):
        ids, scores = model.similar_items(item, N=6)
        row = W[item].copy()
        row[item] = -np.inf
        order = np.lexsort((-np.arange(40), -row.astype(np.float64)))[:6]
        assert item not in ids
        assert_array_equal(ids, order)
        assert_array_equal(bits(scores), bits(row[order]))
    batch_ids, _ = model.similar_items(np.array([0, 13, 39]), N=6)
    assert_array_equal(batch_ids[1], model.similar_items(13, N=6)[0])
    everything, _ = model.similar_items(5, N=40)
    assert len(everything) == 39 and 5 not in everything
    with pytest.raises(NotImplementedError, match="SLIM"):
        model.similar_users(0)
    with pytest.raises(ValueError, match="SLIM"):
        SLIM().recommend(0, sp.csr_matrix((1, 40), dtype=np.float32))


def test_save_load_and_pickle_round_trips(fitted, tmp_path):
    from implicit_amd.slim import SLIM

    model, X, W = fitted
    want = model.recommend(np.arange(10), X[:10], N=5)
    path = str(tmp_path / "slim_model.npz")
    model.save(path)
    buf = io.BytesIO()
    model.save(buf)
    buf.seek(0)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"l1_regularization", "l2_regularization", "positive", "max_sweeps", "tol", "sweeps_", "indptr",
                                "indices", "data", "shape"}
        assert all(z[k].size < 40 * 40 for k in z.files)  # no dense items^2 array
        assert z["data"].size == np.count_nonzero(W)
    for other in (SLIM.load(path), SLIM.load(buf), pickle.loads(pickle.dumps(model))):
        for name in ("l1_regularization", "l2_regularization", "positive", "max_sweeps", "tol", "density"):
            assert getattr(other, name) == getattr(model, name), name
        assert_array_equal(bits(other.item_weights.to_numpy()), bits(W))
        assert other.sweeps_.dtype == np.int32
        assert_array_equal(other.sweeps_, model.sweeps_)
        got = other.recommend(np.arange(10), X[:10], N=5)
        assert_array_equal(got[0], want[0])
        assert_array_equal(bits(got[1]), bits(want[1]))
    unfitted = pickle.loads(pickle.dumps(SLIM(l1_regularization=3.0, positive=False)))
    assert unfitted.item_weights is None and unfitted.l1_regularization == 3.0 and unfitted.positive is False


def test_fit_errors(gpu, gold, monkeypatch):
    from implicit_amd.slim import SLIM

    X = sp.csr_matrix(gold["X"])
    with pytest.raises(NotImplementedError, match="SLIM"):
        SLIM().fit(X, callback=lambda *a: None)
    with pytest.raises(ValueError, match="not positive at item 38; raise l2_regularization"):
        SLIM(l2_regularization=0.0).fit(X)  # the item nobody has
    wide = sp.csr_matrix((1, ref.MAX_ITEMS + 1), dtype=np.float32)
    with pytest.raises(ValueError, match=f"at most {ref.MAX_ITEMS}"):
        SLIM().fit(wide)
    import implicit_amd.gpu as g

    need = 2 * 40 * 40 * 4 + g.slim_workspace_bytes(40)
    monkeypatch.setattr(g, "mem_get_info", lambda: (need - 1, 2 * need))
    with pytest.raises(MemoryError, match=f"{need}.*{need - 1}"):
        SLIM().fit(X)
    monkeypatch.setattr(g, "mem_get_info", lambda: (need, 2 * need))
    SLIM().fit(X)


def test_fit_sums_duplicates(gpu, gold):
    from implicit_amd.slim import SLIM

    X = sp.csr_matrix(gold["X"])
    # every entry stored twice with half its value (the values are integers: the halves add up exactly)
    dup = sp.csr_matrix((np.repeat(X.data / 2, 2), np.repeat(X.indices, 2), X.indptr * 2), shape=X.shape)
    assert not dup.has_canonical_format and dup.nnz == 2 * X.nnz
    a, b = SLIM(), SLIM()
    a.fit(X)
    b.fit(dup)
    assert_array_equal(bits(a.item_weights.to_numpy()), bits(b.item_weights.to_numpy()))
    assert_array_equal(a.sweeps_, b.sweeps_)


def test_ranking_metrics_on_a_planted_block_problem(gpu):
    from implicit_amd.evaluation import leave_k_out_split, ranking_metrics_at_k
    from implicit_amd.slim import SLIM

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
    model = SLIM()
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
    print("planted blocks: precision@10 SLIM", m["precision"], "popularity", hits / total, "density", model.density)
    assert m["precision"] > hits / total
    assert 0 < model.density < 1
