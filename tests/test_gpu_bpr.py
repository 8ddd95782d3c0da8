"""BPR training on the device (imp_bpr_update / bpr_epoch, csrc/bpr.hip) and the model built on it (implicit_amd.gpu.bpr),
judged against the float64 restatement of the contract in bpr_reference.py."""
import io
import pickle

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import csr_matrix

import bpr_reference as ref
import sgd_cases as sc

pytestmark = pytest.mark.gpu

LR, REG = 0.05, 0.01


def _small_matrix(users=40, items=150, seed=0):
    """Skewed popularity (the first items in most rows, so i == j happens without verification), rows of about 70 sorted
    entries (longer than a lane group: the negative check's splitter levels run), one empty user."""
    rng = np.random.default_rng(seed)
    dense = rng.random((users, items)) < np.linspace(0.95, 0.02, items)[None, :]
    dense[3] = False
    return csr_matrix(dense.astype(np.float32))


def _factors(rows, C, rng, bias=None):
    a = (rng.standard_normal((rows, C)) * 0.3).astype(np.float32)
    if bias is not None:
        a[:, C - 1] = bias
    return a


def _device_ids(gpu, m):
    userids, itemids = ref.coo_ids(m)
    return gpu.IntVector(userids), gpu.IntVector(itemids), gpu.IntVector(np.asarray(m.indptr, dtype=np.int32))


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _check_against(Xg, Yg, X64, Y64, X0, Y0, users, items):
    """Touched rows within 2e-6 relative (row norms), every other row bitwise unchanged, user bias exactly 1."""
    for u in range(X0.shape[0]):
        if u in users:
            assert _rel(Xg[u], X64[u]) < 2e-6, ("user", u)
        else:
            assert_array_equal(Xg[u], X0[u])
    for i in range(Y0.shape[0]):
        if i in items:
            assert _rel(Yg[i], Y64[i]) < 2e-6, ("item", i)
        else:
            assert_array_equal(Yg[i], Y0[i])
    assert (Xg[:, -1] == 1.0).all()


def _check_call(Xg, Yg, X64, Y64, X0, Y0, users, items):
    """_check_against for large matrices: the untouched rows are compared in one piece."""
    for u in users:
        assert _rel(Xg[u], X64[u]) < 2e-6, ("user", u)
    for i in items:
        assert _rel(Yg[i], Y64[i]) < 2e-6, ("item", i)
    untouched_u = np.array(sorted(set(range(X0.shape[0])) - set(users)))
    untouched_i = np.array(sorted(set(range(Y0.shape[0])) - set(items)))
    assert_array_equal(Xg[untouched_u].view(np.uint32), X0[untouched_u].view(np.uint32))
    assert_array_equal(Yg[untouched_i].view(np.uint32), Y0[untouched_i].view(np.uint32))
    assert (Xg[:, -1] == 1.0).all()


# ---- 1. single samples are exact ----------------------------------------------------------------------------------------
def _single_steps_exact(gpu, C, verify):
    m = _small_matrix()
    rng = np.random.default_rng(C * 2 + verify)
    X0, Y0 = _factors(m.shape[0], C, rng, bias=1.0), _factors(m.shape[1], C, rng)
    X0[3] = 0.0
    X0[3, -1] = 1.0
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    # 25 calls with fresh seeds; up to 8 of them chosen for an i == j sample (no verification) or a skipped one (verification)
    special, plain = [], []
    for s in (int(v) for v in rng.integers(0, 2**62, 2000)):
        u, i, j = (int(v[0]) for v in ref.sample_ids(m, s, 1))
        hit = bool(ref.liked(m, [u], [j])[0]) if verify else i == j
        (special if hit else plain).append(s)
        if len(special) >= 8 and len(plain) >= 17:
            break
    assert len(special) >= 3
    picked = special[:8] + plain[:25 - len(special[:8])]
    rng.shuffle(picked)
    Xc, Yc = X0.copy(), Y0.copy()
    for s in picked:
        u, i, j = (int(v[0]) for v in ref.sample_ids(m, s, 1))
        sk = verify and bool(ref.liked(m, [u], [j])[0])
        X64, Y64 = Xc.astype(np.float64), Yc.astype(np.float64)
        score = 0.0 if sk else ref.step64(X64, Y64, u, i, j, LR, REG)
        correct, skipped = gpu.bpr_epoch(uid, iid, ptr, X, Y, LR, REG, s, verify, samples=1)
        assert skipped == int(sk)
        if not sk and abs(score) >= 1e-6:
            assert correct == int(score > 0)
        Xg, Yg = X.to_numpy(), Y.to_numpy()
        _check_against(Xg, Yg, X64, Y64, Xc, Yc, set() if sk else {u}, set() if sk else {i, j})
        Xc, Yc = Xg, Yg


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("C", sc.DISPATCH_C)  # both ends of every (lanes, columns per lane) instantiation
def test_single_steps_exact(gpu, C, verify):
    _single_steps_exact(gpu, C, verify)


@pytest.mark.parametrize("lanes, C", [(lanes, C) for lanes, C, _ in sc.LANE_OVERRIDES])
def test_lane_override_routes(gpu, monkeypatch, lanes, C):
    """IMP_BPR_LANES is read by every call (bpr_group): other group widths than the dispatch picks reach the twelve
    instantiations nothing else does (sgd_cases.LANE_OVERRIDES).  16 lanes at C = 257 cannot hold a row in 16 registers a
    lane: there the switch is ignored."""
    monkeypatch.setenv("IMP_BPR_LANES", str(lanes))
    _single_steps_exact(gpu, C, True)
    _single_steps_exact(gpu, C, False)


# ---- 2. a multi-sample call without conflicts is exact --------------------------------------------------------------------
@pytest.mark.parametrize("C", [17, 101, 257, 1024])
def test_conflict_free_call_exact(gpu, C):
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(4000, 20000, 60_000, gamma=1.0, seed=3)
    n = 64
    for seed in range(1, 5000):
        u, i, j = ref.sample_ids(m, seed, n)
        if len(set(u.tolist())) == n and len(set(i.tolist()) | set(j.tolist())) == 2 * n:
            break
    else:
        pytest.fail("no conflict-free seed found")
    rng = np.random.default_rng(C)
    X0, Y0 = _factors(m.shape[0], C, rng, bias=1.0), _factors(m.shape[1], C, rng)
    X64, Y64 = X0.astype(np.float64), Y0.astype(np.float64)
    correct = sum(ref.step64(X64, Y64, a, b, c, LR, REG) > 0 for a, b, c in zip(u.tolist(), i.tolist(), j.tolist()))
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    got = gpu.bpr_epoch(uid, iid, ptr, X, Y, LR, REG, seed, False, samples=n)
    assert got == (correct, 0)
    Xg, Yg = X.to_numpy(), Y.to_numpy()
    touched_u, touched_i = set(u.tolist()), set(i.tolist()) | set(j.tolist())
    assert _rel(Xg[u], X64[u]) < 2e-6 and _rel(Yg[i], Y64[i]) < 2e-6 and _rel(Yg[j], Y64[j]) < 2e-6
    untouched_u = np.array(sorted(set(range(m.shape[0])) - touched_u))
    untouched_i = np.array(sorted(set(range(m.shape[1])) - touched_i))
    assert_array_equal(Xg[untouched_u], X0[untouched_u])
    assert_array_equal(Yg[untouched_i], Y0[untouched_i])
    assert (Xg[:, -1] == 1.0).all()


@pytest.mark.parametrize("C", sc.ROUNDS_C)
def test_conflict_free_call_exact_over_rounds(gpu, C):
    """24 samples on a 256-user matrix: 16 samples in flight, so every group's loop takes a second step for half of the
    groups, with the second sample's draw prefetched during the first (sgd_cases.py, section 2)."""
    m = sc.rounds_matrix()
    n = sc.ROUNDS_N
    seed, u, i, j = sc.bpr_rounds_seed(m)
    X0, Y0 = sc.rounds_factors(m, C)
    X64, Y64 = X0.astype(np.float64), Y0.astype(np.float64)
    correct = sum(ref.step64(X64, Y64, a, b, c, LR, REG) > 0 for a, b, c in zip(u.tolist(), i.tolist(), j.tolist()))
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    got = gpu.bpr_epoch(uid, iid, ptr, X, Y, LR, REG, seed, False, samples=n)
    assert got == (correct, 0)
    Xg, Yg = X.to_numpy(), Y.to_numpy()
    _check_call(Xg, Yg, X64, Y64, X0, Y0, set(u.tolist()), set(i.tolist()) | set(j.tolist()))


# ---- 3. whole epochs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, C", [("ml100k", 65), ("lastfm360k", 101)])
def test_whole_epoch(gpu, name, C):
    from implicit_amd.synthetic import named

    m = named(name, empty_frac=0.02)
    m = csr_matrix((m.data, m.indices, m.indptr), shape=(m.shape[0], m.shape[1] + 64))  # 64 items nobody liked
    m.has_sorted_indices = True
    X0, Y0, _ = ref.init_factors(m, C - 1, 7)
    uid, iid, ptr = _device_ids(gpu, m)
    empty_users = np.diff(m.indptr) == 0
    unused_items = np.bincount(m.indices, minlength=m.shape[1]) == 0
    assert empty_users.any() and unused_items.any()
    for verify in (True, False):
        want = ref.predicted_skipped(m, 1234, verify)
        runs = []
        for _ in range(2):
            X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
            correct, skipped = gpu.bpr_epoch(uid, iid, ptr, X, Y, 0.01, 0.01, 1234, verify)
            runs.append(skipped)
            assert skipped == want
            assert 0 < correct <= m.nnz - skipped
        assert runs[0] == runs[1]
        Xg, Yg = X.to_numpy(), Y.to_numpy()
        assert np.isfinite(Xg).all() and np.isfinite(Yg).all()
        assert_array_equal(Xg[empty_users], X0[empty_users])
        assert_array_equal(Yg[unused_items], Y0[unused_items])
        assert (Xg[:, -1] == 1.0).all()
        assert not np.array_equal(Yg, Y0)
    assert want == 0


@pytest.mark.parametrize("C", sc.SEARCH_C)
def test_zero_learning_rate_epoch_is_exact(gpu, C):
    """lr = reg = 0: every store writes back what its lane loaded, so an epoch -- some 22 000 chained samples, 16 in flight --
    returns counts that are a pure function of the initial factors, and X and Y bit for bit.  The matrix has rows on both
    sides of every cut of the membership search (sgd_cases.search_matrix; tests/test_sgd_cases_host.py shows which hits and
    misses the epoch meets).  `correct` is compared with samples of a float64 |score| < 1e-6 left out: none at these C."""
    m = sc.search_matrix()
    X0, Y0 = sc.bpr_frozen_factors(m, C)
    skipped, correct_lo, unsure, _, _ = sc.bpr_frozen_counts(m, X0, Y0)
    assert skipped == ref.predicted_skipped(m, sc.SEARCH_EPOCH_SEED, True) and unsure <= 0.001 * m.nnz
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    for _ in range(2):
        correct, got_skipped = gpu.bpr_epoch(uid, iid, ptr, X, Y, 0.0, 0.0, sc.SEARCH_EPOCH_SEED, True)
        print(f"C={C}: correct {correct} (float64 {correct_lo} .. {correct_lo + unsure}), skipped {got_skipped} ({skipped})")
        assert got_skipped == skipped
        assert correct_lo <= correct <= correct_lo + unsure
        assert_array_equal(X.to_numpy().view(np.uint32), X0.view(np.uint32))
        assert_array_equal(Y.to_numpy().view(np.uint32), Y0.view(np.uint32))


# ---- 4. learning quality --------------------------------------------------------------------------------------------------
def _planted(seed):
    """Rank-8 planted preferences, 300 users x 200 items, 24 positives per user; one held out per user."""
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((300, 8)), rng.standard_normal((200, 8))
    scores = U @ V.T + 0.5 * rng.standard_normal((300, 200))
    top = np.argsort(-scores, axis=1)[:, :25]
    held = top[np.arange(300), rng.integers(0, 25, 300)]
    train = np.zeros((300, 200), dtype=np.float32)
    train[np.repeat(np.arange(300), 25), top.ravel()] = 1.0
    train[np.arange(300), held] = 0.0
    return csr_matrix(train), held


def _held_out_auc(X, Y, train, held):
    s = X.astype(np.float64) @ Y.astype(np.float64).T
    dense = train.toarray() > 0
    aucs = []
    for u in range(X.shape[0]):
        neg = ~dense[u]
        neg[held[u]] = False
        aucs.append((s[u, neg] < s[u, held[u]]).mean())
    return float(np.mean(aucs))


def test_learning_quality_against_serial(gpu):
    """The GPU model's held-out AUC against the serial float64 SGD over the same draws (the same initial factors, epoch seeds
    and sample sequence; only the Hogwild interleaving differs).  Calibrated on the MI355X, seeds 0 / 1 / 2, 20 epochs,
    factors 8, lr 0.05: GPU - serial = -0.0016 / -0.0051 / -0.0037 (serial AUC 0.921 - 0.925); the margin, 0.02, is the worst
    of the three plus 0.015 of slack."""
    import implicit_amd.gpu.bpr as gbpr

    worst = 1.0
    for seed in range(3):
        train, held = _planted(seed)
        seen = []
        model = gbpr.BayesianPersonalizedRanking(factors=8, learning_rate=0.05, regularization=0.01, iterations=20,
                                                 random_state=seed)
        model.fit(train, show_progress=False, callback=lambda e, t, c, s: seen.append((c, s)))
        auc_gpu = _held_out_auc(model.user_factors.to_numpy(), model.item_factors.to_numpy(), train, held)
        X0, Y0, rs = ref.init_factors(train, 8, seed)
        seeds = [rs.integers(2**31) for _ in range(20)]
        X, Y, counts = ref.serial_epochs(train, X0, Y0, seeds, 0.05, 0.01, True)
        auc_ser = _held_out_auc(X, Y, train, held)
        print(f"seed {seed}: held-out AUC gpu {auc_gpu:.4f} serial {auc_ser:.4f} (diff {auc_gpu - auc_ser:+.4f})")
        worst = min(worst, auc_gpu - auc_ser)
        assert [s for _, s in seen] == [s for _, s in counts]  # the same draws: skipped counts agree exactly
        rate = [c / (train.nnz - s) for c, s in seen]
        assert 0.35 < rate[0] < 0.65 and rate[-1] > 0.8, rate
        assert auc_ser > 0.8
    assert worst > -0.02


# ---- 5. the model -----------------------------------------------------------------------------------------------------------
def _model(**kw):
    import implicit_amd.bpr

    args = dict(factors=16, learning_rate=0.05, regularization=0.01, iterations=3, random_state=42)
    args.update(kw)
    return implicit_amd.bpr.BayesianPersonalizedRanking(**args)


def test_initial_factors_match_reference_formula(gpu):
    m = _small_matrix(users=60, items=50, seed=2)
    model = _model(iterations=0)
    model.fit(m, show_progress=False)
    X0, Y0, _ = ref.init_factors(m, 16, 42)
    assert_array_equal(model.user_factors.to_numpy(), X0)
    assert_array_equal(model.item_factors.to_numpy(), Y0)


def test_callback_and_degenerate_matrices(gpu):
    calls = []
    m = _small_matrix()
    model = _model(iterations=5)
    model.fit(m, show_progress=False, callback=lambda *a: calls.append(a))
    assert len(calls) == 5 and all(len(a) == 4 for a in calls)
    _model().fit(csr_matrix(np.zeros((3, 3), dtype=np.float32)), show_progress=False)
    _model().fit(csr_matrix(np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float32)), show_progress=False)
    model.fit(m.astype(np.float64), show_progress=False)  # non-fp32 input, existing factors kept


def test_unsorted_input_gives_sorted_skips(gpu):
    m = _small_matrix(users=80, items=40, seed=5)
    rev = m.copy()
    for r in range(rev.shape[0]):  # reverse every row's column order
        a, b = rev.indptr[r], rev.indptr[r + 1]
        rev.indices[a:b] = rev.indices[a:b][::-1].copy()
        rev.data[a:b] = rev.data[a:b][::-1].copy()
    rev.has_sorted_indices = False
    skips = {}
    for key, mat in (("sorted", m), ("unsorted", rev)):
        seen = []
        _model(iterations=3).fit(mat, show_progress=False, callback=lambda e, t, c, s: seen.append(s))
        skips[key] = seen
    assert skips["sorted"] == skips["unsorted"] and sum(skips["sorted"]) > 0
    assert rev.has_sorted_indices is False or not np.array_equal(rev.indices, m.indices)  # caller's matrix left alone


def _knn_ids(gpu, Y, Q, k):
    return gpu.KnnQuery().topk(gpu.Matrix(Y), gpu.Matrix(Q), k)[0]


def test_recommend_and_similar_items_follow_factors(gpu):
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(2000, 16000, 60_000, seed=9)
    model = _model(factors=64, learning_rate=0.5, iterations=2)
    users = np.arange(256)
    model.fit(m, show_progress=False)
    ids1, _ = model.recommend(users, m[users], N=10, filter_already_liked_items=False)
    X, Y = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    assert (ids1 == _knn_ids(gpu, Y, X[users], 10)).mean() > 0.99
    sim, _ = model.similar_items(np.arange(32), N=5)
    norms = np.linalg.norm(Y.astype(np.float64), axis=1)
    cos = (Y[:32].astype(np.float64) @ Y.astype(np.float64).T) / np.maximum(norms, 1e-10)[None, :]
    want = np.argsort(-cos, axis=1, kind="stable")[:, :5]
    assert (sim == want).mean() > 0.95
    # a second fit rewrites the item factors in place: the cached planes of the model's KnnQuery must not be used
    model.fit(m, show_progress=False)
    ids2, _ = model.recommend(users, m[users], N=10, filter_already_liked_items=False)
    X2, Y2 = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    want2 = _knn_ids(gpu, Y2, X2[users], 10)
    assert (ids2 == want2).mean() > 0.99
    assert (want2 != ids1).mean() > 0.2  # the factors did change enough for stale planes to show


def test_plane_cache_invalidated_by_bpr_epoch(gpu):
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(4000, 16000, 100_000, seed=11)
    rng = np.random.default_rng(1)
    X0, Y0 = _factors(m.shape[0], 65, rng, bias=1.0), _factors(m.shape[1], 65, rng)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    knn, Q = gpu.KnnQuery(), gpu.Matrix(X0[:64])
    before = knn.topk(Y, Q, 10)[0]
    uid, iid, ptr = _device_ids(gpu, m)
    for seed in range(3):
        gpu.bpr_epoch(uid, iid, ptr, X, Y, 1.0, 0.0, seed, False)
    after = knn.topk(Y, Q, 10)[0]
    want = _knn_ids(gpu, Y.to_numpy(), X0[:64], 10)
    assert (after == want).mean() > 0.99 and (before != want).mean() > 0.2


def test_save_load_and_pickle(gpu, tmp_path):
    import implicit_amd.gpu.bpr as gbpr

    m = _small_matrix()
    model = _model()
    model.fit(m, show_progress=False)
    path = str(tmp_path / "bpr.npz")
    model.save(path)
    with np.load(path) as data:
        assert set(data.files) == {"user_factors", "item_factors", "regularization", "factors", "learning_rate",
                                   "verify_negative_samples", "iterations", "dtype", "random_state"}
    loaded = gbpr.BayesianPersonalizedRanking.load(path)
    assert_array_equal(loaded.item_factors.to_numpy(), model.item_factors.to_numpy())
    assert loaded.learning_rate == model.learning_rate and loaded.factors == 16
    buf = io.BytesIO()
    pickle.dump(model, buf)
    again = pickle.loads(buf.getvalue())
    assert_array_equal(again.user_factors.to_numpy(), model.user_factors.to_numpy())
    ids, _ = again.recommend(0, m[0], N=3)
    assert_array_equal(ids, model.recommend(0, m[0], N=3)[0])


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    m = _small_matrix()
    uid, iid, ptr = _device_ids(gpu, m)
    rng = np.random.default_rng(3)
    X0, Y0 = _factors(m.shape[0], 17, rng, bias=1.0), _factors(m.shape[1], 17, rng)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    with pytest.raises(ValueError):
        gpu.bpr_epoch(uid, iid, ptr, X, gpu.Matrix(_factors(m.shape[1], 18, rng)), LR, REG, 1, True)
    with pytest.raises(ValueError):
        gpu.bpr_epoch(uid, iid, ptr, gpu.Matrix(_factors(m.shape[0], 1025, rng)), gpu.Matrix(_factors(m.shape[1], 1025, rng)),
                      LR, REG, 1, True)
    with pytest.raises(ValueError):
        gpu.bpr_epoch(uid, iid, ptr, X.astype(np.float16), Y.astype(np.float16), LR, REG, 1, True)
    with pytest.raises(ValueError):
        gpu.bpr_epoch(uid, iid, gpu.IntVector(np.asarray(m.indptr[:-1], dtype=np.int32)), X, Y, LR, REG, 1, True)
    with pytest.raises(ValueError):
        gpu.bpr_epoch(uid, gpu.IntVector(np.asarray(m.indices[:-1], dtype=np.int32)), ptr, X, Y, LR, REG, 1, True)
    bad = np.asarray(m.indices, dtype=np.int32).copy()
    bad[len(bad) // 2] = m.shape[1]  # one past the last item row
    with pytest.raises(IndexError):
        gpu.bpr_epoch(uid, gpu.IntVector(bad), ptr, X, Y, LR, REG, 1, False)
    bad_u = ref.coo_ids(m)[0].copy()
    bad_u[0] = -1
    with pytest.raises(IndexError):
        gpu.bpr_epoch(gpu.IntVector(bad_u), iid, ptr, X, Y, LR, REG, 1, False)
    # the pre-pass reads the ids four at a time and the rest one by one: a bad id in the last position of every tail length,
    # and row pointers outside [0, nnz]
    users_all, items_all = ref.coo_ids(m)
    for tail in (1, 2, 3):
        nnz = (m.nnz - 4) // 4 * 4 + tail
        mt = csr_matrix((m.data[:nnz], m.indices[:nnz], np.minimum(m.indptr, nnz)), shape=m.shape)
        assert mt.nnz == nnz and nnz % 4 == tail
        uid_t, iid_t, ptr_t = _device_ids(gpu, mt)
        for bad_value in (m.shape[1], -1):
            bad = items_all[:nnz].copy()
            bad[-1] = bad_value
            with pytest.raises(IndexError):
                gpu.bpr_epoch(uid_t, gpu.IntVector(bad), ptr_t, X, Y, LR, REG, 1, False)
        for bad_value in (m.shape[0], -1):
            bad_u = users_all[:nnz].copy()
            bad_u[-1] = bad_value
            with pytest.raises(IndexError):
                gpu.bpr_epoch(gpu.IntVector(bad_u), iid_t, ptr_t, X, Y, LR, REG, 1, False)
        for at, bad_value in ((0, -1), (len(mt.indptr) // 2, -1), (len(mt.indptr) - 1, nnz + 1), (5, nnz + 1)):
            bad_ptr = np.asarray(mt.indptr, dtype=np.int32).copy()
            bad_ptr[at] = bad_value
            with pytest.raises(IndexError):
                gpu.bpr_epoch(uid_t, iid_t, gpu.IntVector(bad_ptr), X, Y, LR, REG, 1, True)
        assert_array_equal(X.to_numpy().view(np.uint32), X0.view(np.uint32))
        assert_array_equal(Y.to_numpy().view(np.uint32), Y0.view(np.uint32))
        # a valid call still works
        assert gpu.bpr_epoch(uid_t, iid_t, ptr_t, X, Y, 0.0, 0.0, 1, True)[1] == ref.predicted_skipped(mt, 1, True) > 0
    assert_array_equal(X.to_numpy(), X0)
    assert_array_equal(Y.to_numpy(), Y0)
    assert gpu.bpr_epoch(gpu.IntVector(np.zeros(0, np.int32)), gpu.IntVector(np.zeros(0, np.int32)),
                         gpu.IntVector(np.zeros(m.shape[0] + 1, np.int32)), X, Y, LR, REG, 1, True) == (0, 0)
