"""WARP training on the device (imp_warp_update / warp_epoch, csrc/warp.hip) and the model built on it
(implicit_amd.gpu.warp), judged against the float64 restatement of the contract in warp_reference.py.  The matrices, the
row comparison and the planted problem are those of the BPR tests."""
import io
import pickle

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import csr_matrix

import bpr_reference as bref
import sgd_cases as sc
import warp_reference as ref
from test_gpu_bpr import _check_against, _check_call, _device_ids, _factors, _held_out_auc, _knn_ids, _planted, _rel, _small_matrix

pytestmark = pytest.mark.gpu

LR, REG = 0.05, 0.01
MARGIN = 1e-4  # seeds are chosen so that no examined trial is closer to the violation threshold: fp32 and float64 then agree


# ---- 1. single samples are exact ----------------------------------------------------------------------------------------
def _single_steps_exact(gpu, C):
    """25 chained single-sample calls, max_sampled 6 (the second Philox block is used).  The seeds are picked on the host, from
    2000 at most, for a closest margin >= 1e-4 on the factors the chain has reached; at least 3 have a liked first candidate
    and at least 3 a first violation at t >= 2."""
    m = _small_matrix()
    rows, items, max_sampled = ref.liked_sets(m), m.shape[1], 6
    rng = np.random.default_rng(C)
    X0, Y0 = _factors(m.shape[0], C, rng, bias=1.0), _factors(m.shape[1], C, rng)
    X0[3] = 0.0
    X0[3, -1] = 1.0
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    Xc, Yc = X0.copy(), Y0.copy()
    done = liked_first = late = tried = 0
    for s in (int(v) for v in rng.integers(0, 2**62, 2000)):
        if done == 25:
            break
        tried += 1
        (u,), (i,) = (v.tolist() for v in ref.positives(m, s, 1))
        cand = ref.candidates(s, 0, items, max_sampled)
        X64, Y64 = Xc.astype(np.float64), Yc.astype(np.float64)
        t, trials, closest = ref.step64(X64, Y64, rows[u], u, i, cand, LR, REG)
        if closest < MARGIN:
            continue
        is_liked_first, is_late = int(cand[0]) in rows[u], t is not None and t >= 2
        owed = max(0, 3 - liked_first) + max(0, 3 - late)
        if 25 - done <= owed and not (is_liked_first and liked_first < 3) and not (is_late and late < 3):
            continue  # the remaining calls are kept for the two kinds still missing
        got = gpu.warp_epoch(uid, iid, ptr, X, Y, LR, REG, s, max_sampled, samples=1)
        assert got == (int(t is None), trials), (s, got, t, trials)
        Xg, Yg = X.to_numpy(), Y.to_numpy()
        _check_against(Xg, Yg, X64, Y64, Xc, Yc, set() if t is None else {u}, set() if t is None else {i, int(cand[t - 1])})
        Xc, Yc = Xg, Yg
        done, liked_first, late = done + 1, liked_first + is_liked_first, late + is_late
    assert done == 25, (done, tried)
    assert liked_first >= 3 and late >= 3, (liked_first, late)


@pytest.mark.parametrize("C", sc.DISPATCH_C)  # both ends of every (lanes, columns per lane) instantiation
def test_single_steps_exact(gpu, C):
    _single_steps_exact(gpu, C)


@pytest.mark.parametrize("lanes, C", [(lanes, C) for lanes, C, _ in sc.LANE_OVERRIDES])
def test_lane_override_routes(gpu, monkeypatch, lanes, C):
    """IMP_BPR_LANES is read by every call (bpr_group): other group widths than the dispatch picks reach the twelve
    instantiations nothing else does (sgd_cases.LANE_OVERRIDES).  16 lanes at C = 257 cannot hold a row in 16 registers a
    lane: there the switch is ignored."""
    monkeypatch.setenv("IMP_BPR_LANES", str(lanes))
    _single_steps_exact(gpu, C)


@pytest.mark.parametrize("C", sc.DISPATCH_C)
def test_satisfied_sample_writes_nothing(gpu, C):
    """|dot| < 1 without the bias; the bias is -4 on every item outside the user's row and 0 inside it: no candidate violates."""
    m = _small_matrix()
    rng = np.random.default_rng(1000 + C)
    X0, Y0 = _factors(m.shape[0], C, rng), _factors(m.shape[1], C, rng)
    X0 *= 0.05
    Y0 *= 0.05
    X0[:, -1] = 1.0
    seed = 4242 + C
    (u,), _ = (v.tolist() for v in ref.positives(m, seed, 1))
    Y0[:, -1] = -4.0
    Y0[m.indices[m.indptr[u]:m.indptr[u + 1]], -1] = 0.0
    assert np.abs(X0[:, :-1].astype(np.float64) @ Y0[:, :-1].astype(np.float64).T).max() < 1.0
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    for max_sampled in (1, 4, 5):
        assert gpu.warp_epoch(uid, iid, ptr, X, Y, LR, REG, seed, max_sampled, samples=1) == (1, max_sampled)
        assert_array_equal(X.to_numpy(), X0)
        assert_array_equal(Y.to_numpy(), Y0)


# ---- 2. a multi-sample call without conflicts is exact --------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse_matrix():
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(4000, 20000, 60_000, gamma=1.0, seed=3)
    return m, ref.liked_sets(m)


@pytest.mark.parametrize("C", [17, 101, 257, 1024])
def test_conflict_free_call_exact(gpu, C, sparse_matrix):
    m, rows = sparse_matrix
    n, max_sampled, items = 64, 4, m.shape[1]
    rng = np.random.default_rng(C)
    X0, Y0 = _factors(m.shape[0], C, rng, bias=1.0), _factors(m.shape[1], C, rng)
    X64, Y64 = X0.astype(np.float64), Y0.astype(np.float64)
    for seed in range(1, 5000):
        us, iis = (v.tolist() for v in ref.positives(m, seed, n))
        if len(set(us)) < n or len(set(iis)) < n:
            continue
        satisfied = trials = 0
        touched, closest = list(iis), np.inf
        for s, (u, i) in enumerate(zip(us, iis)):
            cand = ref.candidates(seed, s, items, max_sampled)
            t, used, margin = ref.step64(X64, Y64, rows[u], u, i, cand, LR, REG)
            satisfied, trials, closest = satisfied + (t is None), trials + used, min(closest, margin)
            touched += [j for j in cand[:used].tolist() if j not in rows[u]]  # the candidates it examined
        if len(set(touched)) == len(touched) and closest >= MARGIN:
            break
        X64[us], Y64[touched] = X0[us], Y0[touched]  # as before this seed
    else:
        pytest.fail("no conflict-free seed found")
    assert satisfied < n  # the call does update
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    assert gpu.warp_epoch(uid, iid, ptr, X, Y, LR, REG, seed, max_sampled, samples=n) == (satisfied, trials)
    Xg, Yg = X.to_numpy(), Y.to_numpy()
    for u in us:
        assert _rel(Xg[u], X64[u]) < 2e-6, ("user", u)
    for j in touched:
        assert _rel(Yg[j], Y64[j]) < 2e-6, ("item", j)
    untouched_u = np.array(sorted(set(range(m.shape[0])) - set(us)))
    untouched_i = np.array(sorted(set(range(m.shape[1])) - set(touched)))
    assert_array_equal(Xg[untouched_u], X0[untouched_u])
    assert_array_equal(Yg[untouched_i], Y0[untouched_i])
    assert (Xg[:, -1] == 1.0).all()


@pytest.fixture(scope="module")
def rounds_matrix():
    m = sc.rounds_matrix()
    return m, ref.liked_sets(m)


@pytest.mark.parametrize("C", sc.ROUNDS_C)
def test_conflict_free_call_exact_over_rounds(gpu, C, rounds_matrix):
    """24 samples on a 256-user matrix: 16 samples in flight, so half of the groups start a second sample, in the pass where
    their neighbours run their next trial or have left the loop (sgd_cases.py, section 2).  The margin filter and the seed
    search are those of test_conflict_free_call_exact."""
    m, rows = rounds_matrix
    n = sc.ROUNDS_N
    case = sc.warp_rounds_case(m, rows, C)
    assert case is not None, "no conflict-free seed found"
    us, touched, X0, Y0, X64, Y64 = (case[k] for k in ("us", "touched", "X0", "Y0", "X64", "Y64"))
    assert case["satisfied"] < n  # the call does update
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    got = gpu.warp_epoch(uid, iid, ptr, X, Y, LR, REG, case["seed"], sc.ROUNDS_MAX_SAMPLED, samples=n)
    assert got == (case["satisfied"], case["trials"])
    Xg, Yg = X.to_numpy(), Y.to_numpy()
    # a satisfied sample's user and positive are listed as touched and unchanged in float64: 0 relative difference
    _check_call(Xg, Yg, X64, Y64, X0, Y0, set(us), set(touched))


# ---- 3. a whole epoch -----------------------------------------------------------------------------------------------------
def test_whole_epoch(gpu):
    from implicit_amd.synthetic import named

    m = named("ml100k", empty_frac=0.02)
    C, max_sampled = 65, 10
    X0, Y0, _ = bref.init_factors(m, C - 1, 7)
    uid, iid, ptr = _device_ids(gpu, m)
    empty_users = np.diff(m.indptr) == 0
    assert empty_users.any()
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    satisfied, trials = gpu.warp_epoch(uid, iid, ptr, X, Y, 0.02, 0.01, 1234, max_sampled)
    samples = m.nnz
    # satisfied + updated = samples.  The call does not return the updated count, so this is checked through a proxy, the
    # trial accounting that the identity implies: a satisfied sample consumed max_sampled draws, an updated one 1 .. max_sampled
    assert 0 <= satisfied < samples
    assert samples <= max_sampled * satisfied + (samples - satisfied) <= trials <= max_sampled * samples
    Xg, Yg = X.to_numpy(), Y.to_numpy()
    assert np.isfinite(Xg).all() and np.isfinite(Yg).all()
    assert_array_equal(Xg[empty_users], X0[empty_users])
    assert (Xg[:, -1] == 1.0).all()
    assert not np.array_equal(Yg, Y0)  # never-liked items may change too: they are valid negatives here


@pytest.mark.parametrize("C", sc.SEARCH_C)
def test_zero_learning_rate_epoch_is_exact(gpu, C):
    """lr = reg = 0: every store writes back what its lane loaded, so an epoch -- some 22 000 chained samples, 16 in flight,
    63 000 trials -- returns the counts of the serial restatement on the initial factors, and X and Y bit for bit.  The matrix
    has rows on both sides of every cut of the membership search, six items in seven carry a bias of -4 so that satisfied,
    first-trial and late samples all occur, and no margin of the epoch is below 1e-4 (sgd_cases.py, section 3;
    tests/test_sgd_cases_host.py shows which hits and misses the epoch meets)."""
    m = sc.search_matrix()
    X0, Y0 = sc.warp_frozen_factors(m, C)
    _, _, (want,), closest = ref.serial_epochs(m, X0, Y0, [sc.SEARCH_EPOCH_SEED], 0.0, 0.0, sc.SEARCH_MAX_SAMPLED, with_margin=True)
    assert closest >= MARGIN and 0 < want[0] < m.nnz
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    for _ in range(2):
        got = gpu.warp_epoch(uid, iid, ptr, X, Y, 0.0, 0.0, sc.SEARCH_EPOCH_SEED, sc.SEARCH_MAX_SAMPLED)
        print(f"C={C}: (satisfied, trials) {got}, serial {want}, closest margin {closest:.3g}")
        assert got == want
        assert_array_equal(X.to_numpy().view(np.uint32), X0.view(np.uint32))
        assert_array_equal(Y.to_numpy().view(np.uint32), Y0.view(np.uint32))


# ---- 4. learning quality --------------------------------------------------------------------------------------------------
def test_learning_quality_against_serial(gpu):
    """The GPU model's held-out AUC against the serial float64 SGD over the same draws (the same initial factors and epoch
    seeds; the Hogwild interleaving differs, and with it which candidates a sample examines).  Planted problem, seeds 0 / 1
    / 2, factors 8, lr 0.02, reg 0.01, max_sampled 10, 8 epochs.  Calibrated on the MI355X with BPR's cap on the samples in
    flight, on the kernel with write-through stores: the first measurement gave GPU - serial = -0.0021 / +0.0004 / -0.0146
    (serial AUC 0.957 / 0.947 / 0.951); the margin, 0.0296, is the worst of the three plus 0.015 of slack for the
    run-to-run variation of Hogwild.  Fifteen later differences (five runs) lay between -0.0046 and +0.0039 (DESIGN.md
    4.15)."""
    import implicit_amd.gpu.warp as gwarp

    worst = 1.0
    for seed in range(3):
        train, held = _planted(seed)
        seen = []
        model = gwarp.WARPMatrixFactorization(factors=8, learning_rate=0.02, regularization=0.01, iterations=8, max_sampled=10,
                                              random_state=seed)
        model.fit(train, show_progress=False, callback=lambda e, t, sat, tr: seen.append((sat, tr)))
        auc_gpu = _held_out_auc(model.user_factors.to_numpy(), model.item_factors.to_numpy(), train, held)
        X0, Y0, rs = bref.init_factors(train, 8, seed)
        seeds = [rs.integers(2**31) for _ in range(8)]
        X, Y, counts = ref.serial_epochs(train, X0, Y0, seeds, 0.02, 0.01, 10)
        auc_ser = _held_out_auc(X, Y, train, held)
        share = [sat / train.nnz for sat, _ in counts]
        print(f"seed {seed}: held-out AUC gpu {auc_gpu:.4f} serial {auc_ser:.4f} (diff {auc_gpu - auc_ser:+.4f}); satisfied share "
              f"serial {share[0]:.3f} -> {share[-1]:.3f}, gpu {seen[0][0] / train.nnz:.3f} -> {seen[-1][0] / train.nnz:.3f}")
        worst = min(worst, auc_gpu - auc_ser)
        assert auc_ser > 0.9
        assert share[0] < 0.1 and share[-1] > 0.5, share
    assert worst > -0.0296


# ---- 5. the model -----------------------------------------------------------------------------------------------------------
def _model(**kw):
    import implicit_amd.warp

    args = dict(factors=16, learning_rate=0.05, regularization=0.01, iterations=3, max_sampled=10, random_state=42)
    args.update(kw)
    return implicit_amd.warp.WARPMatrixFactorization(**args)


def test_initial_factors_match_bpr_formula(gpu):
    m = _small_matrix(users=60, items=50, seed=2)
    model = _model(iterations=0)
    model.fit(m, show_progress=False)
    X0, Y0, _ = bref.init_factors(m, 16, 42)
    assert_array_equal(model.user_factors.to_numpy(), X0)
    assert_array_equal(model.item_factors.to_numpy(), Y0)


def test_callback_and_degenerate_matrices(gpu):
    calls = []
    m = _small_matrix()
    model = _model(iterations=5)
    model.fit(m, show_progress=False, callback=lambda *a: calls.append(a))
    assert len(calls) == 5 and [a[0] for a in calls] == list(range(5))
    for _, _, satisfied, trials in calls:
        assert 0 <= satisfied <= m.nnz and m.nnz <= trials <= 10 * m.nnz
    _model().fit(csr_matrix(np.zeros((3, 3), dtype=np.float32)), show_progress=False)  # nothing to sample: no launch
    one_user = _model()
    one_user.fit(csr_matrix(np.array([[0, 1, 0, 1, 0, 0, 0, 1]], dtype=np.float32)), show_progress=False)
    assert np.isfinite(one_user.item_factors.to_numpy()).all() and one_user.user_factors.shape == (1, 17)
    model.fit(m.astype(np.float64), show_progress=False)  # non-fp32 input, existing factors kept
    # users who like every item: every trial is consumed, every sample is satisfied, nothing is written
    full, calls = csr_matrix(np.ones((5, 40), dtype=np.float32)), []
    everything = _model(iterations=2, max_sampled=7)
    everything.fit(full, show_progress=False, callback=lambda *a: calls.append(a[2:]))
    assert calls == [(full.nnz, 7 * full.nnz)] * 2
    X0, Y0, _ = bref.init_factors(full, 16, 42)
    assert_array_equal(everything.user_factors.to_numpy(), X0)
    assert_array_equal(everything.item_factors.to_numpy(), Y0)


def test_unsorted_input_gives_sorted_counts(gpu):
    """With a zero learning rate the factors stand still, so every sample of an epoch is a single-sample call on the initial
    factors and the counts of the epoch are the restatement's, whatever the interleaving: they depend on the liked search
    alone, which needs sorted rows."""
    m = _small_matrix(users=80, items=40, seed=5)
    rev = m.copy()
    for r in range(rev.shape[0]):  # reverse every row's column order
        a, b = rev.indptr[r], rev.indptr[r + 1]
        rev.indices[a:b] = rev.indices[a:b][::-1].copy()
        rev.data[a:b] = rev.data[a:b][::-1].copy()
    rev.has_sorted_indices = False
    rev_indices = rev.indices.copy()
    counts = {}
    for key, mat in (("sorted", m), ("unsorted", rev)):
        seen = []
        _model(iterations=3, learning_rate=0.0, regularization=0.0).fit(mat, show_progress=False,
                                                                        callback=lambda e, t, sat, tr: seen.append((sat, tr)))
        counts[key] = seen
    X0, Y0, rs = bref.init_factors(m, 16, 42)
    want = ref.serial_epochs(m, X0, Y0, [rs.integers(2**31) for _ in range(3)], 0.0, 0.0, 10)[2]
    assert counts["sorted"] == want and counts["unsorted"] == want
    assert sum(tr for _, tr in want) > 3 * m.nnz  # liked candidates were drawn and consumed
    assert_array_equal(rev.indices, rev_indices)  # the caller's matrix is left alone


def test_recommend_and_similar_items_follow_factors(gpu):
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(2000, 16000, 60_000, seed=9)
    model = _model(factors=64, iterations=2)
    users = np.arange(256)
    model.fit(m, show_progress=False)
    X, Y = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    assert np.isfinite(X).all() and np.isfinite(Y).all()
    ids, _ = model.recommend(users, m[users], N=10, filter_already_liked_items=False)
    assert (ids == _knn_ids(gpu, Y, X[users], 10)).mean() > 0.99
    sim, _ = model.similar_items(np.arange(32), N=5)
    norms = np.linalg.norm(Y.astype(np.float64), axis=1)
    cos = (Y[:32].astype(np.float64) @ Y.astype(np.float64).T) / np.maximum(norms, 1e-10)[None, :]
    assert (sim == np.argsort(-cos, axis=1, kind="stable")[:, :5]).mean() > 0.95


def test_ranking_metrics_run_on_the_model(gpu):
    import implicit_amd.evaluation as ev

    train, held = _planted(0)
    test = csr_matrix((np.ones(300, dtype=np.float32), (np.arange(300), held)), shape=train.shape)
    model = _model(factors=8, learning_rate=0.02, iterations=4)
    model.fit(train, show_progress=False)
    got = ev.ranking_metrics_at_k(model, train, test, K=10, show_progress=False)
    assert set(got) == {"precision", "map", "ndcg", "auc"}
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in got.values()), got


def test_save_load_and_pickle(gpu, tmp_path):
    import implicit_amd.gpu.warp as gwarp

    m = _small_matrix()
    model = _model(max_sampled=7)
    model.fit(m, show_progress=False)
    path = str(tmp_path / "warp.npz")
    model.save(path)
    with np.load(path) as data:
        assert set(data.files) == {"user_factors", "item_factors", "regularization", "factors", "learning_rate", "max_sampled",
                                   "iterations", "dtype", "random_state"}
    loaded = gwarp.WARPMatrixFactorization.load(path)
    assert_array_equal(loaded.item_factors.to_numpy(), model.item_factors.to_numpy())
    assert_array_equal(loaded.user_factors.to_numpy(), model.user_factors.to_numpy())
    assert loaded.learning_rate == model.learning_rate and loaded.factors == 16 and loaded.max_sampled == 7
    buf = io.BytesIO()
    pickle.dump(model, buf)
    again = pickle.loads(buf.getvalue())
    assert again.max_sampled == 7
    assert_array_equal(again.user_factors.to_numpy(), model.user_factors.to_numpy())
    ids, _ = again.recommend(0, m[0], N=3)
    assert_array_equal(ids, model.recommend(0, m[0], N=3)[0])


def test_argument_errors(gpu):
    m = _small_matrix()
    uid, iid, ptr = _device_ids(gpu, m)
    rng = np.random.default_rng(3)
    X0, Y0 = _factors(m.shape[0], 17, rng, bias=1.0), _factors(m.shape[1], 17, rng)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    for max_sampled in (0, 5000):
        with pytest.raises(ValueError):
            gpu.warp_epoch(uid, iid, ptr, X, Y, LR, REG, 1, max_sampled)
        with pytest.raises(ValueError):
            _model(max_sampled=max_sampled)
    with pytest.raises(ValueError):
        gpu.warp_epoch(uid, iid, ptr, X, gpu.Matrix(_factors(m.shape[1], 18, rng)), LR, REG, 1)
    with pytest.raises(ValueError):
        gpu.warp_epoch(uid, iid, ptr, gpu.Matrix(_factors(m.shape[0], 1025, rng)), gpu.Matrix(_factors(m.shape[1], 1025, rng)),
                       LR, REG, 1)
    with pytest.raises(ValueError):
        gpu.warp_epoch(uid, iid, ptr, X.astype(np.float16), Y.astype(np.float16), LR, REG, 1)
    with pytest.raises(ValueError):
        gpu.warp_epoch(uid, iid, gpu.IntVector(np.asarray(m.indptr[:-1], dtype=np.int32)), X, Y, LR, REG, 1)
    with pytest.raises(ValueError):
        gpu.warp_epoch(uid, gpu.IntVector(np.asarray(m.indices[:-1], dtype=np.int32)), ptr, X, Y, LR, REG, 1)
    bad = np.asarray(m.indices, dtype=np.int32).copy()
    bad[len(bad) // 2] = m.shape[1]  # one past the last item row
    with pytest.raises(IndexError):
        gpu.warp_epoch(uid, gpu.IntVector(bad), ptr, X, Y, LR, REG, 1)
    bad_u = bref.coo_ids(m)[0].copy()
    bad_u[0] = -1
    with pytest.raises(IndexError):
        gpu.warp_epoch(gpu.IntVector(bad_u), iid, ptr, X, Y, LR, REG, 1)
    # the pre-pass reads the ids four at a time and the rest one by one: a bad id in the last position of every tail length,
    # and row pointers outside [0, nnz]
    users_all, items_all = bref.coo_ids(m)
    for tail in (1, 2, 3):
        nnz = (m.nnz - 4) // 4 * 4 + tail
        mt = csr_matrix((m.data[:nnz], m.indices[:nnz], np.minimum(m.indptr, nnz)), shape=m.shape)
        assert mt.nnz == nnz and nnz % 4 == tail
        uid_t, iid_t, ptr_t = _device_ids(gpu, mt)
        for bad_value in (m.shape[1], -1):
            bad = items_all[:nnz].copy()
            bad[-1] = bad_value
            with pytest.raises(IndexError):
                gpu.warp_epoch(uid_t, gpu.IntVector(bad), ptr_t, X, Y, LR, REG, 1)
        for bad_value in (m.shape[0], -1):
            bad_u = users_all[:nnz].copy()
            bad_u[-1] = bad_value
            with pytest.raises(IndexError):
                gpu.warp_epoch(gpu.IntVector(bad_u), iid_t, ptr_t, X, Y, LR, REG, 1)
        for at, bad_value in ((0, -1), (len(mt.indptr) // 2, -1), (len(mt.indptr) - 1, nnz + 1), (5, nnz + 1)):
            bad_ptr = np.asarray(mt.indptr, dtype=np.int32).copy()
            bad_ptr[at] = bad_value
            with pytest.raises(IndexError):
                gpu.warp_epoch(uid_t, iid_t, gpu.IntVector(bad_ptr), X, Y, LR, REG, 1)
        assert_array_equal(X.to_numpy().view(np.uint32), X0.view(np.uint32))
        assert_array_equal(Y.to_numpy().view(np.uint32), Y0.view(np.uint32))
        # a valid call still works: at a zero learning rate its counts are the serial restatement's
        _, _, (want,), closest = ref.serial_epochs(mt, X0, Y0, [1], 0.0, 0.0, 3, with_margin=True)
        assert closest >= MARGIN
        assert gpu.warp_epoch(uid_t, iid_t, ptr_t, X, Y, 0.0, 0.0, 1, 3) == want
    assert_array_equal(X.to_numpy(), X0)
    assert_array_equal(Y.to_numpy(), Y0)
    assert gpu.warp_epoch(gpu.IntVector(np.zeros(0, np.int32)), gpu.IntVector(np.zeros(0, np.int32)),
                          gpu.IntVector(np.zeros(m.shape[0] + 1, np.int32)), X, Y, LR, REG, 1) == (0, 0)


# ---- 6. what later kernels read, and cache invalidation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [65, 101])
def test_later_kernels_read_the_rows_a_host_copy_holds(gpu, C):
    """Once the call has returned there is one X and one Y: a kernel launched afterwards (calculate_norms) reads, for every row,
    what a device-to-host copy holds.  250 samples in flight here: several workgroups, on several XCDs.  With plain stores
    in the update about 900 of the 16000 item rows were read in an older version (the lines stayed in the L2 of the XCD that
    wrote them) in every round but a process's first: hence three rounds."""
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(4000, 16000, 100_000, seed=11)
    uid, iid, ptr = _device_ids(gpu, m)
    for rnd in range(3):
        rng = np.random.default_rng(rnd)
        X, Y = gpu.Matrix(_factors(m.shape[0], C, rng, bias=1.0)), gpu.Matrix(_factors(m.shape[1], C, rng))
        for seed in range(3):
            gpu.warp_epoch(uid, iid, ptr, X, Y, 0.02, 0.0, seed)
        for M in (Y, X):
            seen = gpu.calculate_norms(M).to_numpy().ravel().astype(np.float64)  # the kernel reads first, then the copy
            want = np.linalg.norm(M.to_numpy().astype(np.float64), axis=1)
            # 1e-5 relative: well above the rounding of an fp32 norm of C terms (about 1e-7 C^0.5), well below what one SGD step
            # of lr 0.02 changes in a row's norm
            assert np.flatnonzero(np.abs(seen - want) > 1e-5 * np.maximum(want, 1e-30)).size == 0, (rnd, M is Y)


def test_plane_cache_invalidated_by_warp_epoch(gpu):
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(4000, 16000, 100_000, seed=11)
    rng = np.random.default_rng(1)
    X0, Y0 = _factors(m.shape[0], 65, rng, bias=1.0), _factors(m.shape[1], 65, rng)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    knn, Q = gpu.KnnQuery(), gpu.Matrix(X0[:64])
    before = knn.topk(Y, Q, 10)[0]
    uid, iid, ptr = _device_ids(gpu, m)
    for seed in range(3):
        gpu.warp_epoch(uid, iid, ptr, X, Y, 0.1, 0.0, seed)
    after = knn.topk(Y, Q, 10)[0]
    Yg = Y.to_numpy()
    assert np.isfinite(Yg).all()
    want = _knn_ids(gpu, Yg, X0[:64], 10)
    assert (after == want).mean() > 0.99 and (before != want).mean() > 0.2
