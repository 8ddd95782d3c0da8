"""Sampled-softmax training on the device (softmax_epoch, csrc/softmax_mf.hip) and its model, against the float64 restatement
softmax_reference.py.  The exactness tests run on matrices with fewer than 2048 rows on one side: one workgroup in flight, a
call is the serial mini-batch SGD.  Their tolerance is 4 x the relative Frobenius distance between the float64 and the float32
run of the restatement on the test's own input (the matrix instruction and the atomic adds sum in another order than numpy)."""
import io
import pickle

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import csr_matrix

import bpr_reference as bref
import softmax_reference as ref
from test_gpu_bpr import _device_ids, _factors, _held_out_auc, _knn_ids, _rel, _small_matrix

pytestmark = pytest.mark.gpu

LR, REG, CAP = 0.05, 0.01, 1024  # CAP: the widest C the entry point accepts
MARGIN = 1e-4  # no row of the float64 run has its positive closer to its best unmasked negative: the counts are decided


def _exact(gpu, m, X0, Y0, calls, N):
    # `calls` = [(seed, samples), ...] chained on the device and in the restatement (float64 and float32)
    uid, iid, ptr = _device_ids(gpu, m)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    X64, Y64, X32, Y32 = X0, Y0, X0, Y0
    for seed, samples in calls:
        X64, Y64, correct, masked, closest = ref.serial(m, X64, Y64, seed, LR, REG, N, samples)
        X32, Y32 = ref.serial(m, X32, Y32, seed, LR, REG, N, samples, dtype=np.float32)[:2]
        assert closest >= MARGIN
        assert gpu.softmax_epoch(uid, iid, ptr, X, Y, LR, REG, seed, N, samples=samples) == (correct, masked)
    Xg, Yg = X.to_numpy(), Y.to_numpy()
    tol_x, tol_y = 4 * _rel(X32, X64), 4 * _rel(Y32, Y64)
    print(f"fp32 restatement from float64: X {tol_x / 4:.3g} Y {tol_y / 4:.3g}; device: X {_rel(Xg, X64):.3g} Y {_rel(Yg, Y64):.3g}")
    assert _rel(Xg, X64) <= tol_x and _rel(Yg, Y64) <= tol_y
    assert (Xg[:, -1] == 1.0).all()
    return Xg


def _start(m, C, seed):
    rng = np.random.default_rng(seed)
    return _factors(m.shape[0], C, rng, bias=1.0), _factors(m.shape[1], C, rng)


# every C at one (samples, N), and every (samples, N) at C = 65
ONE_BATCH = [(C, 64, 128) for C in (2, 3, 5, 33, 65, 101, 129, 257, CAP)] + \
            [(65, samples, N) for samples in (1, 63, 64) for N in (32, 128, 256) if (samples, N) != (64, 128)]


@pytest.mark.parametrize("C, samples, N", ONE_BATCH)
def test_one_batch_exact(gpu, C, samples, N):
    """Distances of the float32 restatement from float64 on these inputs: X 3.3e-9 (one sample) .. 5.0e-8 (C = 1024), Y 1.2e-8
    .. 5.7e-8; the tolerances are 4 x these.  Measured on the MI355X, the device lay at X 3.3e-9 .. 8.3e-8 and Y 1.2e-8 ..
    5.7e-8 from float64, at most 1.7 x the restatement's own distance (C = 1024).  The users no sample drew stay bit for bit."""
    m = _small_matrix()
    X0, Y0 = _start(m, C, C)
    Xg = _exact(gpu, m, X0, Y0, [(100 + C, samples)], N)
    untouched = np.setdiff1d(np.arange(m.shape[0]), ref.positives(m, 100 + C, samples)[0])
    assert_array_equal(Xg[untouched].view(np.uint32), X0[untouched].view(np.uint32))


def test_duplicates_and_masks_exact(gpu):
    """3 users x 40 items, 64 samples against 32 negatives: user 0 likes everything (every negative masked: p_r = 1, only the
    reg terms move its rows), user 1 a single item, user 2 eight.  Users and positives repeat within the batch, negatives
    repeat, and negatives are other rows' positives.  fp32 restatement from float64: X 3.65e-7, Y 6.3e-8 (device the same)."""
    dense = np.zeros((3, 40), dtype=np.float32)
    dense[0], dense[1, 7], dense[2, ::5] = 1.0, 1.0, 1.0
    m, seed = csr_matrix(dense), 3
    us, iis = (set(v.tolist()) for v in ref.positives(m, seed, 64))
    js = set(ref.negatives(seed, 0, 40, 32).tolist())
    assert us == {0, 1, 2} and len(iis) < 40 and len(js) < 32 and js & iis
    _exact(gpu, m, *_start(m, 17, 5), [(seed, 64)], 32)


def test_chained_batches_exact(gpu):
    """Six batches (the last of 7 rows) in one workgroup, two calls: a batch reads what the one before it added and nothing
    of its own adds.  fp32 restatement from float64: X 9.9e-8, Y 1.24e-7 (device 9.8e-8, 1.24e-7)."""
    m = _small_matrix()
    _exact(gpu, m, *_start(m, 65, 11), [(21, 64 * 5 + 7), (22, 64 * 5 + 7)], 128)


def test_zero_rates_count_and_leave_the_factors(gpu):
    m = _small_matrix()
    X0, Y0 = _start(m, 33, 4)
    _, _, correct, masked, closest = ref.serial(m, X0, Y0, 9, 0.0, 0.0, 64)
    assert closest >= MARGIN and 0 < correct < m.nnz and masked > 0
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    assert gpu.softmax_epoch(*_device_ids(gpu, m), X, Y, 0.0, 0.0, 9, 64) == (correct, masked)
    assert_array_equal(X.to_numpy(), X0)  # every add is +-0
    assert_array_equal(Y.to_numpy(), Y0)


def _planted_large(seed):
    # test_gpu_bpr._planted enlarged to 4096 users x 2048 items: two workgroups in flight
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((4096, 8)), rng.standard_normal((2048, 8))
    top = np.argsort(-(U @ V.T + 0.5 * rng.standard_normal((4096, 2048))), axis=1)[:, :25]
    held = top[np.arange(4096), rng.integers(0, 25, 4096)]
    train = np.zeros((4096, 2048), dtype=np.float32)
    train[np.repeat(np.arange(4096), 25), top.ravel()] = 1.0
    train[np.arange(4096), held] = 0.0
    return csr_matrix(train), held


def test_learning_quality_against_serial(gpu):
    """Two workgroups in flight: the model's held-out AUC against the serial float64 mini-batch SGD over the same draws (only
    the interleaving of the batches differs).  Seeds 0 / 1 / 2, factors 8, lr 0.1, reg 0.01, N = 32, 4 epochs.  First run on
    the MI355X: GPU - serial = +0.0000 / -0.0000 / -0.0000 to the four digits printed then, +0.00003 / -0.00004 / -0.00007 in
    the next (serial AUC 0.9896 / 0.9887 / 0.9901).  The margin, 0.0151, is the worst of these plus 0.015."""
    import implicit_amd.gpu.softmax as gsoftmax

    worst = 1.0
    for seed in range(3):
        train, held = _planted_large(seed)
        model = gsoftmax.SampledSoftmaxMatrixFactorization(factors=8, learning_rate=0.1, regularization=0.01, iterations=4,
                                                           negatives=32, random_state=seed)
        model.fit(train, show_progress=False)
        auc_gpu = _held_out_auc(model.user_factors.to_numpy(), model.item_factors.to_numpy(), train, held)
        X, Y, rs = bref.init_factors(train, 8, seed)
        for _ in range(4):
            X, Y = ref.serial(train, X, Y, rs.integers(2**31), 0.1, 0.01, 32)[:2]
        auc_ser = _held_out_auc(X, Y, train, held)
        print(f"seed {seed}: held-out AUC gpu {auc_gpu:.5f} serial {auc_ser:.5f} (diff {auc_gpu - auc_ser:+.5f})")
        worst = min(worst, auc_gpu - auc_ser)
        assert auc_ser > 0.9
    assert worst > -0.0151


def test_later_kernels_and_cached_planes_see_the_epochs(gpu):
    """WARP's test_later_kernels_read_the_rows_a_host_copy_holds and test_plane_cache_invalidated_by_warp_epoch on their shape
    (three workgroups in flight): calculate_norms sees what a host copy holds, top-k the new rows, not the cached planes."""
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(4000, 16000, 100_000, seed=11)
    uid, iid, ptr = _device_ids(gpu, m)
    for rnd in range(3):
        X0, Y0 = _start(m, 65, rnd)
        X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
        knn, Q = gpu.KnnQuery(), gpu.Matrix(X0[:64])
        before = knn.topk(Y, Q, 10)[0]
        for seed in range(3):
            gpu.softmax_epoch(uid, iid, ptr, X, Y, 0.1, 0.0, seed)
        after = knn.topk(Y, Q, 10)[0]
        for M in (Y, X):
            seen = gpu.calculate_norms(M).to_numpy().ravel().astype(np.float64)  # the kernel reads first, then the copy
            want = np.linalg.norm(M.to_numpy().astype(np.float64), axis=1)
            assert np.flatnonzero(np.abs(seen - want) > 1e-5 * np.maximum(want, 1e-30)).size == 0, (rnd, M is Y)
        want = _knn_ids(gpu, Y.to_numpy(), X0[:64], 10)
        assert (after == want).mean() > 0.99 and (before != want).mean() > 0.2


# ---- the model --------------------------------------------------------------------------------------------------------------
def _model(**kw):
    import implicit_amd.softmax

    args = dict(factors=16, learning_rate=0.05, regularization=0.01, iterations=3, negatives=64, random_state=42)
    return implicit_amd.softmax.SampledSoftmaxMatrixFactorization(**{**args, **kw})


def test_argument_errors(gpu):
    m = _small_matrix()
    uid, iid, ptr = _device_ids(gpu, m)
    X0, Y0 = _start(m, 17, 3)
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    for negatives in (0, 48, 288):
        with pytest.raises(ValueError):
            gpu.softmax_epoch(uid, iid, ptr, X, Y, LR, REG, 1, negatives)
        with pytest.raises(ValueError):
            _model(negatives=negatives)
    rng = np.random.default_rng(0)
    for Xb, Yb in ((X, gpu.Matrix(_factors(m.shape[1], 18, rng))),
                   (gpu.Matrix(_factors(m.shape[0], CAP + 1, rng)), gpu.Matrix(_factors(m.shape[1], CAP + 1, rng))),
                   (X.astype(np.float16), Y.astype(np.float16))):
        with pytest.raises(ValueError):
            gpu.softmax_epoch(uid, iid, ptr, Xb, Yb, LR, REG, 1)
    bad = np.asarray(m.indices, dtype=np.int32).copy()
    bad[len(bad) // 2] = m.shape[1]  # one past the last item row
    with pytest.raises(IndexError):
        gpu.softmax_epoch(uid, gpu.IntVector(bad), ptr, X, Y, LR, REG, 1)
    assert_array_equal(X.to_numpy().view(np.uint32), X0.view(np.uint32))
    assert_array_equal(Y.to_numpy().view(np.uint32), Y0.view(np.uint32))


def test_model_recommends_and_round_trips(gpu, tmp_path):
    from implicit_amd.synthetic import synthetic_csr

    m, calls, users = synthetic_csr(2000, 16000, 60_000, seed=9), [], np.arange(256)
    model = _model(factors=64, iterations=2, negatives=96)
    model.fit(m, show_progress=False, callback=lambda *a: calls.append(a))
    assert [c[0] for c in calls] == [0, 1] and all(0 <= c[2] <= m.nnz and 0 <= c[3] <= 96 * m.nnz for c in calls)
    X, Y = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    assert np.isfinite(X).all() and np.isfinite(Y).all() and not np.array_equal(Y, bref.init_factors(m, 64, 42)[1])
    ids, _ = model.recommend(users, m[users], N=10, filter_already_liked_items=False)
    assert (ids == _knn_ids(gpu, Y, X[users], 10)).mean() > 0.99
    path, buf = str(tmp_path / "softmax.npz"), io.BytesIO()
    model.save(path)
    pickle.dump(model, buf)
    with np.load(path) as data:
        assert set(data.files) == {"user_factors", "item_factors", *model._npz_keys}
    for again in (type(model).load(path), pickle.loads(buf.getvalue())):
        assert again.factors == 64 and again.negatives == 96
        assert_array_equal(again.item_factors.to_numpy(), Y)
        assert_array_equal(again.user_factors.to_numpy(), X)
        assert_array_equal(again.recommend(users, m[users], N=10)[0], model.recommend(users, m[users], N=10)[0])
