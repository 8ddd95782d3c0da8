"""LMF training on the device (imp_lmf_update / lmf_update, csrc/lmf.hip) and the model built on it (implicit_amd.gpu.lmf),
judged against the reference's own lmf_update (tests/golden/lmf_golden.npz) and the float64 restatement of the contract in
lmf_reference.py."""
import io
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import coo_matrix, csr_matrix

import lmf_reference as ref
import sgd_cases as sc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "lmf_golden.npz")
SUITE = os.path.join(ROOT, "build", "refsuite")


def _golden_csr(g, name):
    return csr_matrix((g[name + "_data"], g[name + "_indices"], g[name + "_indptr"]), shape=tuple(g[name + "_shape"]))


def _class_matrix(users, seed=0):
    """A (users x items) matrix whose item side (the transpose) has a row in every length class of imp_csr: a column of
    0.85 x users entries (many 512-entry segments), rows of 1500 / 600 / 513 (long), 512, 300, 200, 100, 64, 40, 20, 16,
    5, 1 and 0 entries, and 40 short random ones.  Confidences other than 1.  The user side has short and empty rows."""
    rng = np.random.default_rng(seed)
    lens = [int(0.85 * users), 1500, 600, 513, 512, 300, 200, 100, 64, 40, 20, 16, 5, 1, 0] + rng.integers(0, 30, 40).tolist()
    lens = [min(n, users) for n in lens]
    rows = np.concatenate([rng.choice(users, n, replace=False) for n in lens])
    cols = np.repeat(np.arange(len(lens)), lens)
    m = coo_matrix((rng.uniform(0.5, 4.0, len(rows)).astype(np.float32), (rows, cols)), shape=(users, len(lens))).tocsr()
    m.sort_indices()
    return m


def _factors(rows, C, rng, scale=0.3):
    return (rng.standard_normal((rows, C)) * scale).astype(np.float32)


def _sweep(gpu, m, X0, Y0, G0, lr, reg, neg_prop, seed, one_col=-1):
    X, Y, G = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix(G0)
    gpu.lmf_update(gpu.CSRMatrix(m), X, Y, G, lr, reg, neg_prop, seed, one_col)
    return X.to_numpy(), G.to_numpy()


def _assert_within(got, want, bound, what, factor=2.0):
    ok, worst = ref.within(got, want, bound, factor)
    assert ok, f"{what}: worst |diff| / bound = {worst:.3g}"


# ---- 1. neg_prop = 0 against the reference's own output ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["np0_c5", "np0_c32", "np0_c66"])
def test_neg_prop_0_matches_reference(gpu, name):
    g = np.load(GOLDEN)
    m = _golden_csr(g, name)
    lr, reg = float(g[name + "_lr"]), float(g[name + "_reg"])
    X, Y = g[name + "_X0"], g[name + "_Y"]
    G = np.zeros_like(X)
    for step in (1, 2):  # each call from the reference's fp32 state before it
        Xg, Gg = _sweep(gpu, m, X, Y, G, lr, reg, 0, 1234)
        X64, G64, bX, bG = ref.half_sweep64(m, X, Y, G, lr, reg, 0, 0)
        _assert_within(Xg, X64, bX, f"X step {step} vs float64")
        _assert_within(Gg, G64, bG, f"G step {step} vs float64")
        _assert_within(Xg, g[f"{name}_X{step}"], bX, f"X step {step} vs reference", factor=4.0)
        _assert_within(Gg, g[f"{name}_G{step}"], bG, f"G step {step} vs reference", factor=4.0)
        X, G = g[f"{name}_X{step}"], g[f"{name}_G{step}"]


# ---- 2. neg_prop > 0 against the float64 restatement with the same draws ----------------------------------------------------
@pytest.mark.parametrize("C", sc.LMF_DISPATCH_C)  # both ends of every (lanes, columns per lane) instantiation of launch_lmf
def test_half_sweeps_match_float64(gpu, C):
    """The C the test ran at before keep the full class matrix; the ends of the dispatch ranges added to them run on the
    reduced one (sgd_cases.lmf_reduced_matrix), whose float64 restatement stays below 100 MB an array at every C."""
    if C in sc.LMF_EXISTING_C:
        m = _class_matrix(24000 if C <= 130 else 3000, seed=C)
    else:
        m = sc.lmf_reduced_matrix(C, seed=C)
    mt = m.T.tocsr()
    mt.sort_indices()
    lens = np.diff(mt.indptr)
    if C in sc.LMF_EXISTING_C:
        assert lens.max() > 2000 and (lens == 0).any() and ((lens > 16) & (lens <= 32)).any()
    else:
        G = sc.lmf_instantiation(C)[0]
        assert lens.max() > 512 and {512, G - 1, G, G + 1, 1, 0} <= set(lens.tolist())
    rng = np.random.default_rng(C)
    U, V = _factors(m.shape[0], C, rng), _factors(m.shape[1], C, rng)
    for name, csr, X0, Y0, neg_prop in (("items", mt, V, U, 30), ("users", m, U, V, 3)):
        G0 = rng.uniform(0.0, 2.0, X0.shape).astype(np.float32)
        seed = int(rng.integers(2**62))
        Xg, Gg = _sweep(gpu, csr, X0, Y0, G0, 0.7, 0.2, neg_prop, seed)
        X64, G64, bX, bG = ref.half_sweep64(csr, X0, Y0, G0, 0.7, 0.2, neg_prop, seed)
        _assert_within(Xg, X64, bX, f"{name} X")
        _assert_within(Gg, G64, bG, f"{name} G")
        empty = np.diff(csr.indptr) == 0
        assert empty.any()
        assert_array_equal(Xg[empty], X0[empty])
        assert_array_equal(Gg[empty], G0[empty])


@pytest.mark.parametrize("rows, C, entries", sc.LMF_ROUND_SHAPES)
def test_rows_kernel_second_grid_round(gpu, rows, C, entries):
    """More rows of 1 .. 512 entries than lmf_rows_kernel has groups in flight on 256 CUs (32 768 at 16 lanes, 16 384 at 32,
    8 192 at 64): its `i += ngroups` takes a second step.  The rows a dropped second step would leave alone are the last of
    the schedule order, the shortest rows with the highest ids.  The 32-lane shape is the user side of the class matrix that
    test_half_sweeps_match_float64 runs at C = 130; the other two have 40 items, so Y is small."""
    m = _class_matrix(rows, seed=C) if C == 130 else sc.lmf_round_matrix(rows, entries, seed=C)
    order = sc.lmf_schedule_order(m)
    in_flight = sc.lmf_groups_in_flight(C)
    assert m.shape[0] == rows and in_flight < len(order) < 2 * in_flight
    rng = np.random.default_rng(C)
    X0, Y0 = _factors(m.shape[0], C, rng), _factors(m.shape[1], C, rng)
    G0 = rng.uniform(0.0, 2.0, X0.shape).astype(np.float32)
    Xg, Gg = _sweep(gpu, m, X0, Y0, G0, 0.7, 0.2, 1, 99)
    X64, G64, bX, bG = ref.half_sweep64(m, X0, Y0, G0, 0.7, 0.2, 1, 99)
    second = order[in_flight:]  # the rows of the second step
    _assert_within(Xg[second], X64[second], bX[second], "X, rows of the second round")
    _assert_within(Gg[second], G64[second], bG[second], "G, rows of the second round")
    _assert_within(Xg, X64, bX, "X")
    _assert_within(Gg, G64, bG, "G")
    empty = np.diff(m.indptr) == 0
    assert empty.any()
    assert_array_equal(Xg[empty], X0[empty])
    assert_array_equal(Gg[empty], G0[empty])
    # no row with entries is left as it was: the bound alone would let a row through whose step is below it
    assert not (Xg[~empty] == X0[~empty]).all(axis=1).any()
    assert not (Gg[~empty] == G0[~empty]).all(axis=1).any()


# ---- 3. the negative count -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neg_prop", [1, 2, 30])
def test_negative_count_probe(gpu, neg_prop):
    g = np.load(GOLDEN)
    m = _golden_csr(g, "kprobe")
    C = int(g["kprobe_C"])
    _, Gg = _sweep(gpu, m, np.zeros((3, C), np.float32), np.ones((30, C), np.float32), np.zeros((3, C), np.float32), 1.0, 0.0,
                   neg_prop, 77)
    assert_array_equal(Gg, g[f"kprobe_G_np{neg_prop}"])


# ---- 4. the bias column, empty rows, determinism ------------------------------------------------------------------------------
def test_one_col_reset_and_empty_rows(gpu):
    m = _class_matrix(3000, seed=4)
    rng = np.random.default_rng(4)
    C = 12
    X0, Y0 = _factors(m.shape[0], C, rng), _factors(m.shape[1], C, rng)
    empty = np.diff(m.indptr) == 0
    assert empty.any() and (~empty).any()
    for one_col in (C - 2, C - 1):
        Xg, Gg = _sweep(gpu, m, X0, Y0, np.zeros_like(X0), 1.0, 0.6, 30, 5, one_col)
        assert (Xg[:, one_col] == 1.0).all()
        others = np.arange(C) != one_col
        assert_array_equal(Xg[empty][:, others], X0[empty][:, others])
        assert not Gg[empty].any() and Gg[~empty].all()
        assert (Xg[~empty][:, others] != X0[~empty][:, others]).mean() > 0.99


def test_bitwise_reproducible_and_seed_dependent(gpu):
    m = _class_matrix(20000, seed=5).T.tocsr()
    rng = np.random.default_rng(5)
    C = 34
    X0, Y0 = _factors(m.shape[0], C, rng), _factors(m.shape[1], C, rng)
    G0 = rng.uniform(0, 1, X0.shape).astype(np.float32)
    cui = gpu.CSRMatrix(m)
    runs = []
    for seed in (11, 11, 12):
        X, Y, G = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix(G0)
        gpu.lmf_update(cui, X, Y, G, 1.0, 0.6, 30, seed, C - 1)
        runs.append((X.to_numpy(), G.to_numpy()))
    assert_array_equal(runs[0][0], runs[1][0])
    assert_array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][0], runs[2][0]) and not np.array_equal(runs[0][1], runs[2][1])


def test_empty_matrix_only_sets_one_col(gpu):
    X0 = _factors(4, 6, np.random.default_rng(0))
    Xg, Gg = _sweep(gpu, csr_matrix((4, 3), dtype=np.float32), X0, np.ones((3, 6), np.float32), np.zeros_like(X0), 1.0, 0.6, 30,
                    1, 4)
    want = X0.copy()
    want[:, 4] = 1.0
    assert_array_equal(Xg, want)
    assert not Gg.any()


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    m = _class_matrix(2000, seed=6)
    rng = np.random.default_rng(6)
    C = 10
    X0, Y0 = _factors(m.shape[0], C, rng), _factors(m.shape[1], C, rng)
    G0 = rng.uniform(0, 1, X0.shape).astype(np.float32)
    cui = gpu.CSRMatrix(m)
    X, Y, G = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix(G0)
    users, items = m.shape
    bad = [
        (cui, gpu.Matrix(_factors(users + 1, C, rng)), Y, gpu.Matrix(_factors(users + 1, C, rng)), 30, -1),  # X.rows
        (cui, X, gpu.Matrix(_factors(items + 1, C, rng)), G, 30, -1),  # Y.rows
        (cui, X, gpu.Matrix(_factors(items, C + 1, rng)), G, 30, -1),  # columns
        (cui, X, Y, gpu.Matrix(_factors(users, C - 1, rng)), 30, -1),  # G's shape
        (cui, X, Y, gpu.Matrix(_factors(users - 1, C, rng)), 30, -1),
        (cui, X, Y.astype(np.float16), G, 30, -1),  # dtype
        (cui, X, Y, G.astype(np.float16), 30, -1),
        (cui, X, Y, G, -1, -1),  # neg_prop
        (cui, X, Y, G, 30, C),  # one_col
        (cui, X, Y, G, 30, -2),
        (cui, X, Y, X, 30, -1),  # X is G
    ]
    for C_bad in (2, 1025):
        bad.append((cui, gpu.Matrix(_factors(users, C_bad, rng)), gpu.Matrix(_factors(items, C_bad, rng)),
                    gpu.Matrix(_factors(users, C_bad, rng)), 30, -1))
    square = csr_matrix(np.eye(8, dtype=np.float32))
    S = gpu.Matrix(_factors(8, C, rng))
    bad.append((gpu.CSRMatrix(square), S, S, gpu.Matrix(_factors(8, C, rng)), 30, -1))  # X is Y
    for k, (c, x, y, gg, neg_prop, one_col) in enumerate(bad):
        with pytest.raises(ValueError):
            gpu.lmf_update(c, x, y, gg, 1.0, 0.6, neg_prop, 1, one_col)
        assert_array_equal(X.to_numpy(), X0, err_msg=str(k))
        assert_array_equal(G.to_numpy(), G0, err_msg=str(k))
    with pytest.raises(TypeError):
        gpu.lmf_update(m, X, Y, G, 1.0, 0.6, 30, 1)
    with pytest.raises(TypeError):
        gpu.lmf_update(cui, X0, Y, G, 1.0, 0.6, 30, 1)
    assert_array_equal(X.to_numpy(), X0)


def test_plane_cache_invalidated_by_lmf_update(gpu):
    m = _class_matrix(4000, seed=7).T.tocsr()  # rows of X are the items KnnQuery ranks
    rng = np.random.default_rng(7)
    C = 66
    X0, Y0 = _factors(m.shape[0], C, rng), _factors(m.shape[1], C, rng)
    X, Y, G = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix.zeros(m.shape[0], C)
    knn, Q = gpu.KnnQuery(), gpu.Matrix(Y0[:64])
    before = knn.topk(X, Q, 10)[0]
    gpu.lmf_update(gpu.CSRMatrix(m), X, Y, G, 1.0, 0.0, 30, 3, C - 1)
    after = knn.topk(X, Q, 10)[0]
    want = gpu.KnnQuery().topk(gpu.Matrix(X.to_numpy()), gpu.Matrix(Y0[:64]), 10)[0]
    assert (after == want).mean() > 0.99 and (before != want).mean() > 0.2


# ---- 6. the model -----------------------------------------------------------------------------------------------------------
def _model(**kw):
    import implicit_amd.lmf

    args = dict(factors=16, iterations=3, random_state=42)
    args.update(kw)
    return implicit_amd.lmf.LogisticMatrixFactorization(**args)


def _small_matrix(users=60, items=50, seed=2):
    rng = np.random.default_rng(seed)
    dense = (rng.random((users, items)) < 0.2) * rng.uniform(1, 3, (users, items))
    dense[3] = 0  # an empty user
    dense[:, 7] = 0  # an item nobody liked
    return csr_matrix(dense.astype(np.float32))


def test_initial_factors_match_reference_formula(gpu):
    m = _small_matrix()
    model = _model(iterations=0)
    model.fit(m, show_progress=False)
    X0, Y0, _ = ref.init_factors(m, 16, 42)
    assert_array_equal(model.user_factors.to_numpy(), X0)
    assert_array_equal(model.item_factors.to_numpy(), Y0)


def test_fit_bias_columns_callback_and_inputs(gpu):
    from implicit_amd.utils import ParameterWarning

    m = _small_matrix()
    calls = []
    model = _model(iterations=5)
    model.fit(m, show_progress=False, callback=lambda *a: calls.append(a))
    assert len(calls) == 5 and all(len(a) == 2 for a in calls)
    X, Y = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    assert (X[:, -2] == 1.0).all() and (Y[:, -1] == 1.0).all()
    assert np.isfinite(X).all() and np.isfinite(Y).all()
    for data in (m.astype(np.float64), m.tocoo()):
        model = _model()
        if isinstance(data, csr_matrix):
            with warnings.catch_warnings():
                warnings.simplefilter("error", ParameterWarning)
                model.fit(data, show_progress=False)
        else:
            with pytest.warns(ParameterWarning):
                model.fit(data, show_progress=False)
        again = _model()
        again.fit(m, show_progress=False)
        assert_array_equal(model.user_factors.to_numpy(), again.user_factors.to_numpy())


def test_second_fit_continues_with_fresh_accumulators(gpu):
    m = _small_matrix()
    model = _model(iterations=2)
    model.fit(m, show_progress=False)
    X1, Y1 = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    model.iterations = 1
    model.fit(m, show_progress=False)
    rs = np.random.default_rng(42)  # factors exist: no initial draws, the first two integers seed the two halves
    X, Y = gpu.Matrix(X1), gpu.Matrix(Y1)
    C = X1.shape[1]
    mt = m.T.tocsr()
    mt.sort_indices()
    gpu.lmf_update(gpu.CSRMatrix(m), X, Y, gpu.Matrix.zeros(*X1.shape), 1.0, 0.6, 30, rs.integers(2**31), C - 2)
    gpu.lmf_update(gpu.CSRMatrix(mt), Y, X, gpu.Matrix.zeros(*Y1.shape), 1.0, 0.6, 30, rs.integers(2**31), C - 1)
    assert_array_equal(model.user_factors.to_numpy(), X.to_numpy())
    assert_array_equal(model.item_factors.to_numpy(), Y.to_numpy())


def test_save_load_and_pickle(gpu, tmp_path):
    import implicit_amd.gpu.lmf as glmf

    m = _small_matrix()
    model = _model()
    model.fit(m, show_progress=False)
    path = str(tmp_path / "lmf.npz")
    model.save(path)
    with np.load(path) as data:
        assert set(data.files) == {"user_factors", "item_factors", "regularization", "factors", "learning_rate", "neg_prop",
                                   "iterations", "dtype", "random_state"}
    loaded = glmf.LogisticMatrixFactorization.load(path)
    assert_array_equal(loaded.item_factors.to_numpy(), model.item_factors.to_numpy())
    assert loaded.neg_prop == 30 and loaded.factors == 16
    buf = io.BytesIO()
    pickle.dump(model, buf)
    again = pickle.loads(buf.getvalue())
    assert_array_equal(again.user_factors.to_numpy(), model.user_factors.to_numpy())
    ids, _ = again.recommend(0, m[0], N=3)
    assert_array_equal(ids, model.recommend(0, m[0], N=3)[0])


# ---- 7. learning ------------------------------------------------------------------------------------------------------------
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


_REF_SCRIPT = r"""
import sys, warnings
import numpy as np
from scipy.sparse import load_npz
warnings.simplefilter("ignore")
from implicit.cpu.lmf import LogisticMatrixFactorization
m = LogisticMatrixFactorization(factors=8, iterations=20, random_state=int(sys.argv[2]), num_threads=8)
m.fit(load_npz(sys.argv[1]), show_progress=False)
np.save(sys.argv[3], m.user_factors); np.save(sys.argv[4], m.item_factors)
"""


def test_learning_against_serial_and_reference(gpu, tmp_path):
    """Held-out AUC of the GPU model (defaults: lr 1, reg 0.6, neg_prop 30; factors 8, 20 epochs) against the serial float64
    fit over the same draws (per seed, within 0.01) and, where the reference is built, against its CPU LMF from the same
    random_state -- identical initial factors, its own draws (the mean over three seeds within 0.02; per seed they differ
    by up to 0.018 on the host)."""
    import implicit_amd.gpu.lmf as glmf
    from scipy.sparse import save_npz

    aucs_gpu, aucs_ref = [], []
    for seed in range(3):
        train, held = _planted(seed)
        model = glmf.LogisticMatrixFactorization(factors=8, iterations=20, random_state=seed)
        model.fit(train, show_progress=False)
        auc_gpu = _held_out_auc(model.user_factors.to_numpy(), model.item_factors.to_numpy(), train, held)
        X0, Y0, rs = ref.init_factors(train, 8, seed)
        X, Y = ref.serial_fit(train, X0, Y0, [rs.integers(2**31) for _ in range(40)], 1.0, 0.6, 30)
        auc_ser = _held_out_auc(X, Y, train, held)
        print(f"seed {seed}: held-out AUC gpu {auc_gpu:.4f} serial {auc_ser:.4f}")
        assert abs(auc_gpu - auc_ser) < 0.01 and auc_gpu > 0.85
        aucs_gpu.append(auc_gpu)
        if os.path.isdir(SUITE):
            path = str(tmp_path / f"train{seed}.npz")
            save_npz(path, train)
            out = [str(tmp_path / f"{w}{seed}.npy") for w in "XY"]
            env = dict(os.environ, PYTHONPATH=os.pathsep.join([SUITE, ROOT]), OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="8")
            subprocess.run([sys.executable, "-c", _REF_SCRIPT, path, str(seed), *out], env=env, check=True, timeout=300)
            aucs_ref.append(_held_out_auc(np.load(out[0]), np.load(out[1]), train, held))
    if aucs_ref:
        print(f"mean held-out AUC gpu {np.mean(aucs_gpu):.4f} reference {np.mean(aucs_ref):.4f}")
        assert abs(np.mean(aucs_gpu) - np.mean(aucs_ref)) < 0.02
