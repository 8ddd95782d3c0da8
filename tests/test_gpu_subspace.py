"""The block-subspace half sweep (iALS++; csrc/als_subspace.hip) from the C entry point up to the model.  Problems and the two
restatements: tests/subspace_cases.py, proved on the CPU by tests/test_subspace_cases_host.py.

The yardstick throughout: with d the relative Frobenius distance from the float64 restatement, the GPU may be at most twice as
far as the float32 restatement whose sums run left to right, d_gpu <= max(2 d_f32, 2^-23) -- a different summation order of
the same length errs by the same order (the rule of tests/test_gpu_ease.py for the inverse) -- and no single row may be
further than twice the worst row of the float32 restatement.

A ValueError from a non-positive pivot is an answer of the API, not a fault of the device."""
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import cholesky_cases as cc
import subspace_cases as sc

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -23


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def call(gpu, p, k, sweeps=1, X0=None, C=None, solver=None):
    """(X after the call -- every row of X0, those beyond the matrix too --, the ValueError or None, Y and gramian after)."""
    solver = solver or gpu.LeastSquaresSolver()
    Xd, Yd, gram = gpu.Matrix(p.X0 if X0 is None else X0), gpu.Matrix(p.Y), gpu.Matrix(p.gram)
    error = None
    try:
        solver.least_squares_subspace(gpu.CSRMatrix(p.C if C is None else C), Xd, gram, Yd, p.reg, k, sweeps)
    except ValueError as e:
        error = e
    return Xd.to_numpy(), error, Yd.to_numpy(), gram.to_numpy()


def judge(label, got, x64, x32, rows=None):
    """Prints the figures, then holds `got` to the yardstick over `rows` (all rows of the restatements by default)."""
    rows = np.arange(len(x64)) if rows is None else np.asarray(rows)
    got = np.asarray(got)[:len(x64)]
    d_gpu, d_f32 = sc.distance(got, x64, rows), sc.distance(x32, x64, rows)
    e_gpu, e_f32 = cc.row_errors(got, x64)[rows], cc.row_errors(x32, x64)[rows]
    print(f"{label}: d_gpu = {d_gpu:.3e}  d_f32 = {d_f32:.3e}  ratio = {d_gpu / d_f32:.2f}  "
          f"worst row gpu = {e_gpu.max():.3e} (row {rows[e_gpu.argmax()]})  f32 = {e_f32.max():.3e}")
    assert np.isfinite(got[rows]).all()
    assert d_gpu <= max(2 * d_f32, FLOOR), (label, d_gpu, d_f32)
    worst = rows[e_gpu.argmax()]
    assert e_gpu.max() <= 2 * e_f32.max(), (label, int(worst), float(e_gpu.max()), float(e_f32.max()))


# ---- 1. the grid against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", sc.SWEEPS)
@pytest.mark.parametrize("f,k", sc.GRID)
def test_grid_against_float64(gpu, f, k, sweeps):
    p = sc.routes_problem(f)
    x64, x32, _ = sc.reference("routes", f, k, max(sc.SWEEPS))
    got, error, _, _ = call(gpu, p, k, sweeps)
    assert error is None
    judge(f"f={f} k={k} sweeps={sweeps}", got, x64[sweeps - 1], x32[sweeps - 1])


# ---- 2. one block that covers the row is the exact solve, whatever the start -----------------------------------------------------
@pytest.mark.parametrize("f", [8, 16, 32])
def test_one_block_is_the_cholesky_half_sweep(gpu, f):
    p = sc.routes_problem(f)
    exact, failing = cc.solve_f64(p.C, p.Y, p.gram, p.reg)
    assert failing == []
    n = p.C.shape[0]
    chol = gpu.Matrix(p.X0)
    gpu.LeastSquaresSolver().least_squares_cholesky(gpu.CSRMatrix(p.C), chol, gpu.Matrix(p.gram), gpu.Matrix(p.Y), p.reg)
    chol = chol.to_numpy()[:n]
    rng = np.random.default_rng(f)
    for name, X0 in (("warm", p.X0), ("far", (rng.standard_normal(p.X0.shape) * 0.3).astype(np.float32))):
        (x32,), _ = sc.sweep_f32(p.C, X0, p.Y, p.gram, p.reg, f)
        got, error, _, _ = call(gpu, p, f, 1, X0=X0)
        assert error is None
        judge(f"exact f=k={f} {name} start", got, exact, x32)
        yard = max(2 * sc.distance(x32, exact), FLOOR)
        d_chol, apart = sc.distance(chol, exact), sc.distance(got[:n], chol)
        print(f"    least_squares_cholesky: d = {d_chol:.3e}; subspace to cholesky = {apart:.3e}; yardstick = {yard:.3e}")
        assert apart <= 2 * yard  # each within the yardstick of the float64 solve


# ---- 3. / 4. what a call writes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,k", [(20, 8), (130, 32), (16, 4)])
def test_only_the_rows_of_the_matrix_are_written(gpu, f, k):
    p = sc.routes_problem(f)
    lens = np.diff(p.C.indptr)
    n = p.C.shape[0]
    X0 = p.X0 + np.float32(1.0)  # nothing is zero before the call
    # the whole matrix (its last row goes through the segment kernels), and its first 19 rows (the last one: one wavefront):
    # a block's padding beyond the last factor would land in the row after
    for rows in (n, len(cc.LENGTHS)):
        got, error, Y, gram = call(gpu, p, k, 2, X0=X0, C=p.C[:rows])
        assert error is None
        assert not got[:rows][lens[:rows] == 0].any(), "empty rows"
        assert np.signbit(got[:rows][lens[:rows] == 0]).sum() == 0
        assert bits(got[rows:]) == bits(X0[rows:]), "rows beyond the matrix"
        assert (got[:rows][lens[:rows] > 0] != X0[:rows][lens[:rows] > 0]).any(axis=1).all(), "every other row is solved"
        assert bits(Y) == bits(p.Y) and bits(gram) == bits(p.gram)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,k,sweeps", [(130, 32, 3), (20, 1, 1), (64, 16, 2)])
def test_equal_inputs_give_equal_bits(gpu, f, k, sweeps):
    p = sc.routes_problem(f)
    first, _, _, _ = call(gpu, p, k, sweeps)
    gpu.release_workspaces()
    second, _, _, _ = call(gpu, p, k, sweeps)
    assert bits(first) == bits(second)


# ---- 6. the failure path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,k,failing", [(64, 16, s) for s in sc.FAILING_SETS] + [(32, 32, sc.FAILING_SETS[0]),
                                                                                   (20, 8, sc.FAILING_SETS[0])])
def test_a_failing_block_names_the_smallest_row_and_spares_the_others(gpu, f, k, failing):
    p = sc.failing_problem(f, tuple(failing))
    x64, x32, bad = sc.reference("failing", f, k, 1, tuple(failing))
    assert bad == sorted(failing)
    solver = gpu.LeastSquaresSolver()
    got, error, _, _ = call(gpu, p, k, 1, solver=solver)
    assert isinstance(error, ValueError) and error.failed_row == min(failing), error
    n = p.C.shape[0]
    sound = [u for u in range(n) if u not in failing]
    judge(f"failing {failing} f={f} k={k}, the other rows", got, x64[0], x32[0], rows=sound)
    assert bits(got[n:]) == bits(p.X0[n:])
    # nothing is left behind: a sound problem on the same solver right afterwards
    q = sc.routes_problem(f)
    y64, y32, _ = sc.reference("routes", f, k, max(sc.SWEEPS))
    again, error, _, _ = call(gpu, q, k, 1, solver=solver)
    assert error is None
    judge(f"sound problem after failing {failing} f={f} k={k}", again, y64[0], y32[0])


@pytest.mark.parametrize("failing", cc.BLOCK_FAILING_SETS, ids=lambda s: "rows" + "_".join(map(str, s)))
def test_a_failing_row_is_numbered_in_the_whole_matrix_across_row_blocks(gpu, monkeypatch, failing):
    """The matrix held as four row blocks (rows 0 .. 14, 15, 16 .. 17, 18: the nonzeros per row are those of the Cholesky problem,
    tests/test_cholesky_cases_host.py::test_block_limit_puts_the_failing_rows_in_three_blocks): a block reports a row numbered
    inside the block, the call names the row of the whole matrix -- row 16 from the third block, row 15 from the second before
    row 16 from the third, row 4 from the first."""
    f, k = 64, 16
    p = sc.failing_problem(f, tuple(failing))
    x64, x32, bad = sc.reference("failing", f, k, 1, tuple(failing))
    assert bad == sorted(failing)
    C64 = p.C.copy()
    C64.indptr = C64.indptr.astype(np.int64)
    C64.indices = C64.indices.astype(np.int64)
    monkeypatch.setenv("IMP_CSR_PART_NNZ", str(cc.BLOCK_NNZ))
    blocks = gpu.CSRMatrix(C64)
    monkeypatch.delenv("IMP_CSR_PART_NNZ")
    Xd = gpu.Matrix(p.X0)
    with pytest.raises(ValueError) as e:
        gpu.LeastSquaresSolver().least_squares_subspace(blocks, Xd, gpu.Matrix(p.gram), gpu.Matrix(p.Y), p.reg, k, 1)
    assert e.value.failed_row == min(failing), e.value
    got, n = Xd.to_numpy(), p.C.shape[0]
    sound = [u for u in range(n) if u not in failing]
    judge(f"failing {failing} f={f} k={k} in row blocks, the other rows", got, x64[0], x32[0], rows=sound)
    assert bits(got[n:]) == bits(p.X0[n:])


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_value_errors(gpu):
    p = sc.routes_problem(16)
    solver, C = gpu.LeastSquaresSolver(), gpu.CSRMatrix(p.C)
    X, Y, gram = gpu.Matrix(p.X0), gpu.Matrix(p.Y), gpu.Matrix(p.gram)

    def refused(*args):
        with pytest.raises(ValueError) as e:
            solver.least_squares_subspace(*args)
        assert e.value.failed_row == -1
        assert bits(X.to_numpy()) == bits(p.X0)

    refused(C, gpu.Matrix(p.X0.astype(np.float16)), gram, Y, p.reg, 8, 1)
    refused(C, X, gram, gpu.Matrix(p.Y.astype(np.float16)), p.reg, 8, 1)
    refused(C, X, gram, Y, p.reg, 0, 1)
    refused(C, X, gram, Y, p.reg, 33, 1)
    refused(C, X, gram, Y, p.reg, 8, 0)
    refused(C, X, gpu.Matrix(np.eye(17, dtype=np.float32)), Y, p.reg, 8, 1)
    refused(C, X, gpu.Matrix(np.zeros((15, 16), np.float32)), Y, p.reg, 8, 1)
    refused(C, X, gram, gpu.Matrix(p.Y[:100]), p.reg, 8, 1)          # fewer item rows than columns
    refused(gpu.CSRMatrix(sc.routes_problem(8).C[:3]), gpu.Matrix.zeros(3, 1025), gpu.Matrix.zeros(1025, 1025),
            gpu.Matrix.zeros(sc.COLS, 1025), p.reg, 8, 1)
    solver.least_squares_subspace(C, X, gram, Y, p.reg, 8, 1)         # and the sound call goes through
    assert bits(X.to_numpy()) != bits(p.X0)


# ---- 8. - 10. the model ---------------------------------------------------------------------------------------------------------------
FACTORS, BLOCK, ITERATIONS, SEED = 40, 16, 3, 7
_MODEL = {}


def fitted(gpu):
    """(matrix, initial factors, the fitted model, host restatements): fitted once."""
    if not _MODEL:
        from implicit_amd.gpu.als import AlternatingLeastSquares
        from implicit_amd.synthetic import synthetic_csr
        from implicit_amd.utils import check_random_state, random_factors

        Cui = synthetic_csr(300, 200, 5000, seed=11, neg_frac=0.05)
        rng = check_random_state(SEED)
        X0 = random_factors(rng, Cui.shape[0], FACTORS)
        Y0 = random_factors(rng, Cui.shape[1], FACTORS)
        model = AlternatingLeastSquares(factors=FACTORS, block_size=BLOCK, iterations=ITERATIONS, random_state=SEED)
        model.fit(Cui, show_progress=False)
        _MODEL.update(Cui=Cui, X0=X0, Y0=Y0, model=model, X=model.user_factors.to_numpy(), Y=model.item_factors.to_numpy(),
                      f64=sc.alternate(sc.sweep_f64, Cui, X0, Y0, model.regularization, BLOCK, ITERATIONS),
                      f32=sc.alternate(sc.sweep_f32, Cui, X0, Y0, model.regularization, BLOCK, ITERATIONS))
    return SimpleNamespace(**_MODEL)


def test_model_fit_is_the_alternated_sweep(gpu):
    m = fitted(gpu)
    for name, got, want, ref in (("users", m.X, m.f64[0], m.f32[0]), ("items", m.Y, m.f64[1], m.f32[1])):
        d_gpu, d_f32 = sc.distance(got, want), sc.distance(ref, want)
        print(f"model {name}: d_gpu = {d_gpu:.3e}  d_f32 = {d_f32:.3e}  ratio = {d_gpu / d_f32:.2f}")
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert d_gpu <= max(2 * d_f32, FLOOR)


def test_model_loss_falls_and_the_derived_caches_follow(gpu):
    from implicit_amd.gpu.als import calculate_loss

    m = fitted(gpu)
    model = m.model
    before = calculate_loss(m.Cui, m.X0, m.Y0, model.regularization)
    after = calculate_loss(m.Cui, m.X, m.Y, model.regularization)
    print(f"loss {before:.5f} -> {after:.5f}")
    assert after < before
    user, item, N = 5, 3, 6

    def expected():
        X, Y = model.user_factors.to_numpy().astype(np.float64), model.item_factors.to_numpy().astype(np.float64)
        scores = np.sort(Y @ X[user])[::-1][:N]
        norms = np.maximum(np.linalg.norm(Y, axis=1), 1e-10)  # what calculate_norms makes of an unused item's zero row
        cosine = np.sort((Y @ Y[item]) / norms / norms[item])[::-1][:N]
        return scores, cosine

    def served():
        _, scores = model.recommend(user, m.Cui[user], N=N, filter_already_liked_items=False)
        _, cosine = model.similar_items(item, N=N)
        return np.asarray(scores, np.float64), np.asarray(cosine, np.float64)

    first = served()
    for got, want in zip(first, expected()):
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
    old = bits(model.item_factors.to_numpy())
    model.fit(m.Cui * 3.0, show_progress=False)  # a second fit, from the current factors, on other confidences
    assert bits(model.item_factors.to_numpy()) != old
    second = served()
    for got, want in zip(second, expected()):
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
    assert not np.allclose(first[0], second[0], rtol=1e-4)


def test_model_pickle_default_and_refused_arguments(gpu):
    from implicit_amd.als import AlternatingLeastSquares as factory
    from implicit_amd.gpu.als import AlternatingLeastSquares

    m = fitted(gpu)
    twin = pickle.loads(pickle.dumps(m.model))
    assert twin.block_size == BLOCK and twin.subspace_sweeps == 1
    assert bits(twin.user_factors.to_numpy()) == bits(m.model.user_factors.to_numpy())
    assert factory(factors=FACTORS, block_size=8, subspace_sweeps=2).block_size == 8

    plain = AlternatingLeastSquares(factors=FACTORS, iterations=2, random_state=SEED)
    keyword = AlternatingLeastSquares(factors=FACTORS, iterations=2, random_state=SEED, block_size=None)
    assert keyword.block_size is None
    for model in (plain, keyword):
        model.fit(m.Cui, show_progress=False)
    assert bits(plain.user_factors.to_numpy()) == bits(keyword.user_factors.to_numpy())
    assert bits(plain.item_factors.to_numpy()) == bits(keyword.item_factors.to_numpy())
    assert bits(plain.user_factors.to_numpy()) != bits(m.X[:, :FACTORS])  # and the subspace fit is another solver

    for refused in (dict(use_cg=False), dict(dtype=np.float16), dict(comm=SimpleNamespace(nranks=2, rank=0)),
                    dict(block_size=0), dict(block_size=33), dict(subspace_sweeps=0)):
        with pytest.raises(ValueError):
            AlternatingLeastSquares(**{"factors": FACTORS, "block_size": BLOCK, **refused})
