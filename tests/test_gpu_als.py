"""GPU parity tests for the ALS solvers: HIP kernels (through the C-ABI shim) vs the CPU oracle.

Tolerances (BASELINE.json north_star): factor matrices within 1e-4 relative Frobenius of the
reference CPU path on the same inputs.  The cold first sweep from the default init is
ill-conditioned -- there the fp32 oracle itself is 1e-4..1e-3 away from the exact (fp64) answer
 -- so it is gated against the oracle's own fp64 distance instead.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from implicit_amd.synthetic import synthetic_csr

pytestmark = pytest.mark.gpu

TOL = 1e-4


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _problem(users, items, nnz, f, seed=1, neg=0.05, empty=0.01):
    C = synthetic_csr(users, items, nnz, seed=seed, neg_frac=neg, empty_frac=empty)
    rng = np.random.default_rng(7)
    X0 = rng.random((users, f), dtype=np.float32) * 0.01
    Y0 = rng.random((items, f), dtype=np.float32) * 0.01
    return C, X0, Y0


def _gpu_cg(gpu, C, X, Y, reg, cg_steps):
    solver = gpu.LeastSquaresSolver()
    Xd, Yd = gpu.Matrix(X), gpu.Matrix(Y)
    gram = gpu.Matrix.zeros(X.shape[1], X.shape[1])
    solver.calculate_yty(Yd, gram, reg)
    solver.least_squares(gpu.CSRMatrix(C), Xd, gram, Yd, cg_steps)
    return Xd.to_numpy(), gram.to_numpy()


@pytest.mark.parametrize("f", [16, 32, 50, 64, 100, 128, 256])
def test_gramian(gpu, oracle, f):
    rng = np.random.default_rng(0)
    Y = (rng.random((3001, f), dtype=np.float32) - 0.3).astype(np.float32)
    solver = gpu.LeastSquaresSolver()
    out = gpu.Matrix.zeros(f, f)
    solver.calculate_yty(gpu.Matrix(Y), out, 0.25)
    want = oracle.gramian(Y) + np.float32(0.25) * np.eye(f, dtype=np.float32)
    got = out.to_numpy()
    assert rel(got, want) < 1e-6
    assert np.array_equal(got, got.T)  # symmetric bit for bit is not required, but transposition bugs show here
    

@pytest.mark.parametrize("f", [6, 16, 32, 50, 64, 100, 128, 200, 256])
@pytest.mark.parametrize("cg_steps", [1, 3])
def test_cg_warm_sweep(gpu, oracle, f, cg_steps):
    """Per-call parity from identical inputs in a warm state (after oracle sweeps)."""
    C, X0, Y0 = _problem(3000, 1200, 90_000, f)
    Ct = C.T.tocsr()
    X, Y = X0.copy(), Y0.copy()
    for _ in range(2):
        oracle.least_squares_cg(C, X, Y, 0.01)
        oracle.least_squares_cg(Ct, Y, X, 0.01)
    for M, A, B in ((C, X, Y), (Ct, Y, X)):
        want = A.copy()
        oracle.least_squares_cg(M, want, B, 0.01, cg_steps=cg_steps)
        got, _ = _gpu_cg(gpu, M, A.copy(), B, 0.01, cg_steps)
        err = rel(got, want)
        print(f"f={f} cg={cg_steps} rows={M.shape[0]} warm rel={err:.2e}")
        assert err < TOL


@pytest.mark.parametrize("f", [64, 128])
def test_cg_cold_sweep_vs_fp64(gpu, oracle, f):
    """Cold first sweep: gated against the exact (fp64) answer with the oracle's own noise as the bar."""
    C, X0, Y0 = _problem(4000, 1500, 120_000, f)
    exact = oracle.least_squares_cg_f64(C, X0, Y0, 0.01)
    want = X0.copy()
    oracle.least_squares_cg(C, want, Y0, 0.01)
    got, _ = _gpu_cg(gpu, C, X0.copy(), Y0, 0.01, 3)
    e_gpu, e_oracle = rel(got, exact), rel(want, exact)
    print(f"f={f} cold: gpu-vs-fp64 {e_gpu:.2e}  oracle-vs-fp64 {e_oracle:.2e}  gpu-vs-oracle {rel(got, want):.2e}")
    assert e_gpu < max(TOL, 2.0 * e_oracle)


# every cut of the row schedule from both sides (and the cuts of round 6's experiment with team widths 3 and 5, 96 and 160
# nonzeros: measured slower, not kept -- DESIGN 4.1, profiles/r06_team_widths.txt) with several rows per length so that teams of one workgroup get rows of
# different lengths
TEAM_EDGE_LENGTHS = [30, 32, 33, 40, 63, 64, 65, 66, 80, 93, 95, 96, 97, 100, 127, 128, 129, 130, 144, 157, 159, 160, 161, 162, 200, 255,
                     256, 257, 300, 511, 512, 513, 0]


def _edge_matrix(lengths, items, seed, neg_frac=0.1):
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for n in lengths:
        cols = np.sort(rng.choice(items, size=n, replace=False))
        c = 1 + 4 * rng.random(n)
        c[rng.random(n) < neg_frac] *= -1
        indices.append(cols)
        data.append(c)
        indptr.append(indptr[-1] + n)
    return sp.csr_matrix((np.concatenate(data).astype(np.float32), np.concatenate(indices).astype(np.int32), np.array(indptr)),
                         shape=(len(lengths), items))


@pytest.mark.parametrize("cg_steps", [1, 3])
@pytest.mark.parametrize("f", [128, 64])
def test_team_width_boundaries_row_by_row(gpu, oracle, f, cg_steps):
    """Per-ROW parity (1e-4 each: a wrong share of the gramian rows or of the entries in ONE team would hide in a Frobenius norm)
    at every cut of the schedule.  Reference: implicit/gpu/als.cu:23-111 == implicit/cpu/_als.pyx:152-248."""
    items = 3000
    lengths = TEAM_EDGE_LENGTHS * 7   # 7 rows per length: more rows than teams in a workgroup, a ragged last round
    C = _edge_matrix(lengths, items, seed=f + cg_steps)
    rng = np.random.default_rng(11)
    Y = ((rng.random((items, f), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    X = ((rng.random((C.shape[0], f), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    want = X.copy()
    oracle.least_squares_cg(C, want, Y, 0.05, cg_steps=cg_steps)
    got, _ = _gpu_cg(gpu, C, X.copy(), Y, 0.05, cg_steps)
    num = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    err = num / np.maximum(np.linalg.norm(want.astype(np.float64), axis=1), 1e-30)
    print("f", f, "cg", cg_steps, "per-row rel max %.2e" % err.max(), "at length", lengths[int(err.argmax())])
    assert err.max() < TOL
    empty = np.asarray(lengths) == 0
    assert not got[empty].any()


# the cuts of the packed-fp16 team kernel (64 entries per wavefront: team widths 1 / 2 / 4 / 8 up to 64 / 128 / 256 / 512
# nonzeros) and of the short rows (<= 32) from both sides
HALF_TEAM_EDGE_LENGTHS = [31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 0]


@pytest.mark.parametrize("cg_steps", [1, 3])
@pytest.mark.parametrize("f", [128, 64])
def test_half_team_width_boundaries_row_by_row(gpu, oracle, f, cg_steps):
    """float16 storage: per-ROW parity at every cut of the packed 64-entry tile kernel, within 1e-3 of the oracle run on the
    fp16-rounded inputs (the result is stored in fp16).  The oracle is handed the GPU's gramian of the fp16 factors, which
    test_native_fp16_factor_storage pins to the fp32 gramian bit for bit.  The grid covers every row here, so each team
    solves one row: a wrong share of the entries or of the gramian rows, or a wrong weight-table slot, shows in that row."""
    items = 3000
    lengths = HALF_TEAM_EDGE_LENGTHS * 7   # 7 rows per length: several workgroups per class
    C = _edge_matrix(lengths, items, seed=f + cg_steps)
    rng = np.random.default_rng(11)
    Y = ((rng.random((items, f), dtype=np.float32) - 0.5) * 0.2).astype(np.float16)
    X = ((rng.random((C.shape[0], f), dtype=np.float32) - 0.5) * 0.2).astype(np.float16)
    got, gram = _gpu_cg(gpu, C, X.copy(), Y, 0.05, cg_steps)
    assert got.dtype == np.float16
    want = X.astype(np.float32)
    oracle.least_squares_cg(C, want, Y.astype(np.float32), 0.05, cg_steps=cg_steps, YtY=gram)
    num = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    err = num / np.maximum(np.linalg.norm(want.astype(np.float64), axis=1), 1e-30)
    print("f", f, "cg", cg_steps, "fp16 per-row rel max %.2e" % err.max(), "at length", lengths[int(err.argmax())])
    assert err.max() < 1e-3
    empty = np.asarray(lengths) == 0
    assert not got[empty].any()


def test_cg_long_rows_and_edge_cases(gpu, oracle):
    """Rows long enough for the workgroup-per-row class, empty rows, explicit zeros, negatives."""
    rng = np.random.default_rng(3)
    users, items, f = 300, 5000, 128
    dense_rows = sp.random(6, items, density=0.6, format="csr", dtype=np.float32, random_state=5)
    dense_rows.data = 1 + 4 * dense_rows.data
    rest = synthetic_csr(users - 6, items, 20_000, seed=9, neg_frac=0.1, empty_frac=0.05)
    C = sp.vstack([dense_rows, rest]).tocsr().astype(np.float32)
    C.data[::97] = 0.0  # explicit zeros take the `else` branch with confidence 0
    C.sort_indices()
    X0 = rng.random((users, f), dtype=np.float32) * 0.1 - 0.05
    Y0 = rng.random((items, f), dtype=np.float32) * 0.1 - 0.05
    want = X0.copy()
    oracle.least_squares_cg(C, want, Y0, 0.05)
    got, _ = _gpu_cg(gpu, C, X0.copy(), Y0, 0.05, 3)
    assert rel(got, want) < TOL
    empty = np.diff(C.indptr) == 0
    assert empty.any() and not got[empty].any()


@pytest.mark.parametrize("stripe", ["0", "256", "1024", None])
@pytest.mark.parametrize("f", [64, 128, 96])
def test_cg_long_rows_striped_plan(gpu, oracle, monkeypatch, stripe, f):
    """Long rows that re-use the gathered matrix >= 4x are cut at column-stripe boundaries and swept per XCD
    (imp_csr_create); plain plan (IMP_STRIPE=0), narrow stripes (many short segments) and the default must agree
    with the oracle, and an unsorted row falls back to the plain plan."""
    if stripe is None:
        monkeypatch.delenv("IMP_STRIPE", raising=False)
    else:
        monkeypatch.setenv("IMP_STRIPE", stripe)
    rng = np.random.default_rng(11)
    users, items = 200, 3000
    dense_rows = sp.random(14, items, density=0.45, format="csr", dtype=np.float32, random_state=2)
    dense_rows.data = 1 + 9 * dense_rows.data
    dense_rows.data[::13] *= -1  # negative confidence (dislikes)
    rest = synthetic_csr(users - 14, items, 9_000, seed=4, neg_frac=0.1, empty_frac=0.05)
    C = sp.vstack([rest[:50], dense_rows, rest[50:]]).tocsr().astype(np.float32)
    C.sort_indices()
    lens = np.diff(C.indptr)
    assert lens.max() > 1024 and lens[lens > 512].sum() >= 4 * items  # the striping condition holds
    X0 = rng.random((users, f), dtype=np.float32) * 0.1 - 0.05
    Y0 = rng.random((items, f), dtype=np.float32) * 0.1 - 0.05
    want = X0.copy()
    oracle.least_squares_cg(C, want, Y0, 0.05)
    got, _ = _gpu_cg(gpu, C, X0.copy(), Y0, 0.05, 3)
    assert rel(got, want) < TOL
    # same matrix with one long row's entries reversed (unsorted indices): plain plan, same answer
    U = C.copy()
    r = int(np.argmax(lens))
    lo, hi = U.indptr[r], U.indptr[r + 1]
    U.indices[lo:hi] = U.indices[lo:hi][::-1].copy()
    U.data[lo:hi] = U.data[lo:hi][::-1].copy()
    got_u, _ = _gpu_cg(gpu, U, X0.copy(), Y0, 0.05, 3)
    assert rel(got_u, want) < TOL


@pytest.mark.parametrize("f", [6, 32, 64, 100, 128, 160, 200, 256])  # > 160: packed-triangle LDS image
def test_cholesky_sweep(gpu, oracle, f):
    C, X0, Y0 = _problem(2000, 800, 60_000, f)
    want = X0.copy()
    oracle.least_squares(C, want, Y0, 0.01)
    solver = gpu.LeastSquaresSolver()
    Xd, Yd = gpu.Matrix(X0), gpu.Matrix(Y0)
    gram = gpu.Matrix.zeros(f, f)
    solver.calculate_yty(Yd, gram, 0.0)
    solver.least_squares_cholesky(gpu.CSRMatrix(C), Xd, gram, Yd, 0.01)
    err = rel(Xd.to_numpy(), want)
    print(f"f={f} cholesky rel={err:.2e}")
    assert err < TOL


@pytest.mark.parametrize("f", [260, 320, 640, 1024])  # beyond the LDS: the triangle in a device workspace (the CPU reference takes any f)
def test_cholesky_sweep_beyond_256_factors(gpu, oracle, f):
    C, X0, Y0 = _problem(300, 400, 9_000, f)
    C = C.tolil()
    C[5] = 0                                          # an empty row: zeroed (_als.pyx:95-97)
    C = C.tocsr()
    C.eliminate_zeros()
    want = X0.copy()
    oracle.least_squares(C, want, Y0, 0.01)
    solver = gpu.LeastSquaresSolver()
    Xd, Yd = gpu.Matrix(X0), gpu.Matrix(Y0)
    gram = gpu.Matrix.zeros(f, f)
    solver.calculate_yty(Yd, gram, 0.0)
    solver.least_squares_cholesky(gpu.CSRMatrix(C), Xd, gram, Yd, 0.01)
    got = Xd.to_numpy()
    err = rel(got, want)
    print(f"f={f} cholesky (workspace kernel) rel={err:.2e}")
    assert err < TOL
    assert not got[5].any()
    if f == 320:                                      # not positive definite -> ValueError naming the row, as below
        with pytest.raises(ValueError) as info:
            solver.least_squares_cholesky(gpu.CSRMatrix(C), gpu.Matrix(X0), gpu.Matrix.zeros(f, f),
                                          gpu.Matrix(np.zeros_like(Y0)), 0.0)
        assert C.indptr[1] > C.indptr[0] and info.value.failed_row == 0   # every non-empty row fails: row 0 is the smallest


def test_cholesky_not_positive_definite_raises(gpu):
    # zero factors + zero regularisation: the oracle raises ValueError (_als.pyx:136-138)
    C = sp.csr_matrix(np.ones((3, 4), dtype=np.float32))
    Y = np.zeros((4, 8), dtype=np.float32)
    X = np.zeros((3, 8), dtype=np.float32)
    solver = gpu.LeastSquaresSolver()
    gram = gpu.Matrix.zeros(8, 8)
    with pytest.raises(ValueError):
        solver.least_squares_cholesky(gpu.CSRMatrix(C), gpu.Matrix(X), gram, gpu.Matrix(Y), 0.0)


@pytest.mark.parametrize("f", [32, 128])
def test_loss(gpu, oracle, f):
    C, X0, Y0 = _problem(1500, 700, 40_000, f)
    X, Y = X0 * 30, Y0 * 30
    for reg in (0.0, 1.0):
        want = oracle.calculate_loss(C, X, Y, reg)
        got = gpu.LeastSquaresSolver().calculate_loss(gpu.CSRMatrix(C), gpu.Matrix(X), gpu.Matrix(Y), reg)
        assert got == pytest.approx(want, rel=1e-4)


def test_loss_known_answers(gpu):
    """tests/als_test.py:304-324 of the reference: losses 1.0 and 2.0."""
    ratings = sp.coo_matrix(([1.0], ([0], [0])), shape=(1, 2)).tocsr()
    item_factors = np.array([[0.0], [1.0]], dtype="float32")
    user_factors = np.array([[1.0]], dtype="float32")
    from implicit_amd.gpu.als import calculate_loss

    assert calculate_loss(ratings, user_factors, item_factors, regularization=0) == pytest.approx(1.0)
    assert calculate_loss(ratings, user_factors, item_factors, regularization=1.0) == pytest.approx(2.0)


def test_other_factor_counts_ride_the_resident_kernels(gpu, oracle):
    """Factor counts below 128 other than 64 are zero-padded onto the f = 64 / 128 kernels (exact for CG: the padded
    components of residual, direction and iterate stay zero).  A matrix with every row class -- short, team widths, rows
    beyond 512 and 4096 nonzeros -- at f = 100 and f = 20, a row-range view of X, and the outputs' padded columns never
    leak: the rows of X past the CSR's rows are untouched."""
    from implicit_amd.synthetic import synthetic_csr

    C = synthetic_csr(900, 30_000, 700_000, seed=31, neg_frac=0.04, empty_frac=0.02, sigma=2.0)
    assert np.diff(C.indptr).max() > 4096
    for f in (100, 20):
        rng = np.random.default_rng(f)
        X0 = rng.random((C.shape[0] + 7, f), dtype=np.float32) * 0.2 - 0.1   # 7 extra rows: not solved, must stay as they are
        Y0 = rng.random((C.shape[1], f), dtype=np.float32) * 0.2 - 0.1
        Xd, Yd, gram = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix.zeros(f, f)
        solver = gpu.LeastSquaresSolver()
        solver.calculate_yty(Yd, gram, 0.05)
        solver.least_squares(gpu.CSRMatrix(C), Xd, gram, Yd, 3)
        got = Xd.to_numpy()
        want = X0[:C.shape[0]].copy()
        oracle.least_squares_cg(C, want, Y0, 0.05, cg_steps=3, YtY=gram.to_numpy())
        err = rel(got[:C.shape[0]], want)
        print(f"f={f} padded route rel={err:.2e}")
        assert err < TOL
        np.testing.assert_array_equal(got[C.shape[0]:], X0[C.shape[0]:])


@pytest.mark.parametrize("f", [192, 320, 640, 1024])
def test_reference_factor_grid_beyond_128(gpu, oracle, f):
    """The reference's kernels take any factor count up to 1024 (one thread per factor, implicit/gpu/als.cu:177-182) and its
    benchmarks publish f = 192 (benchmarks/README.md:31,35).  129..255 ride the f = 256 kernels zero-padded, larger counts the
    lane-strided kernels; rows of every class (beyond 512 and 4096 nonzeros too), gramian and loss at the same f."""
    C = synthetic_csr(400, 9_000, 160_000 if f <= 320 else 60_000, seed=37, neg_frac=0.04, empty_frac=0.02, sigma=2.0)
    assert np.diff(C.indptr).max() > (4096 if f <= 320 else 512)
    rng = np.random.default_rng(f)
    X0 = rng.random((C.shape[0], f), dtype=np.float32) * 0.2 - 0.1
    Y0 = rng.random((C.shape[1], f), dtype=np.float32) * 0.2 - 0.1
    Xd, Yd, gram = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix.zeros(f, f)
    solver = gpu.LeastSquaresSolver()
    solver.calculate_yty(Yd, gram, 0.05)
    want_gram = oracle.gramian(Y0) + np.float32(0.05) * np.eye(f, dtype=np.float32)
    assert rel(gram.to_numpy(), want_gram) < 1e-6
    Cd = gpu.CSRMatrix(C)
    solver.least_squares(Cd, Xd, gram, Yd, 3)
    want = X0.copy()
    oracle.least_squares_cg(C, want, Y0, 0.05, cg_steps=3, YtY=gram.to_numpy())
    err = rel(Xd.to_numpy(), want)
    print(f"f={f} rel={err:.2e}")
    assert err < TOL
    loss = solver.calculate_loss(Cd, Xd, Yd, 0.05)
    assert loss == pytest.approx(oracle.calculate_loss(C, Xd.to_numpy(), Y0, 0.05), rel=1e-4)


def test_more_than_1024_factors_is_an_error_like_the_reference(gpu):
    C = synthetic_csr(10, 10, 30, seed=1)
    f = 1025
    X, Y, gram = gpu.Matrix.zeros(10, f), gpu.Matrix.zeros(10, f), gpu.Matrix.zeros(f, f)
    with pytest.raises(ValueError):
        gpu.LeastSquaresSolver().least_squares(gpu.CSRMatrix(C), X, gram, Y, 3)


def test_padded_copy_of_y_is_reused_only_while_it_is_valid(gpu, oracle):
    """f = 100 rides the f = 128 kernels on a zero-padded copy of Y.  The row chunks of a half sweep solve against the same Y
    under the same gramian: the copy is made once (decided on the device through the gramian, als_cg.hip).  It must NOT
    survive a write to Y through the library, nor a different gramian.  (Every other writer of Y, and memory the library cannot
    watch: tests/test_gpu_derived_state.py.)"""
    f = 100
    C = synthetic_csr(2400, 900, 60_000, seed=41, neg_frac=0.05, empty_frac=0.02)
    rng = np.random.default_rng(5)
    X0 = rng.random((C.shape[0], f), dtype=np.float32) * 0.2 - 0.1
    Y0 = rng.random((C.shape[1], f), dtype=np.float32) * 0.2 - 0.1
    solver = gpu.LeastSquaresSolver()
    Yd, gram = gpu.Matrix(Y0), gpu.Matrix.zeros(f, f)
    solver.calculate_yty(Yd, gram, 0.05)

    def oracle_rows(Y, rows=slice(None)):
        want = X0[rows].copy()
        oracle.least_squares_cg(C[rows], want, Y, 0.05, cg_steps=3, YtY=oracle.gramian(Y) + np.float32(0.05) * np.eye(f, dtype=np.float32))
        return want

    # three chunks against one Y: the second and third call find the copy in place
    Xd = gpu.Matrix(X0)
    cuts = [0, 800, 1600, 2400]
    gpu.Profiler.reset()
    gpu.Profiler.enable(True)
    for a, b in zip(cuts[:-1], cuts[1:]):
        solver.least_squares(gpu.CSRMatrix(C[a:b]), Xd[a:b], gram, Yd, 3)
    gpu.Profiler.enable(False)
    assert rel(Xd.to_numpy(), oracle_rows(Y0)) < TOL
    # Y rewritten in place through the library, gramian recomputed: the copy is remade
    Y1 = (Y0 * 0.5 + 0.03).astype(np.float32)
    Yd.copy_from_numpy(Y1)
    solver.calculate_yty(Yd, gram, 0.05)
    Xd = gpu.Matrix(X0)
    solver.least_squares(gpu.CSRMatrix(C), Xd, gram, Yd, 3)
    assert rel(Xd.to_numpy(), oracle_rows(Y1)) < TOL
    # Y rewritten, the caller's gramian NOT recomputed (a stale gramian is the caller's business -- the factors used must
    # still be the ones in Y now): same result as a fresh solver state given the same (Y, gramian) pair
    Y2 = (Y0 * 0.25 - 0.01).astype(np.float32)
    Yd.copy_from_numpy(Y2)
    Xa = gpu.Matrix(X0)
    solver.least_squares(gpu.CSRMatrix(C), Xa, gram, Yd, 3)
    fresh_Y, fresh_gram = gpu.Matrix(Y2), gpu.Matrix(gram.to_numpy())
    Xb = gpu.Matrix(X0)
    solver.least_squares(gpu.CSRMatrix(C), Xb, fresh_gram, fresh_Y, 3)
    np.testing.assert_array_equal(Xa.to_numpy(), Xb.to_numpy())
