"""The dense helper kernels at their edges, against the host restatements of tests/dense_reference.py: gramian
(csrc/gramian.hip), training loss (als_loss_kernel, csrc/solver.hip), row norms, casts, gather / scatter
(csrc/containers.hip) and RandomState (csrc/random.hip).

Most of it compares with ZERO tolerance: the library is built with -ffp-contract=off and the inputs are small integers
(or bit patterns that are only moved), so a dropped, doubled or mis-masked row, a misplaced tile or a wrong stride changes
an exactly known answer (tests/test_dense_host.py asserts the < 2^24 condition for every case).  The shapes were derived
from the launch formulas for the 256-CU device (quoted where the shapes are defined, dense_reference.py and below); the
geometry itself is not asserted -- on another CU count the same cases still check the same answers.
"""
import numpy as np
import pytest

import dense_reference as ref

pytestmark = pytest.mark.gpu

REG = 0.25
DTYPES = (np.float32, np.float16)


def _gramian(gpu, solver, yd, f, reg=REG):
    out = gpu.Matrix.zeros(f, f)
    solver.calculate_yty(yd, out, reg)
    return out.to_numpy()


def _check_exact(gpu, solver, y, tag=""):
    """fp32 and fp16 storage of the same integer matrix against the exact answer."""
    f = y.shape[1]
    want = ref.gramian_exact(y, REG)
    for dtype in DTYPES:
        got = _gramian(gpu, solver, gpu.Matrix(y.astype(dtype)), f)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (f"{tag} N={y.shape[0]} f={f} {np.dtype(dtype).name}: {len(bad)} wrong elements, first at "
                               f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}; G[0,0]={got[0, 0]!r}")


# ---- A. gramian, exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f, n", ref.vec_cases())
def test_gramian_vector_kernel_exact(gpu, f, n):
    """f = 64 / 128: every tail length of the 24-row trip and the 264-row chunk, N below one trip, the odd last row, and
    the reduce kernel's unrolled loop (131 chunks) and mixed groups (56 chunks)."""
    _check_exact(gpu, gpu.LeastSquaresSolver(), ref.int_factors(n, f), "vector")


@pytest.mark.parametrize("f, n", ref.generic_cases())
def test_gramian_generic_kernel_exact(gpu, f, n):
    """Every other f: tails of the 16-row trip and the 256-row chunk, column tails of the last 32-wide tile, grid.y > 1 with
    waves that own 3, 2, 1 and 0 tile pairs, more than 64 chunks."""
    _check_exact(gpu, gpu.LeastSquaresSolver(), ref.int_factors(n, f), "generic")


@pytest.mark.parametrize("f", [64, 128])
def test_gramian_reduce_ignores_stale_chunks(gpu, f):
    """131 chunks, then 56 on the same workspace: partial tiles 56..130 of the first call are still there, and a reduce
    that walks past its chunk count (or an unrolled loop entered one round too often) adds them."""
    solver = gpu.LeastSquaresSolver()
    _check_exact(gpu, solver, ref.int_factors(ref.VEC_ROWS_131_CHUNKS, f, seed=1), "first")
    _check_exact(gpu, solver, ref.int_factors(ref.VEC_ROWS_56_CHUNKS, f, seed=1), "second")
    _check_exact(gpu, solver, ref.int_factors(17 * 264 + 1, f, seed=1), "third")  # 18 chunks: groups 0, 1 take two, no unrolled round


@pytest.mark.parametrize("f, a, n", ref.VIEW_CASES)
def test_gramian_of_a_row_range_view(gpu, f, a, n):
    """Y_full[a : a + n] with odd a inside a parent whose other rows are NaN: a read past either end of the view that is not
    masked out shows as NaN."""
    y = ref.int_factors(n, f, seed=2)
    parent = np.full((a + n + ref.VIEW_PAD, f), np.nan, dtype=np.float32)
    parent[a:a + n] = y
    want = ref.gramian_exact(y, REG)
    solver = gpu.LeastSquaresSolver()
    for dtype in DTYPES:
        full = gpu.Matrix(parent.astype(dtype))
        got = _gramian(gpu, solver, full[a:a + n], f)
        assert np.array_equal(got, want), f"view [{a}:{a + n}] f={f} {np.dtype(dtype).name}: G[0,0]={got[0, 0]!r}, nan={np.isnan(got).sum()}"


@pytest.mark.parametrize("f", [64, 128, 100, 320])
def test_gramian_of_a_one_row_view(gpu, f):
    """Y_full[k]: the outer product of one row, its neighbours NaN."""
    parent = np.full((9, f), np.nan, dtype=np.float32)
    parent[5] = ref.int_factors(1, f, seed=3)[0]
    want = ref.gramian_exact(parent[5:6], REG)
    solver = gpu.LeastSquaresSolver()
    for dtype in DTYPES:
        got = _gramian(gpu, solver, gpu.Matrix(parent.astype(dtype))[5], f)
        assert np.array_equal(got, want), f"f={f} {np.dtype(dtype).name}"


def test_gramian_workspace_reuse(gpu):
    """The persistent split-K workspace across calls of one solver: large N, small N, a larger f (other tile layout), back
    to the vector layout, and the same input twice -- nothing stale, every answer exact."""
    solver = gpu.LeastSquaresSolver()
    for f, n in ((128, ref.VEC_ROWS_131_CHUNKS), (128, 7), (320, 300), (64, 529), (100, 3001), (128, 25), (128, 25)):
        _check_exact(gpu, solver, ref.int_factors(n, f, seed=4), "reuse")
    gpu.release_workspaces()  # and from a fresh workspace
    _check_exact(gpu, solver, ref.int_factors(49, 128, seed=4), "fresh")


# ---- B. gramian, real-valued, element by element -----------------------------------------------------------------------------
@pytest.mark.parametrize("f", [64, 100, 128, 320])
@pytest.mark.parametrize("profile", ref.REAL_PROFILES)
def test_gramian_real_valued_elementwise(gpu, profile, f):
    """Each element within (N + 1) 2^-24 (|Y|^T |Y|)_ij of the float64 product of the STORED values (fp16: after rounding) --
    the worst case of an N-term fp32 sum of products in any order, so a derived bar -- and bitwise symmetric.  reg = 0: the
    bar is that of the sum alone."""
    solver = gpu.LeastSquaresSolver()
    many = ref.VEC_ROWS_56_CHUNKS if f in (64, 128) else ref.GENERIC_ROWS_66_CHUNKS
    for n in (3001, many):
        y = ref.real_factors(profile, n, f)
        for dtype in DTYPES:
            stored = y.astype(dtype)
            want, bar = ref.gramian_f64_and_bound(stored)
            got = _gramian(gpu, solver, gpu.Matrix(stored), f, reg=0.0)
            err = np.abs(got.astype(np.float64) - want)
            ratio = float((err / bar).max())
            print(f"gramian {profile} f={f} N={n} {np.dtype(dtype).name}: worst error / bound = {ratio:.3e}")
            assert np.isfinite(got).all() and (err <= bar).all(), f"worst error / bound {ratio:.3e} at {np.unravel_index((err / bar).argmax(), err.shape)}"
            assert np.array_equal(got, got.T)


# ---- C. loss, exact ----------------------------------------------------------------------------------------------------------
def _gpu_loss(gpu, c, x, y, reg=ref.LOSS_REG):
    return np.float32(gpu.LeastSquaresSolver().calculate_loss(gpu.CSRMatrix(c), gpu.Matrix(x), gpu.Matrix(y), reg))


@pytest.mark.parametrize("f", ref.LOSS_F)
def test_loss_exact(gpu, f):
    """Every values-per-lane template (ceil(f / 64) in 1, 2, 3, 4, 5..8, 9..12, 13..16) from both sides of its cut; an empty
    user row and an all-negative one.  All fp32 intermediates are small integers, the fp64 atomics exact in any order."""
    c, x, y = ref.loss_problem(ref.LOSS_USERS, ref.LOSS_ITEMS, f)
    got, want = _gpu_loss(gpu, c, x, y), ref.loss_ref(c, x, y, ref.LOSS_REG)
    assert got == want, f"f={f}: got {got!r}, want {want!r}"
    assert _gpu_loss(gpu, c, x, y, 0.0) == ref.loss_ref(c, x, y, 0.0)


def test_loss_exact_grid_stride(gpu):
    """8192 + 37 users at f = 64: one wavefront per user, min(ceil(users / 4), 8 CUs) blocks of 4 -- at most 8192 wavefronts on
    256 CUs, so 37 users are a wavefront's second row."""
    c, x, y = ref.loss_problem(ref.LOSS_STRIDE_USERS, ref.LOSS_ITEMS, 64)
    got, want = _gpu_loss(gpu, c, x, y), ref.loss_ref(c, x, y, ref.LOSS_REG)
    assert got == want, f"got {got!r}, want {want!r}"


def test_loss_exact_half_storage(gpu):
    """fp16 X and Y (the values are exact in fp16): the same number."""
    c, x, y = ref.loss_problem(ref.LOSS_USERS, ref.LOSS_ITEMS, 129)
    got = _gpu_loss(gpu, c, x.astype(np.float16), y.astype(np.float16))
    assert got == ref.loss_ref(c, x, y, ref.LOSS_REG)


# ---- D. row norms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", ref.NORM_COLS)
def test_row_norms_exact(gpu, cols):
    """8192 + 5 rows (one wavefront per row, 8192 wavefronts on 256 CUs: the last five are second rounds), column tails of
    the 64-lane stride, all-zero rows -> 1e-10.  The sum of squares is exact, so the only rounding is sqrtf's, and HIP's fp32
    square root is correctly rounded by default: measured 0 ulp from numpy's correctly rounded fp32 sqrt of the exact sum in
    every case on the MI355X, so the comparison is bit for bit."""
    m = ref.norm_rows(cols)
    want = ref.norms_ref(m)
    for dtype in DTYPES:
        got = gpu.calculate_norms(gpu.Matrix(m.astype(dtype))).to_numpy()
        assert got.shape == (1, ref.NORM_ROWS)
        ulps = ref.ulp_distance(got[0], want)
        print(f"row_norms cols={cols} {np.dtype(dtype).name}: worst distance {int(ulps.max())} ulp")
        assert np.array_equal(got[0], want), f"cols={cols} {np.dtype(dtype).name}: worst distance {int(ulps.max())} ulp at row {int(ulps.argmax())}"


# ---- E. casts, gather, scatter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, 9])
def test_cast_half_to_float_every_bit_pattern(gpu, copies):
    """All 65 536 fp16 patterns (subnormals, infinities, NaNs); 9 copies = 589 824 elements, past the 8 x 256 CUs x 256
    threads of one grid round."""
    h = np.tile(ref.all_half_bits(), (copies, 1))
    got = gpu.Matrix(h).astype(np.float32).to_numpy()
    assert got.dtype == np.float32 and ref.same_bits_or_nan(got, h.astype(np.float32))


@pytest.mark.parametrize("copies, cols", [(1, 1), (1, 67), (3, 129)])
def test_cast_float_to_half_rounds_to_nearest_even(gpu, copies, cols):
    """Every finite half, every tie between two halves and its fp32 neighbours, the steps to inf and to zero, fp32 subnormals,
    signed zeros, infinities, NaN: bit-equal to numpy's round-to-nearest-even.  3 copies = 761 958 elements, past one grid
    round; the matrix is padded with zeros to whole rows."""
    v = np.tile(ref.half_rounding_inputs(), copies)
    v = np.concatenate([v, np.zeros(-len(v) % cols, dtype=np.float32)]).reshape(-1, cols)
    with np.errstate(over="ignore"):
        want = v.astype(np.float16)
    got = gpu.Matrix(v).astype(np.float16).to_numpy()
    assert got.dtype == np.float16
    if not ref.same_bits_or_nan(got, want):
        bad = np.argwhere(got.view(np.uint16) != want.view(np.uint16))
        i = tuple(bad[0])
        raise AssertionError(f"{len(bad)} values differ (NaNs included); first: {v[i]!r} -> {got[i]!r}, want {want[i]!r}")


@pytest.mark.parametrize("cols", [1, 5, 64, 129])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_rows_bits(gpu, dtype, cols):
    """600 000+ output elements (the stride loop starts past 524 288 on 256 CUs), reversed and repeated ids, bit patterns moved
    untouched; then the same from a row-range view."""
    out_rows = -(-600_000 // cols) + 3
    src_rows = out_rows // 2 + 5
    src = ref.random_bits((src_rows, cols), dtype, seed=5)
    rng = np.random.default_rng(cols)
    ids = np.concatenate([np.arange(src_rows - 1, -1, -1), rng.integers(0, src_rows, out_rows - src_rows)]).astype(np.int32)
    u = src.view(np.uint16 if dtype is np.float16 else np.uint32)
    full = gpu.Matrix(src)
    got = full[ids].to_numpy()
    assert got.dtype == np.dtype(dtype) and np.array_equal(got.view(u.dtype), u[ids])
    a, b = 3, src_rows - 4
    view_ids = (ids[:1000 + cols] % (b - a)).astype(np.int32)
    got = full[a:b][view_ids].to_numpy()
    assert np.array_equal(got.view(u.dtype), u[a:b][view_ids])


@pytest.mark.parametrize("cols", [1, 5, 64, 129])
@pytest.mark.parametrize("dtype", DTYPES)
def test_scatter_rows_bits(gpu, dtype, cols):
    """600 000+ scattered elements to a permutation of all but 7 rows (no id twice: the write order is unspecified); the other
    rows keep their bits.  Then a scatter through a row-range view lands in the parent at the view's offset."""
    rows = -(-600_000 // cols) + 3
    udt = np.uint16 if dtype is np.float16 else np.uint32
    dst = ref.random_bits((rows + 7, cols), dtype, seed=6)
    new = ref.random_bits((rows, cols), dtype, seed=7)
    ids = np.random.default_rng(cols).permutation(rows + 7)[:rows].astype(np.int32)
    want = dst.view(udt).copy()
    want[ids] = new.view(udt)
    d = gpu.Matrix(dst)
    d.assign_rows(ids, gpu.Matrix(new))
    assert np.array_equal(d.to_numpy().view(udt), want)
    a, b = 5, 5 + 300
    view_ids = np.random.default_rng(cols + 1).permutation(b - a)[:200].astype(np.int32)
    d[a:b].assign_rows(view_ids, gpu.Matrix(new[:200]))
    want[a + view_ids] = new.view(udt)[:200]
    assert np.array_equal(d.to_numpy().view(udt), want)


# ---- F. RandomState, bit for bit -------------------------------------------------------------------------------------------------
SEEDS = [42, 2 ** 32 + 7, -1]
BIG = (1001, 2099)  # 2 101 099 elements: past the 4 x 8 x 256 CUs x 256 threads one grid round covers, n % 4 == 3, odd columns


@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_bit_for_bit(gpu, seed):
    """Counter (q_lo, q_hi, draw, 0), key (seed_lo, seed_hi), four words per quad in order, the n % 4 tail; fp32
    low + (high - low) * u with every operation rounded."""
    for n in (1, 2, 3, 4, 5, 7, 64 * 3 + 1):
        for low, high in ((0.0, 1.0), (-0.3, 0.9)):
            got = gpu.RandomState(seed).uniform(1, n, low, high).to_numpy()
            assert np.array_equal(got[0], ref.uniform_ref(seed, 0, n, low, high)), f"seed={seed} n={n} [{low}, {high})"


def test_uniform_bit_for_bit_past_one_grid_round(gpu):
    got = gpu.RandomState(42).uniform(*BIG, -0.5, 0.5).to_numpy()
    want = ref.uniform_ref(42, 0, BIG[0] * BIG[1], -0.5, 0.5).reshape(BIG)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first at {tuple(bad[0])}"


def test_uniform_is_independent_of_the_shape(gpu):
    """Element i of a draw is a function of (seed, draw, i) only: three factorisations of n = 3003."""
    want = ref.uniform_ref(7, 0, 3003)
    for shape in ((1, 3003), (39, 77), (273, 11)):
        assert np.array_equal(gpu.RandomState(7).uniform(*shape).to_numpy().ravel(), want), shape


@pytest.mark.parametrize("seed", SEEDS)
def test_draw_counter_is_shared_by_both_methods(gpu, seed):
    """uniform, randn, uniform on one handle are draws 0, 1, 2; a second handle starts again at 0."""
    rs = gpu.RandomState(seed)
    first = rs.uniform(3, 5).to_numpy()
    second = rs.randn(2, 7).to_numpy()
    third = rs.uniform(5, 9, -1.0, 1.0).to_numpy()
    assert np.array_equal(first.ravel(), ref.uniform_ref(seed, 0, 15))
    assert np.abs(second.ravel() - ref.randn_ref(seed, 1, 14)).max() <= 1e-5
    assert np.array_equal(third.ravel(), ref.uniform_ref(seed, 2, 45, -1.0, 1.0))
    assert np.array_equal(gpu.RandomState(seed).uniform(3, 5).to_numpy(), first)


@pytest.mark.parametrize("seed, shape, stddev", [(42, BIG, 1.0), (2 ** 32 + 7, (1001, 499), 0.01), (-1, (1, 5), 1.0)])
def test_randn_against_float64_box_muller(gpu, seed, shape, stddev):
    """Within stddev * 1e-5 (absolute) of the float64 Box-Muller of the same u values.  The budget: 1 ulp of logf, halved
    through the square root; 2 ulp of sinf / cosf; the fp32 rounding of the angle 2 pi u (up to 4.8e-7) times a radius of at
    most 5.9 -- about 3e-6 together, and the bar is three times that."""
    got = gpu.RandomState(seed).randn(*shape, 0.0, stddev).to_numpy()
    want = ref.randn_ref(seed, 0, shape[0] * shape[1], 0.0, stddev).reshape(shape)
    err = np.abs(got.astype(np.float64) - want)
    print(f"randn seed={seed} n={got.size} stddev={stddev}: worst error {err.max():.3e} (bar {stddev * 1e-5:.1e})")
    assert np.isfinite(got).all() and err.max() <= stddev * 1e-5, f"worst error {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def test_unit_draws(gpu):
    """u01 is (0, 1]: where the word's top 24 bits are set, uniform() returns exactly `high`, and randn() a pair with zero
    radius -- finite, and zero."""
    seed, at, _ = ref.UNIT_UNIFORM
    for low, high in ((0.0, 1.0), (-0.5, 0.5)):
        got = gpu.RandomState(seed).uniform(200, 200, low, high).to_numpy().ravel()
        assert got[at] == np.float32(high) and got.max() == np.float32(high) and got.min() > np.float32(low)
    seed, at, _ = ref.UNIT_NORMAL
    got = gpu.RandomState(seed).randn(1, at + 2).to_numpy().ravel()
    assert np.isfinite(got).all() and got[at] == 0.0 and got[at + 1] == 0.0
    assert got[at - 1] != 0.0 and np.abs(got - ref.randn_ref(seed, 0, at + 2)).max() <= 1e-5
