"""Host restatements (numpy only) of the dense helper kernels, for tests/test_dense_host.py and tests/test_gpu_dense.py:
the gramian (csrc/gramian.hip), the training loss (als_loss_kernel, csrc/solver.hip), row norms, casts, gather / scatter
(csrc/containers.hip) and RandomState (csrc/random.hip).

Exact cases.  The library is built with -ffp-contract=off, and the inputs below are small integers: every fp32 partial
sum of the gramian, the loss and the squared norms is then an integer below 2^24, whatever the order of summation, so
the device's answer is known to the last bit and the tests compare with zero tolerance.  max_abs_partial /
loss_max_intermediate give the bound that makes this legitimate; the CPU suite asserts it for every case listed here.

The case lists live here so that the CPU suite checks the very inputs the GPU suite runs.
"""
import numpy as np

from bpr_reference import philox4x32_10

EXACT_LIMIT = 1 << 24  # integers up to here are exact in fp32

# ---- gramian: shapes --------------------------------------------------------------------------------------------------
# f = 64 / 128 ride the vector kernel: 24-row trips, chunks of max(256, ceil(N / (4 CUs))) rows rounded up to whole trips
# = 264 rows while N <= 264 * 1024 on 256 CUs.  Tails of every length class around one, two and three 8-row buffers, one
# and two trips, one and two chunks:
VEC_ROWS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 47, 48, 49, 263, 264, 265, 287, 288, 289, 527, 528, 529]
# the reduce kernel gives chunks g, g + 16, ... to group g, four at a time while c + 48 < chunks:
VEC_ROWS_131_CHUNKS = 130 * 264 + 5  # 131 chunks: the unrolled loop runs twice for groups 0..2, once + remainder for the rest
VEC_ROWS_56_CHUNKS = 55 * 264 + 11   # 56 chunks: groups 0..7 enter the unrolled loop, groups 8..15 do not
# every other f rides the generic kernel: 16-row trips, 256-row chunks while N <= 256 * (1024 / grid.y);
# grid.y = ceil(pairs / 12) with pairs = t (t + 1) / 2, t = ceil(f / 32): 5 at f = 320, 6 at f = 352, 44 at f = 1024.
# The last grid.y slice leaves waves with 0 pairs at f = 129 / 160 (15 pairs), 2 and 1 at f = 320 (55) and f = 352 (66).
GENERIC_F = [1, 6, 31, 32, 33, 96, 100, 129, 160, 161, 192, 256, 257, 320, 352, 1024]
GENERIC_ROWS = [1, 2, 15, 16, 17, 255, 256, 257, 3001]
GENERIC_ROWS_66_CHUNKS = 65 * 256 + 3  # more than 64 chunks: the reduce's unrolled loop and its remainder
GENERIC_ROWS_EVERY_F = (17, 257)


def generic_cases():
    """(f, N): every f at two N, every N (and the many-chunk one) at f = 100 and f = 320."""
    cases = [(f, n) for f in GENERIC_F for n in GENERIC_ROWS_EVERY_F]
    cases += [(f, n) for f in (100, 320) for n in GENERIC_ROWS + [GENERIC_ROWS_66_CHUNKS] if n not in GENERIC_ROWS_EVERY_F]
    return cases


def vec_cases():
    return [(f, n) for f in (64, 128) for n in VEC_ROWS + [VEC_ROWS_56_CHUNKS, VEC_ROWS_131_CHUNKS]]


# (f, first row (odd), rows) of the row-range views: tails of the trip on both kernels, inside a NaN-filled parent
VIEW_CASES = [(f, a, n) for f in (64, 128) for a, n in ((1, 1), (3, 7), (5, 23), (7, 25), (1, 49), (9, 265), (3, 529))]
VIEW_CASES += [(f, a, n) for f in (100, 320) for a, n in ((1, 1), (3, 15), (5, 17), (7, 257))]
VIEW_PAD = 11  # NaN rows after the view: it lies strictly inside the allocation


# ---- gramian: inputs and answers -----------------------------------------------------------------------------------------
def int_factors(n, f, seed=0):
    """n x f fp32 with integer entries in [-3, 3] and column 0 == 1: G[0, 0] counts the rows, no row is zero."""
    rng = np.random.default_rng([int(seed), int(n), int(f)])
    y = rng.integers(-3, 4, size=(n, f)).astype(np.float32)
    y[:, 0] = 1.0
    return y


def gramian_exact(y, reg):
    """fp32 Y^T Y + reg I of an integer-valued Y, exact.  The product is taken in float64 (BLAS): its terms and sums are
    integers far below 2^53, so it equals the int64 product (checked in the CPU suite) whatever order BLAS uses."""
    y64 = np.asarray(y, dtype=np.float64)
    g = y64.T @ y64
    assert np.array_equal(g, np.rint(g))
    g[np.diag_indices_from(g)] += float(reg)
    out = g.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), g), "the expected gramian is not representable in fp32"
    return out


def max_abs_partial(y):
    """max_ij sum_r |y_ri| |y_rj|: no partial sum of (Y^T Y)_ij, in any order, exceeds it."""
    a = np.abs(np.asarray(y, dtype=np.float64))
    return float((a.T @ a).max())


REAL_PROFILES = ("cold_start", "mean_zero", "mixed_scales")


def real_factors(profile, n, f, seed=0):
    """The three magnitude profiles of the element-wise gramian check, fp32."""
    rng = np.random.default_rng([int(seed), int(n), int(f), REAL_PROFILES.index(profile)])
    if profile == "cold_start":  # what a model's first sweep sees: all-positive 0.01 U(0, 1)
        return (0.01 * rng.random((n, f))).astype(np.float32)
    if profile == "mean_zero":  # cancellation: the sums are far smaller than their terms
        return rng.standard_normal((n, f)).astype(np.float32)
    scale = np.logspace(-3, 2, f)[rng.permutation(f)]  # column scales from 1e-3 to 1e+2
    return (rng.standard_normal((n, f)) * scale).astype(np.float32)


def gramian_f64_and_bound(y):
    """(Y^T Y in float64, per-element bar) for stored values y (fp32, or fp16 after rounding).  The bar is the standard
    worst case of an N-term fp32 sum of products taken in any order: (N + 1) 2^-24 (|Y|^T |Y|)_ij."""
    y64 = np.asarray(y, dtype=np.float64)
    a = np.abs(y64)
    return y64.T @ y64, (y64.shape[0] + 1) * 2.0 ** -24 * (a.T @ a)


# ---- loss ---------------------------------------------------------------------------------------------------------------
# one VPL (values per lane, ceil(f / 64)) template per case of the dispatch: 1, 2, 3, 4, 5..8, 9..12, 13..16 -- both sides
# of every cut
LOSS_F = [1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 768, 769, 1024]
LOSS_USERS, LOSS_ITEMS = 50, 40
LOSS_STRIDE_USERS = 8192 + 37  # one wavefront per user, at most 8 * 256 CUs * 4 wavefronts: 37 users are second rounds
LOSS_REG = 0.5


def loss_problem(users, items, f, seed=0):
    """(C, X, Y): X / Y fp32 with entries in {-1, 0, 1} at ~10 % density, C a scipy CSR (users x items) with integer
    confidences in [-4, 8] \\ {0} at ~25 % density.  User 1 has no entries, user 2 only negative ones (where there are
    that many users); the last factor is set in X[0], Y[0] and C[0, 0] so that every case reaches column f - 1."""
    import scipy.sparse as sp

    rng = np.random.default_rng([int(seed), int(users), int(items), int(f)])

    def ternary(shape):
        return (rng.integers(-1, 2, size=shape) * (rng.random(shape) < 0.15)).astype(np.float32)

    x, y = ternary((users, f)), ternary((items, f))
    x[0, f - 1], y[0, f - 1] = 1.0, -1.0
    conf = rng.integers(-4, 8, size=(users, items))
    conf[conf >= 0] += 1  # [-4, -1] and [1, 8]
    conf = conf * (rng.random((users, items)) < 0.25)
    conf[0, 0] = 3
    if users > 2:
        conf[1, :] = 0
        conf[2, :] = -((np.abs(conf[2, :]) + 3) % 4 + 1) * (conf[2, :] != 0)  # [-4, -1] where there is an entry
        conf[2, 1] = -2
    c = sp.csr_matrix(conf.astype(np.float32))
    c.eliminate_zeros()
    c.sort_indices()
    return c, x, y


def _loss_terms(c, x, y):
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    rows = np.repeat(np.arange(c.shape[0]), np.diff(c.indptr))
    conf = c.data.astype(np.float64)
    yk, xk = y64[c.indices], x64[rows]
    d = np.einsum("kf,kf->k", yk, xk)                                   # y . x per stored entry
    a = np.abs(conf)
    w = np.where(conf > 0, -2.0 * conf, 0.0) + (a - 1.0) * d
    return x64, y64, rows, yk, xk, d, a, w


def loss_ref(c, x, y, reg):
    """float64 restatement of calculate_loss (solver.hip): per user r = YtY x + sum_k ((c > 0 ? -2c : 0) + (|c| - 1) y.x) y,
    loss = sum_u (r . x + sum |c|) + reg (|X|^2 + |Y|^2), over sum |c| + users * items - nnz; rounded to fp32 once."""
    x64, y64, _, _, _, d, a, w = _loss_terms(c, x, y)
    g = y64.T @ y64
    loss = np.einsum("uf,fg,ug->", x64, g, x64) + (w * d).sum() + a.sum()
    loss += float(reg) * ((y64 * y64).sum() + (x64 * x64).sum())
    denom = a.sum() + float(c.shape[0]) * float(c.shape[1]) - float(c.nnz)
    return np.float32(loss / denom)


def loss_max_intermediate(c, x, y):
    """An upper bound on the magnitude of every fp32 intermediate of als_loss_kernel on this input (sums of absolute
    values: it holds for any order of the lanes' and the wavefront's partial sums)."""
    x64, y64, rows, yk, xk, d, a, w = _loss_terms(c, x, y)
    ax, ay = np.abs(x64), np.abs(y64)
    g_abs = ay.T @ ay                                   # bounds the gramian's partial sums
    r_abs = ax @ g_abs                                  # bounds YtY x
    d_abs = np.einsum("kf,kf->k", np.abs(yk), np.abs(xk))
    w_abs = 2.0 * a + np.abs(a - 1.0) * d_abs
    np.add.at(r_abs, rows, w_abs[:, None] * np.abs(yk))  # ... + sum |w| |y|
    rx_abs = (r_abs * ax).sum(axis=1)                   # bounds r . x
    return float(max(g_abs.max(), r_abs.max(), d_abs.max(initial=0.0), w_abs.max(initial=0.0), rx_abs.max(),
                     (ax * ax).sum(axis=1).max()))


# ---- row norms ------------------------------------------------------------------------------------------------------------
NORM_ROWS = 8192 + 5  # one wavefront per row, 8 * 256 CUs * 4 wavefronts: five rows are second rounds
NORM_COLS = [1, 63, 64, 65, 200]
NORM_ZERO_ROWS = (0, 77, 8192, 8196)


def norm_rows(cols, seed=0):
    """NORM_ROWS x cols integers in [-3, 3] (fp32; exact in fp16 as well) with a few all-zero rows."""
    rng = np.random.default_rng([int(seed), int(cols)])
    m = rng.integers(-3, 4, size=(NORM_ROWS, cols)).astype(np.float32)
    m[list(NORM_ZERO_ROWS)] = 0.0
    return m


def norms_ref(m):
    """fp32 row norms of an integer matrix: the exact sum of squares, one correctly rounded square root, 0 -> 1e-10."""
    s = (np.asarray(m, dtype=np.float64) ** 2).sum(axis=1)
    n = np.sqrt(s.astype(np.float32))  # s < 2^24 is exact in fp32; numpy's fp32 sqrt is correctly rounded
    return np.where(n == 0, np.float32(1e-10), n).astype(np.float32)


def ulp_distance(a, b):
    """Distance in units in the last place between two finite fp32 arrays."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- casts ----------------------------------------------------------------------------------------------------------------
def all_half_bits():
    """Every fp16 bit pattern as a 256 x 256 fp16 matrix."""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(256, 256)


def half_midpoint_table():
    """For every finite non-negative half h (bit patterns 0 .. 0x7BFF): (h, next, mid) as fp32, where next is the half
    above h (65536 = 2^16 above 65504, the value past which fp16 rounds to inf) and mid = (h + next) / 2, which fp32
    holds exactly (one more significand bit than fp16)."""
    bits = np.arange(0x7C00, dtype=np.uint16)
    h = bits.view(np.float16).astype(np.float64)
    nxt = np.empty_like(h)
    nxt[:-1] = h[1:]
    nxt[-1] = 65536.0
    mid = (h + nxt) / 2
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
    return h.astype(np.float32), nxt.astype(np.float32), mid.astype(np.float32)


def half_rounding_inputs():
    """fp32 values that pin round-to-nearest-even of fp32 -> fp16: every finite half, the midpoint to the next half (a tie)
    and the fp32 neighbours of that midpoint on either side, in both signs -- this covers the half subnormals, the step to
    inf (65504 / 65520) and the step to zero (2^-25) -- plus values below 2^-25, fp32 subnormals, zeros, infinities and NaN."""
    h, _, mid = half_midpoint_table()
    below = np.nextafter(mid, np.float32(0), dtype=np.float32)
    above = np.nextafter(mid, np.float32(np.inf), dtype=np.float32)
    pos = np.concatenate([h, mid, below, above])
    extra = np.array([0.0, 2.0 ** -25, 2.0 ** -26, 2.0 ** -30, 1e-10, 1e-38, 1e-40, 1.4e-45, 65504.0, 65519.996, 65520.0,
                      65520.004, 65536.0, 1e5, 3.4e38, np.inf], dtype=np.float32)
    nan = np.array([np.nan], dtype=np.float32)
    return np.concatenate([pos, -pos, extra, -extra, nan, -nan]).astype(np.float32)


def same_bits_or_nan(got, want):
    """Bit equality of two float arrays of one dtype, NaNs compared by isnan."""
    u = {2: np.uint16, 4: np.uint32}[want.dtype.itemsize]
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))


def random_bits(shape, dtype, seed=0):
    """Finite-or-not bit patterns of `dtype`: gather / scatter move them untouched, compared as integers."""
    u = {2: np.uint16, 4: np.uint32}[np.dtype(dtype).itemsize]
    rng = np.random.default_rng([int(seed), *[int(s) for s in shape]])
    return rng.integers(0, np.iinfo(u).max, size=shape, dtype=u, endpoint=True).view(dtype)


# ---- RandomState ------------------------------------------------------------------------------------------------------------
TAG_UNIFORM, TAG_NORMAL = 0, 1


def rng_words(seed, draw, n, tag):
    """The n 32-bit words of call number `draw` of a handle: quad q = Philox4x32-10(counter (q_lo, q_hi, draw, tag),
    key (seed_lo, seed_hi)), its four words in order."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF  # the int64 seed's two's complement
    q = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    r = philox4x32_10(q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), int(draw), int(tag), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(r, axis=1).reshape(-1)[:int(n)]


def u01_ref(words):
    """fp32 ((x >> 8) + 0.5) / 2^24, each operation rounded: in (0, 1] -- from 2^23 on the sum is a tie that goes to the even
    neighbour, and 16777215.5 goes to 2^24, i.e. 1.0."""
    k = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def uniform_ref(seed, draw, n, low=0.0, high=1.0):
    """RandomState.uniform bit for bit: low + (high - low) * u, fp32, no contraction."""
    lo, hi = np.float32(low), np.float32(high)
    v = u01_ref(rng_words(seed, draw, n, TAG_UNIFORM))
    return (lo + (hi - lo) * v).astype(np.float32)


def randn_ref(seed, draw, n, mean=0.0, stddev=1.0):
    """RandomState.randn in float64 from the device's fp32 u values: Box-Muller, words (0, 1) and (2, 3) of a quad give
    (m cos, m sin) with m = sqrt(-2 ln u_even), angle 2 pi u_odd."""
    quads = (int(n) + 3) // 4
    u = u01_ref(rng_words(seed, draw, 4 * quads, TAG_NORMAL)).astype(np.float64).reshape(quads, 2, 2)
    m = np.sqrt(-2.0 * np.log(u[:, :, 0]))
    ang = 2.0 * np.pi * u[:, :, 1]
    v = np.stack([m * np.cos(ang), m * np.sin(ang)], axis=2).reshape(-1)[:int(n)]
    return float(mean) + float(stddev) * v


def find_unit_word(tag, positions, seeds=range(4096), quads=65536):
    """First (seed, element index, word) of a first draw (draw 0) whose word has its top 24 bits set -- u01 is exactly 1.0
    there -- at an element index with index % 4 in `positions`; 65536 quads per seed."""
    for seed in seeds:
        w = rng_words(seed, 0, 4 * quads, tag)
        hit = np.nonzero((w >> np.uint32(8)) == np.uint32(0xFFFFFF))[0]
        hit = [int(i) for i in hit if i % 4 in positions]
        if hit:
            return seed, hit[0], int(w[hit[0]])
    return None


# pinned by the CPU suite (found with find_unit_word):
UNIT_UNIFORM = (207, 39758, 0xFFFFFFA2)  # seed, element, word: uniform() returns exactly `high` there
UNIT_NORMAL = (876, 111410, 0xFFFFFF3F)   # element % 4 == 2: the radius of elements 111410 / 111411 is sqrt(-2 ln 1) = 0
