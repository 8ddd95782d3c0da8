"""CPU-side checks of tests/dense_reference.py: the host restatements the GPU suite (tests/test_gpu_dense.py) compares the
dense helper kernels with, and the condition under which that suite may compare with zero tolerance -- every fp32
intermediate of every exact-integer case stays below 2^24."""
import numpy as np
import pytest

import dense_reference as ref
from bpr_reference import philox4x32_10


# ---- gramian ---------------------------------------------------------------------------------------------------------------
def test_gramian_exact_equals_the_int64_product():
    y = ref.int_factors(1000, 33)
    want = y.astype(np.int64).T @ y.astype(np.int64)
    got = ref.gramian_exact(y, 0.25)
    assert np.array_equal(got.astype(np.float64), want + 0.25 * np.eye(33))
    assert got[0, 0] == 1000.25  # column 0 is all ones: the corner counts the rows
    assert np.abs(y).sum(axis=1).min() >= 1 and np.abs(y).max() == 3 and np.array_equal(y, np.rint(y))


def test_case_lists_cover_what_they_claim():
    vec, gen = ref.vec_cases(), ref.generic_cases()
    assert {f for f, _ in vec} == {64, 128} and {f for f, _ in gen} == set(ref.GENERIC_F)
    for f in ref.GENERIC_F:
        assert len({n for g, n in gen if g == f}) >= 2
    for f in (100, 320):
        assert {n for g, n in gen if g == f} == set(ref.GENERIC_ROWS) | {ref.GENERIC_ROWS_66_CHUNKS}
    assert len(set(vec)) == len(vec) and len(set(gen)) == len(gen)
    # chunk counts on the 256-CU device (gramian_t: 264-row chunks on the vector path, 256-row chunks on the generic one)
    assert -(-ref.VEC_ROWS_131_CHUNKS // 264) == 131 and 49 <= -(-ref.VEC_ROWS_56_CHUNKS // 264) <= 63
    assert -(-ref.GENERIC_ROWS_66_CHUNKS // 256) > 64
    assert ref.VEC_ROWS_131_CHUNKS * 128 * 4 <= 18 * 2 ** 20  # the largest input
    for f, a, n in ref.VIEW_CASES:
        assert a % 2 == 1 and n in ref.VEC_ROWS + ref.GENERIC_ROWS


@pytest.mark.parametrize("f, n", [(128, ref.VEC_ROWS_131_CHUNKS), (64, ref.VEC_ROWS_131_CHUNKS), (128, ref.VEC_ROWS_56_CHUNKS),
                                  (320, ref.GENERIC_ROWS_66_CHUNKS), (100, ref.GENERIC_ROWS_66_CHUNKS), (1024, 257), (320, 3001)])
def test_gramian_partial_sums_stay_exact(f, n):
    """The largest N of every f class: sum_r |y_ri| |y_rj| < 2^24 (the other cases are row prefixes in size: 9 N bounds all)."""
    assert ref.max_abs_partial(ref.int_factors(n, f)) < ref.EXACT_LIMIT
    assert 9 * max(n for _, n in ref.vec_cases() + ref.generic_cases()) < ref.EXACT_LIMIT


def test_gramian_bound_is_the_n_term_bound():
    y = ref.real_factors("mean_zero", 300, 5)
    g, bar = ref.gramian_f64_and_bound(y)
    y64 = y.astype(np.float64)
    assert np.allclose(g, y64.T @ y64, rtol=1e-15)
    assert np.allclose(bar, 301 * 2.0 ** -24 * (np.abs(y64).T @ np.abs(y64)), rtol=1e-15)
    # a plain fp32 accumulation in row order obeys it
    acc = np.zeros((5, 5), dtype=np.float32)
    for row in y:
        acc += np.outer(row, row)
    assert (np.abs(acc - g) <= bar).all()


def test_profiles_are_what_they_say():
    cold = ref.real_factors("cold_start", 500, 64)
    assert cold.dtype == np.float32 and cold.min() >= 0 and cold.max() <= 0.01
    assert abs(ref.real_factors("mean_zero", 4000, 64).mean()) < 0.01
    mixed = np.abs(ref.real_factors("mixed_scales", 2000, 100)).mean(axis=0)
    assert mixed.max() / mixed.min() > 1e4
    assert np.isfinite(ref.real_factors("mixed_scales", 100, 320).astype(np.float16)).all()


# ---- loss ------------------------------------------------------------------------------------------------------------------
def _loss_by_rows(c, x, y, reg):
    """The kernel's loop, user by user and entry by entry, in float64."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    g = y.T @ y
    loss = conf_sum = norm = 0.0
    for u in range(c.shape[0]):
        r = g @ x[u]
        for k in range(c.indptr[u], c.indptr[u + 1]):
            conf, yk = float(c.data[k]), y[c.indices[k]]
            t = -2.0 * conf if conf > 0 else 0.0
            r = r + (t + (abs(conf) - 1.0) * (yk @ x[u])) * yk
            conf_sum += abs(conf)
        loss += r @ x[u]
        norm += x[u] @ x[u]
    total = loss + conf_sum + reg * ((y * y).sum() + norm)
    return np.float32(total / (conf_sum + c.shape[0] * c.shape[1] - c.nnz))


def test_loss_ref_matches_the_row_loop_and_known_answers():
    import scipy.sparse as sp

    c, x, y = ref.loss_problem(ref.LOSS_USERS, ref.LOSS_ITEMS, 65)
    assert ref.loss_ref(c, x, y, ref.LOSS_REG) == _loss_by_rows(c, x, y, ref.LOSS_REG)
    # the reference's own known answers (its tests/als_test.py): 1.0 and 2.0
    ratings = sp.coo_matrix(([1.0], ([0], [0])), shape=(1, 2)).tocsr().astype(np.float32)
    items, users = np.array([[0.0], [1.0]], dtype=np.float32), np.array([[1.0]], dtype=np.float32)
    assert ref.loss_ref(ratings, users, items, 0.0) == 1.0 and ref.loss_ref(ratings, users, items, 1.0) == 2.0


def test_loss_problem_has_the_rows_it_promises():
    c, x, y = ref.loss_problem(ref.LOSS_USERS, ref.LOSS_ITEMS, 257)
    lengths = np.diff(c.indptr)
    assert lengths[1] == 0 and lengths[2] > 0 and (c.data[c.indptr[2]:c.indptr[3]] < 0).all()
    assert set(np.unique(c.data)) <= set(range(-4, 0)) | set(range(1, 9)) and c.data.min() < 0 < c.data.max()
    assert set(np.unique(x)) == {-1.0, 0.0, 1.0} and 0.05 < (x != 0).mean() < 0.15
    assert x[0, 256] != 0 and y[0, 256] != 0 and c[0, 0] != 0  # the last factor takes part


@pytest.mark.parametrize("users, f", [(ref.LOSS_USERS, f) for f in ref.LOSS_F] + [(ref.LOSS_STRIDE_USERS, 64)])
def test_loss_intermediates_stay_exact(users, f):
    c, x, y = ref.loss_problem(users, ref.LOSS_ITEMS, f)
    assert ref.loss_max_intermediate(c, x, y) < ref.EXACT_LIMIT
    # the three fp64 totals are sums of such integers: exact in any order as long as they stay below 2^53
    assert users * ref.loss_max_intermediate(c, x, y) < 2 ** 53


# ---- row norms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", ref.NORM_COLS)
def test_norm_inputs_are_exact_in_both_dtypes(cols):
    m = ref.norm_rows(cols)
    assert m.shape == (ref.NORM_ROWS, cols) and np.array_equal(m.astype(np.float16).astype(np.float32), m)
    assert (m.astype(np.float64) ** 2).sum(axis=1).max() < ref.EXACT_LIMIT
    n = ref.norms_ref(m)
    assert (n[list(ref.NORM_ZERO_ROWS)] == np.float32(1e-10)).all() and (n > 0).all()
    assert np.allclose(n[5], np.linalg.norm(m[5].astype(np.float64)), rtol=1e-7)


def test_ulp_distance():
    a = np.array([1.0, -1.0, 0.0, 1e-10], dtype=np.float32)
    assert np.array_equal(ref.ulp_distance(a, a), [0, 0, 0, 0])
    assert np.array_equal(ref.ulp_distance(a, np.nextafter(a, np.float32(np.inf), dtype=np.float32)), [1, 1, 1, 1])
    assert ref.ulp_distance(np.float32([-0.0]), np.float32([0.0]))[0] == 0


# ---- casts -------------------------------------------------------------------------------------------------------------------
def test_half_midpoints_are_ties_to_even():
    h, nxt, mid = ref.half_midpoint_table()
    assert len(h) == 0x7C00 and h[0] == 0 and h[-1] == 65504 and mid[-1] == 65520 and mid[0] == 2.0 ** -25
    with np.errstate(over="ignore"):
        down, up, tie = (v.astype(np.float16).view(np.uint16).astype(np.int64) for v in
                         (np.nextafter(mid, np.float32(0), dtype=np.float32), np.nextafter(mid, np.float32(np.inf), dtype=np.float32), mid))
    bits = np.arange(0x7C00, dtype=np.int64)
    assert np.array_equal(down, bits) and np.array_equal(up, bits + 1)  # 0x7BFF + 1 = 0x7C00 = inf
    assert np.array_equal(tie, bits + (bits & 1))                       # the even neighbour
    assert np.array_equal(h.astype(np.float16).view(np.uint16), bits.astype(np.uint16))


def test_half_rounding_inputs_hold_the_edges():
    v = ref.half_rounding_inputs()
    assert v.dtype == np.float32 and np.isnan(v).sum() == 2 and np.isinf(v).sum() == 2
    for edge in (65504.0, 65520.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -14, 0.0):
        assert (v == np.float32(edge)).any() and (v == -np.float32(edge)).any()
    assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    assert ((np.abs(v) < 2.0 ** -25) & (v != 0)).sum() >= 10
    assert np.array_equal(ref.all_half_bits().view(np.uint16).ravel(), np.arange(65536, dtype=np.uint16))


def test_same_bits_or_nan():
    a = np.array([1.0, np.nan, -0.0], dtype=np.float16)
    assert ref.same_bits_or_nan(a.copy(), a)
    assert not ref.same_bits_or_nan(np.array([1.0, np.nan, 0.0], dtype=np.float16), a)
    assert not ref.same_bits_or_nan(np.array([1.0, 2.0, -0.0], dtype=np.float16), a)


# ---- generators --------------------------------------------------------------------------------------------------------------
def test_generators_are_deterministic():
    assert np.array_equal(ref.int_factors(100, 7), ref.int_factors(100, 7))
    assert not np.array_equal(ref.int_factors(100, 7), ref.int_factors(100, 7, seed=1))
    for p in ref.REAL_PROFILES:
        assert np.array_equal(ref.real_factors(p, 50, 9), ref.real_factors(p, 50, 9))
    a, b = ref.loss_problem(20, 10, 5), ref.loss_problem(20, 10, 5)
    assert (a[0] != b[0]).nnz == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(ref.norm_rows(3), ref.norm_rows(3))
    assert np.array_equal(ref.random_bits((5, 3), np.float16).view(np.uint16), ref.random_bits((5, 3), np.float16).view(np.uint16))
    assert ref.random_bits((5, 3), np.float32).dtype == np.float32


# ---- RandomState -------------------------------------------------------------------------------------------------------------
def test_rng_words_layout():
    """Quad q <- counter (q_lo, q_hi, draw, tag), key (seed_lo, seed_hi); words in order; a prefix for every n."""
    seed = 2 ** 32 + 7
    w = ref.rng_words(seed, 3, 11, ref.TAG_NORMAL)
    assert w.dtype == np.uint32 and len(w) == 11
    for q in range(3):
        want = philox4x32_10(q, 0, 3, 1, 7, 1)
        assert [int(v) for v in w[4 * q:4 * q + 4]] == [int(v) for v in want][:len(w[4 * q:4 * q + 4])]
    assert np.array_equal(ref.rng_words(seed, 3, 5, 1), w[:5])
    # the seed's two halves, the draw and the tag all matter; -1 is the all-ones key
    assert not np.array_equal(ref.rng_words(7, 3, 11, 1), w) and not np.array_equal(ref.rng_words(seed, 2, 11, 1), w)
    assert not np.array_equal(ref.rng_words(seed, 3, 11, 0), w) and not np.array_equal(ref.rng_words(seed, 1, 11, 3), w)
    assert [int(v) for v in ref.rng_words(-1, 0, 4, 0)] == [int(v) for v in philox4x32_10(0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF)]


def test_u01_is_half_open_at_zero_and_closed_at_one():
    """((x >> 8) + 0.5f) / 2^24 in fp32: the smallest value is 2^-25, and 16777215 + 0.5 rounds to 2^24, so the largest is
    exactly 1.0 (for the 256 words 0xFFFFFF00 .. 0xFFFFFFFF)."""
    edge = np.array([0, 255, 256, 0x7FFFFFFF, 0x80000000, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32)
    u = ref.u01_ref(edge)
    assert u.dtype == np.float32
    assert u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[-1] == u[-2] == np.float32(1.0) and u[-3] < 1.0
    assert np.float32(16777215.0) + np.float32(0.5) == np.float32(16777216.0)
    wide = ref.u01_ref(ref.rng_words(1, 0, 1 << 16, 0))
    assert wide.min() > 0 and wide.max() <= 1.0 and abs(float(wide.mean()) - 0.5) < 0.01


def test_uniform_ref_is_fp32_affine_in_u():
    u = ref.uniform_ref(42, 0, 1001)
    assert u.dtype == np.float32 and np.array_equal(u, ref.u01_ref(ref.rng_words(42, 0, 1001, 0)))
    v = ref.uniform_ref(42, 0, 1001, -0.3, 0.9)
    lo, hi = np.float32(-0.3), np.float32(0.9)
    assert v.dtype == np.float32 and np.array_equal(v, lo + np.float32(hi - lo) * u)
    assert np.array_equal(ref.uniform_ref(42, 0, 7), u[:7]) and not np.array_equal(ref.uniform_ref(42, 1, 7), u[:7])


def test_randn_ref_is_box_muller_of_the_same_words():
    n = 200_001
    z = ref.randn_ref(42, 0, n)
    assert z.dtype == np.float64 and len(z) == n and abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    u = ref.u01_ref(ref.rng_words(42, 0, 8, 1)).astype(np.float64)
    assert z[4] == np.sqrt(-2 * np.log(u[4])) * np.cos(2 * np.pi * u[5])
    assert z[7] == np.sqrt(-2 * np.log(u[6])) * np.sin(2 * np.pi * u[7])
    assert np.array_equal(ref.randn_ref(42, 0, n, 0.0, 0.01), 0.01 * z)
    # numpy's own fp32 evaluation of the same formula is well inside the bar the device is held to
    u32 = ref.u01_ref(ref.rng_words(42, 0, n + 3, 1)).reshape(-1, 2, 2)
    m = np.sqrt(np.float32(-2) * np.log(u32[:, :, 0]))
    ang = np.float32(6.2831853071795865) * u32[:, :, 1]
    z32 = np.stack([m * np.cos(ang), m * np.sin(ang)], axis=2).reshape(-1)[:n]
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5


def test_unit_draws_are_pinned():
    """The words that make u01 exactly 1.0: uniform() returns `high`, randn() a zero radius."""
    seed, at, word = ref.UNIT_UNIFORM
    assert int(ref.rng_words(seed, 0, at + 1, ref.TAG_UNIFORM)[at]) == word and word >> 8 == 0xFFFFFF
    assert ref.uniform_ref(seed, 0, at + 1)[at] == 1.0 and ref.uniform_ref(seed, 0, at + 1, -0.5, 0.5)[at] == 0.5
    seed, at, word = ref.UNIT_NORMAL
    assert at % 4 in (0, 2) and word >> 8 == 0xFFFFFF
    assert int(ref.rng_words(seed, 0, at + 2, ref.TAG_NORMAL)[at]) == word
    z = ref.randn_ref(seed, 0, at + 2)
    assert z[at] == 0 and z[at + 1] == 0 and np.isfinite(z).all()
    # the search that found them, on the seed it ends at
    assert ref.find_unit_word(ref.TAG_UNIFORM, (0, 1, 2, 3), seeds=[ref.UNIT_UNIFORM[0]]) == ref.UNIT_UNIFORM
    assert ref.find_unit_word(ref.TAG_NORMAL, (0, 2), seeds=[ref.UNIT_NORMAL[0]]) == ref.UNIT_NORMAL
    assert ref.find_unit_word(ref.TAG_NORMAL, (0, 2), seeds=[0], quads=1024) is None
