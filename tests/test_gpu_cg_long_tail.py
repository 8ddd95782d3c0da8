"""The tail of the long-row path of a CG half sweep (rows of more than 512 nonzeros, csrc/als_cg_nm.hip) where fp32 storage at
f = 128 takes the two chained launches: the rows cut into segments are finished at the head of the chain of the three
512-thread classes (nm_finish_items, csrc/als_nm_image.h), the rows listed for the fp32 fix-up are re-solved at the head of the
chain of the two 1024-thread classes (csrc/als_cg_qf.hip).  A chain without rows of its own is not launched and leaves its
passenger to the stand-alone kernels; f = 64, float16 storage and a per-kernel profiler pass keep them throughout
(csrc/long_tail_route.h, pinned on the host in test_long_tail_route_host.py).

Every case is held
  * per row to the CPU oracle at 1e-4 relative (test_gpu_nm.py's bar; rows listed for the fix-up: max(1e-4, 2 x the oracle's own
    distance from its float64 restatement), as there),
  * bit for bit to the same call under an unfiltered profiler, which takes the per-class and stand-alone launches,
  * bit for bit to a second identical call,
and the route it claims is read from the profiler's scope counts: 0 launches of a stand-alone scope where the part is folded, 1
where it is not.  IMP_NM_SEGMENT is set before every CSRMatrix is built, so short rows are "long rows of many segments" here."""
import numpy as np
import pytest

from test_gpu_nm import TOL, _long_row_matrix, _row_errors, _solve

pytestmark = pytest.mark.gpu

F, REG = 128, 0.01
FINISH, FIXUP = "als_cg_nm_finish", "als_cg_fixup"
D = 8  # segments whose loads a thread keeps in flight per piece of the image (kNmSegBatch, csrc/als_nm_image.h)

LONG = [513, 600, 1001, 2500, 6000]  # segment 1000: whole, whole, 2, 3 and 6 segments
MID = [40, 100, 200]                 # the chain of the 512-thread classes: (32,64], (64,128], (128,256]
WIDE = [300, 20, 5]                  # the chain of the 1024-thread classes: (256,512] and the short rows
VARIANTS = {          # lengths, stand-alone launches of (finish, fix-up)
    "a": (LONG + MID + WIDE + [0], (0, 0)),
    "b": (LONG + WIDE + [0], (1, 0)),          # no row in 33 .. 256: no team chain
    "c": (LONG + MID + [0], (0, 1)),           # no row in 257 .. 512 and none <= 32: no wide chain
    "d": (LONG, (1, 1)),                       # long rows only
}


def _factors(rows, items, f, seed):
    rng = np.random.default_rng(seed)
    Y = (rng.standard_normal((items, f)) * 0.1).astype(np.float32)
    X = (rng.standard_normal((rows, f)) * 0.1).astype(np.float32)
    return X, Y


def _scoped(gpu, only, C, X, Y, steps, dtype):
    """The solve under the library profiler: `only` None takes every scope (and with it the per-class and stand-alone launches),
    a name leaves the routes alone and counts that scope.  Returns (result, launches of `only`)."""
    gpu.Profiler.reset()
    if only is None:
        gpu.Profiler.enable(True)
    else:
        gpu.Profiler.enable(True, only=only)
    try:
        got = _solve(gpu, C, X.copy(), Y, REG, steps, dtype)
        count = gpu.Profiler.get(only)[1] if only else -1
    finally:
        gpu.Profiler.enable(False)
        gpu.Profiler.reset()
    return got, count


def _check(gpu, oracle, C, X, Y, steps, routes, dtype="float32", listed=()):
    """All the comparisons of the module docstring for one matrix; `routes` = stand-alone launches of (finish, fix-up)."""
    word = np.uint32
    if dtype == "float16":
        X, Y = X.astype(np.float16).astype(np.float32), Y.astype(np.float16).astype(np.float32)
    got = _solve(gpu, C, X.copy(), Y, REG, steps, dtype)
    again = _solve(gpu, C, X.copy(), Y, REG, steps, dtype)
    per_kernel, _ = _scoped(gpu, None, C, X, Y, steps, dtype)
    with_finish, n_finish = _scoped(gpu, FINISH, C, X, Y, steps, dtype)
    with_fixup, n_fixup = _scoped(gpu, FIXUP, C, X, Y, steps, dtype)
    print("stand-alone launches: finish", n_finish, "fix-up", n_fixup, "claimed", routes)
    assert (n_finish, n_fixup) == routes
    for other in (again, per_kernel, with_finish, with_fixup):
        np.testing.assert_array_equal(other.view(word), got.view(word))
    want = X.copy()
    oracle.least_squares_cg(C, want, Y, REG, cg_steps=steps)
    lens = np.diff(C.indptr)
    assert np.isfinite(got).all()
    assert not got[lens == 0].any()
    if dtype == "float16":  # one fp16 rounding of the result on top of the bar (test_gpu_nm.py::test_fp16_factor_storage)
        bar = np.abs(want).max(axis=1, keepdims=True) * 2.0 ** -10
        assert (np.abs(got - want) <= bar + TOL * np.abs(want)).all()
        return got
    err = _row_errors(got, want)
    bar = np.full(len(lens), TOL)
    if len(listed):  # measured from float64, against the oracle's own distance from it
        assert steps == 3
        idx = list(listed)
        exact = oracle.least_squares_cg_f64(C, X, Y, REG)
        err[idx] = _row_errors(got, exact)[idx]
        bar[idx] = np.maximum(TOL, 2.0 * _row_errors(want, exact)[idx])
    err[lens == 0] = 0.0
    worst = int(np.argmax(err / bar))
    print("per-row rel max %.2e (nnz %d, bar %.1e)" % (err[worst], lens[worst], bar[worst]))
    assert (err < bar).all()
    return got


@pytest.mark.parametrize("variant,steps", [("a", 3), ("a", 1), ("b", 3), ("c", 3), ("d", 3)])
def test_routes(gpu, oracle, monkeypatch, variant, steps):
    monkeypatch.setenv("IMP_NM_SEGMENT", "1000")
    lengths, routes = VARIANTS[variant]
    items = 6500
    C = _long_row_matrix(lengths, items, seed=3)
    X, Y = _factors(len(lengths), items, F, 5)
    _check(gpu, oracle, C, X, Y, steps, routes)


@pytest.mark.parametrize("segment,counts", [(300, [2, 3, 4, 5, D - 1, D, D + 1, 2 * D + 1, 21]), (150, [33, 34, 43])])
def test_segment_count_cuts(gpu, oracle, monkeypatch, segment, counts):
    """Rows of exactly 2, 3, D - 1, D, D + 1, 2 D + 1 and >= 33 segments (and 4 and 5: the loop changes its shape between them);
    the last segment of every row is full or holds one nonzero, alternately."""
    monkeypatch.setenv("IMP_NM_SEGMENT", str(segment))
    lengths = [segment * (n - 1) + (segment if i % 2 == 0 else 1) for i, n in enumerate(counts)]
    assert min(lengths) > 512 and max(lengths) <= 6500
    assert [-(-n // segment) for n in lengths] == counts
    lengths = lengths + MID + WIDE
    items = 6500
    C = _long_row_matrix(lengths, items, seed=7)
    X, Y = _factors(len(lengths), items, F, 9)
    _check(gpu, oracle, C, X, Y, 3, (0, 0))


def _resident_chain_grid():
    from test_gpu_knn_edges import _num_cus

    return 2 * _num_cus()  # workgroups of the 512-thread chain: two per CU (its LDS)


@pytest.mark.parametrize("which", ["1", "G-1", "G", "G+1", "2G+6"])
def test_stride_cuts(gpu, oracle, monkeypatch, which):
    """n_multi rows of three segments on a grid of G workgroups: one row, one short of a row each, a row each, one workgroup with
    two, and two full strides and a few."""
    monkeypatch.setenv("IMP_NM_SEGMENT", "256")
    G = _resident_chain_grid()
    n_multi = {"1": 1, "G-1": G - 1, "G": G, "G+1": G + 1, "2G+6": 2 * G + 6}[which]
    rng = np.random.default_rng(n_multi)
    lengths = list(rng.integers(513, 531, size=n_multi)) + MID + [300, 20]
    items = 3000
    C = _long_row_matrix(lengths, items, seed=n_multi)
    X, Y = _factors(len(lengths), items, F, 13)
    _check(gpu, oracle, C, X, Y, 3, (0, 0))


@pytest.mark.parametrize("variant", ["a", "b", "c"])
def test_listed_rows(gpu, oracle, monkeypatch, variant):
    """The hot-item construction of test_gpu_nm.py::test_operands_beyond_the_fp16_range_are_resolved_in_fp32: a whole long row
    (600) and a row of three segments (2500) leave the fp16 range and are listed, 900 and 5000 stay in range; every other row
    gives the hot items weight zero."""
    monkeypatch.setenv("IMP_NM_SEGMENT", "1000")
    items = 6000
    long_rows = [600, 900, 2500, 5000]
    tail, routes = {"a": (MID + WIDE + [0], (0, 0)), "b": (WIDE + [0], (1, 0)), "c": (MID + [0], (0, 1))}[variant]
    lengths = long_rows + tail
    C = _long_row_matrix(lengths, items, seed=12)
    X, Y = _factors(len(lengths), items, F, 7)
    rng = np.random.default_rng(17)
    hot = np.arange(0, items, 10)
    Y[hot] = (rng.standard_normal((len(hot), F)) * 40).astype(np.float32)
    listed = (0, 2)
    for r in range(len(lengths)):
        lo, hi = C.indptr[r], C.indptr[r + 1]
        C.data[lo:hi][np.isin(C.indices[lo:hi], hot)] = 1e6 if r in listed else 1.0  # 1.0: weight 0
    gpu.fixup_rows(reset=True)
    got = _solve(gpu, C, X.copy(), Y, REG, 3)
    assert gpu.fixup_rows(reset=True) == 2 and np.isfinite(got).all()
    _check(gpu, oracle, C, X, Y, 3, routes, listed=listed)
    gpu.fixup_rows(reset=True)
    # and an ordinary solve leaves the counter alone
    C2 = _long_row_matrix([700, 3000] + tail, items, seed=1)
    _solve(gpu, C2, X[: C2.shape[0]].copy(), Y * np.float32(0.01), REG, 3)
    assert gpu.fixup_rows(reset=True) == 0


@pytest.mark.parametrize("f,dtype", [(64, "float32"), (128, "float16")])
def test_unchanged_routes(gpu, oracle, monkeypatch, f, dtype):
    """f = 64 and float16 storage keep the stand-alone launches."""
    monkeypatch.setenv("IMP_NM_SEGMENT", "1000")
    lengths = [600, 2500] + MID + WIDE + [0]
    items = 3000
    C = _long_row_matrix(lengths, items, seed=6)
    X, Y = _factors(len(lengths), items, f, 3)
    _check(gpu, oracle, C, X, Y, 3, (1, 1), dtype=dtype)
