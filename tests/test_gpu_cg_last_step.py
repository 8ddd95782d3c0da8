"""The last CG step of the tile kernels (rows of up to 512 nonzeros at f = 64 / 128): the last pass forms only the scalar p.Ap
(als_qf_common.h).

Per-row checks against the CPU oracle at every width of the schedule and every position of the last step (cg_steps 1..4), rows
that stop early next to rows that run all their steps (a team whose waves lose count of the generations never finishes), and
bitwise reproducibility (the leader sums the team's scalars in wave order).
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

TOL = 1e-4       # the project's parity bar (tests/test_gpu_als.py)
TOL_HALF = 1e-3  # float16 storage: the result is stored in fp16
ITEMS = 3000

# both sides of every cut: the short-row kernel (<= 32), team widths 2 / 4 / 8 / 16 (64 / 128 / 256 / 512), the packed fp16
# tiles (64 per wave), whole and ragged 4-entry tile steps and 8-entry pairs; one empty row
LENGTHS = [1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 47, 48, 49, 64, 65, 128, 129, 256, 257, 512] * 5 + [0]


def _csr(rows, items):
    indptr = np.cumsum([0] + [len(cols) for cols, _ in rows])
    indices = np.concatenate([cols for cols, _ in rows]).astype(np.int32)
    data = np.concatenate([c for _, c in rows]).astype(np.float32)
    return sp.csr_matrix((data, indices, indptr), shape=(len(rows), items))


def _confidences(rng, n, neg_frac=0.1):
    """1 .. 5, a tenth of them negative -- but never a whole row: with only negative confidences the right-hand side
    sum c+ y is 0, the iterates run towards x = 0 (a factor ~ 1e-3 in norm over four steps here), and a per-row error
    RELATIVE to that vanishing norm measures the fp32 cancellation in x + alpha p, in the oracle as much as in the kernels
    (the oracle itself is then 4e-4 from its own fp64 evaluation)."""
    c = 1 + 4 * rng.random(n)
    c[rng.random(n) < neg_frac] *= -1
    if n and (c < 0).all():
        c[0] = -c[0]
    return c


_cache = {}


def _parity_problem(f):
    """One matrix for every case of a factor count; never modified."""
    if f not in _cache:
        rng = np.random.default_rng(100 + f)
        C = _csr([(np.sort(rng.choice(ITEMS, size=n, replace=False)), _confidences(rng, n)) for n in LENGTHS], ITEMS)
        Y = ((rng.random((ITEMS, f), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
        X = ((rng.random((len(LENGTHS), f), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
        _cache[f] = (C, X, Y)
    return _cache[f]


def _gpu_cg(gpu, C, X, Y, reg, cg_steps, gram=None):
    solver = gpu.LeastSquaresSolver()
    Xd, Yd = gpu.Matrix(X), gpu.Matrix(Y)
    if gram is None:
        gramd = gpu.Matrix.zeros(X.shape[1], X.shape[1])
        solver.calculate_yty(Yd, gramd, reg)
    else:
        gramd = gpu.Matrix(gram)
    solver.least_squares(gpu.CSRMatrix(C), Xd, gramd, Yd, cg_steps)
    return Xd.to_numpy(), gramd.to_numpy()


def _row_errors(got, want):
    num = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    return num / np.maximum(np.linalg.norm(want.astype(np.float64), axis=1), 1e-30)


@pytest.mark.parametrize("cg_steps", [1, 2, 3, 4])
@pytest.mark.parametrize("f", [64, 128])
def test_last_step_row_by_row(gpu, oracle, f, cg_steps):
    """fp32 storage: every row within 1e-4 of the oracle, the empty row set to zero (_als.pyx:182)."""
    C, X, Y = _parity_problem(f)
    want = X.copy()
    oracle.least_squares_cg(C, want, Y, 0.05, cg_steps=cg_steps)
    got, _ = _gpu_cg(gpu, C, X.copy(), Y, 0.05, cg_steps)
    err = _row_errors(got, want)
    print("f", f, "cg", cg_steps, "per-row rel max %.2e" % err.max(), "at length", LENGTHS[int(err.argmax())])
    assert err.max() < TOL
    assert LENGTHS[-1] == 0 and not got[-1].any()


@pytest.mark.parametrize("cg_steps", [1, 2, 3])
@pytest.mark.parametrize("f", [64, 128])
def test_last_step_row_by_row_half(gpu, oracle, f, cg_steps):
    """float16 storage: within 1e-3 of the oracle run on the fp16-rounded inputs with the GPU's gramian of them (as
    test_half_team_width_boundaries_row_by_row in tests/test_gpu_als.py)."""
    C, X, Y = _parity_problem(f)
    X, Y = X.astype(np.float16), Y.astype(np.float16)
    got, gram = _gpu_cg(gpu, C, X.copy(), Y, 0.05, cg_steps)
    assert got.dtype == np.float16
    want = X.astype(np.float32)
    oracle.least_squares_cg(C, want, Y.astype(np.float32), 0.05, cg_steps=cg_steps, YtY=gram)
    err = _row_errors(got, want)
    print("f", f, "cg", cg_steps, "fp16 per-row rel max %.2e" % err.max(), "at length", LENGTHS[int(err.argmax())])
    assert err.max() < TOL_HALF
    assert not got[-1].any()


@pytest.mark.parametrize("f", [64, 128])
def test_early_stops_next_to_full_rows(gpu, oracle, f):
    """Rows that stop before the first step (a), after one step (b) and rows that take all three (c), interleaved in every
    row class, with the identity as the regularised gramian.  (a) and (b) reference only items whose factors are zero, so
    their system is x = 0: (a) starts there and never steps; (b) starts at 1e-5 (U - 0.5), its one step has alpha = 1 and
    lands on 0 -- exactly in the oracle, within rcp's 1 ulp (1e-7 * 1e-5 per component) on the GPU, where the residual
    after it is below 1e-20 as well, also through the three-term bf16 product of the short-row kernel (2^-24 relative).
    The waves of a team count the leader's generations: a team that loses count on one kind of row never returns."""
    zero_items, per_length = 500, 36
    rng = np.random.default_rng(7 + f)
    rows, kinds = [], []
    for n in (20, 40, 100, 200, 400):
        for j in range(per_length):
            kind = "abc"[j % 3]
            pool = np.arange(zero_items, ITEMS) if kind == "c" else np.arange(zero_items)
            rows.append((np.sort(rng.choice(pool, size=n, replace=False)), _confidences(rng, n)))
            kinds.append(kind)
    kinds = np.array(kinds)
    C = _csr(rows, ITEMS)
    Y = ((rng.random((ITEMS, f), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    Y[:zero_items] = 0
    X = ((rng.random((len(rows), f), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    X[kinds == "a"] = 0
    X[kinds == "b"] = (1e-5 * (rng.random((int((kinds == "b").sum()), f), dtype=np.float32) - 0.5)).astype(np.float32)
    gram = np.eye(f, dtype=np.float32)
    want = X.copy()
    oracle.least_squares_cg(C, want, Y, 1.0, cg_steps=3, YtY=gram)
    assert not want[kinds != "c"].any()  # the oracle's (b) rows land on 0 exactly
    got, _ = _gpu_cg(gpu, C, X.copy(), Y, 1.0, 3, gram=gram)
    assert not got[kinds == "a"].any()
    b_max = float(np.abs(got[kinds == "b"]).max())
    err = _row_errors(got[kinds == "c"], want[kinds == "c"])
    print("f", f, "stopped-after-one-step max |x| %.2e" % b_max, "live per-row rel max %.2e" % err.max())
    assert b_max <= 1e-10
    assert err.max() < TOL


def test_last_step_reproducible(gpu):
    """Two launches on the same inputs agree bit for bit: the team's scalars are summed in wave order."""
    C, X, Y = _parity_problem(128)
    first, _ = _gpu_cg(gpu, C, X.copy(), Y, 0.05, 3)
    second, _ = _gpu_cg(gpu, C, X.copy(), Y, 0.05, 3)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
