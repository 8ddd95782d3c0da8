"""Which kernel a factor count reaches: the host dispatch of the CG and Cholesky half sweeps, route by route.

One 19-row matrix serves every case.  Its row lengths sit on both sides of every cut of the row schedule (16, 32, 64, 128,
256, 512), one row lies above the 1024-nonzero cut of the f = 64 Cholesky's segment plan and one (2100 nonzeros) in the first
multi-segment bracket of the normal-matrix plan; two rows are empty.  The factor counts sit on both sides of every cut of the
`if` chain in least_squares_cg, of the padding widths (64 / 128 / 256) and of the Cholesky routes (wave kernels, f = 64,
padded, f = 128, workgroup kernel in LDS and in the device workspace).  The routes an environment switch selects run the same
body in a fresh child process (the switches are read once per process).

Every case is held to the project's parity gate against the CPU oracle -- relative Frobenius distance below 1e-4, 1e-3 for
fp16 factor storage -- over the sweep AND for every non-empty row on its own (one wrong short row would hide behind the
2100-nonzero one in a Frobenius norm).  The oracle's own distance from its fp64 evaluation on this matrix is at most 1.7e-6
per row.  Empty rows come back zero; X has three rows more than the matrix, which come back bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTHS = [0, 1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1100, 2100, 0, 5]
COLS, EXTRA_ROWS, REG = 2400, 3, 0.05
TOL = {"float32": 1e-4, "float16": 1e-3}

CG_FACTORS = [1, 20, 63, 64, 65, 100, 127, 128, 129, 192, 255, 256, 257, 384, 385, 512, 513, 768, 769, 1024]
CHOLESKY_FACTORS = [8, 32, 33, 64, 65, 100, 127, 128, 129, 256, 257]

# a case: (solver, factors, storage, cg_steps, rows); rows = "all" or "fold_in" (the first two non-empty rows only: the padded
# Cholesky route leaves a handful of rows against a large Y, nnz * 4 < Y.rows, to the workgroup kernel)
DEFAULT_CASES = (
    [("cg", f, "float32", 3, "all") for f in CG_FACTORS]
    + [("cg", f, "float32", steps, "all") for f in (64, 256, 320) for steps in (0, 1)]
    + [("cg", f, "float16", 3, "all") for f in (64, 100, 128)]
    + [("cholesky", f, "float32", 3, "all") for f in CHOLESKY_FACTORS]
    + [("cholesky", 100, "float32", 3, "fold_in")]
    + [("cholesky", f, "float16", 3, "all") for f in (64, 100)]
)
SWITCHED_CASES = {
    "IMP_NO_PAD=1": [("cg", f, "float32", 3, "all") for f in (20, 100, 150, 200)],
    "IMP_NM=0": [("cg", f, storage, 3, "all") for f in (64, 128) for storage in ("float32", "float16")],
    "IMP_F256_OLD=1": [("cg", 256, "float32", 3, "all")],
    "IMP_CHOL_PAD=0": [("cholesky", 100, "float32", 3, "all")],
    "IMP_CHOL_NM=0": [("cholesky", f, "float32", 3, "all") for f in (100, 128)],
}


def case_id(case):
    solver, f, storage, steps, rows = case
    return f"{solver}-f{f}-{storage}" + (f"-steps{steps}" if solver == "cg" else "") + ("" if rows == "all" else "-" + rows)


@functools.lru_cache(maxsize=None)
def _matrix():
    """Integers 1 .. 5 as confidences; every row of two or more entries has exactly ONE negated entry (a row of negative
    confidences only has a zero right-hand side: its solution is 0 and a relative distance means nothing)."""
    rng = np.random.default_rng(2024)
    indices, data = [], []
    for n in LENGTHS:
        indices.append(np.sort(rng.choice(COLS, size=n, replace=False)))
        c = rng.integers(1, 6, size=n).astype(np.float32)
        if n >= 2:
            c[rng.integers(n)] *= -1
        data.append(c)
    indptr = np.concatenate([[0], np.cumsum(LENGTHS)])
    return sp.csr_matrix((np.concatenate(data), np.concatenate(indices).astype(np.int32), indptr), shape=(len(LENGTHS), COLS))


@functools.lru_cache(maxsize=None)
def _inputs(f, storage, rows):
    """(C, X0, Y0): the factors in their storage type, X0 with EXTRA_ROWS rows more than C."""
    C = _matrix()
    if rows == "fold_in":
        C = C[[1, 2]]
        assert C.nnz * 4 < COLS
    rng = np.random.default_rng(f)
    X0 = (rng.random((C.shape[0] + EXTRA_ROWS, f), dtype=np.float32) * 0.2 - 0.1).astype(storage)
    Y0 = (rng.random((COLS, f), dtype=np.float32) * 0.2 - 0.1).astype(storage)
    return C, X0, Y0


def solve(gpu, case, solver=None):
    """The half sweep of `case` on the GPU: (X after the call, the gramian the solver was handed).  `solver`: a solver object that
    has been used before (tests/test_gpu_cholesky_edges.py: right after a failing call), instead of a new one."""
    solver_kind, f, storage, steps, rows = case
    C, X0, Y0 = _inputs(f, storage, rows)
    solver = solver or gpu.LeastSquaresSolver()
    Xd, Yd, gram = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix.zeros(f, f)
    if solver_kind == "cg":
        solver.calculate_yty(Yd, gram, REG)
        solver.least_squares(gpu.CSRMatrix(C), Xd, gram, Yd, steps)
    else:
        solver.calculate_yty(Yd, gram, 0.0)
        solver.least_squares_cholesky(gpu.CSRMatrix(C), Xd, gram, Yd, REG)
    return Xd.to_numpy(), gram.to_numpy()


_WANT = {}


def expected(oracle, case, gram):
    """The oracle on the same inputs (fp16 storage: on the fp16-rounded inputs), computed once per case."""
    if case not in _WANT:
        solver_kind, f, storage, steps, rows = case
        C, X0, Y0 = _inputs(f, storage, rows)
        Y32 = Y0.astype(np.float32)
        if solver_kind == "cg":
            want = X0[: C.shape[0]].astype(np.float32)
            oracle.least_squares_cg(C, want, Y32, REG, cg_steps=steps, YtY=gram)
        else:
            want = np.zeros((C.shape[0], f), dtype=np.float32)
            oracle.least_squares(C, want, Y32, REG, YtY=gram)
        want.setflags(write=False)
        _WANT[case] = want
    return _WANT[case]


def check(gpu, oracle, case, solver=None):
    solver_kind, f, storage, steps, rows = case
    C, X0, _ = _inputs(f, storage, rows)
    got, gram = solve(gpu, case, solver)
    want = expected(oracle, case, gram)
    n = C.shape[0]
    assert got.dtype == X0.dtype and got.shape == X0.shape
    np.testing.assert_array_equal(got[n:], X0[n:])          # rows beyond the matrix: untouched, bit for bit
    lens = np.diff(C.indptr)
    assert not got[:n][lens == 0].any()                      # empty rows: zero
    assert np.isfinite(want).all()
    diff = np.linalg.norm(got[:n].astype(np.float64) - want, axis=1)
    norm = np.linalg.norm(want.astype(np.float64), axis=1)
    per_row = diff[lens > 0] / np.maximum(norm[lens > 0], 1e-30)
    whole = float(np.linalg.norm(diff) / max(np.linalg.norm(norm), 1e-30))
    print(f"{case_id(case)}: sweep {whole:.2e}, worst row {per_row.max():.2e} (nnz {lens[lens > 0][per_row.argmax()]})")
    assert whole < TOL[storage], (case_id(case), whole)
    assert (per_row < TOL[storage]).all(), (case_id(case), dict(zip(lens[lens > 0].tolist(), per_row.tolist())))


@pytest.mark.parametrize("case", DEFAULT_CASES, ids=case_id)
def test_default_route(gpu, oracle, case):
    check(gpu, oracle, case)


def run_switched(switch):
    """Body of the child process of test_switched_route."""
    import warnings

    warnings.simplefilter("ignore")
    import implicit_amd.gpu as gpu
    from oracle import oracle

    oracle.build()
    for case in SWITCHED_CASES[switch]:
        check(gpu, oracle, case)
    print("routes ok")


@pytest.mark.parametrize("switch", list(SWITCHED_CASES))
def test_switched_route(gpu, switch):
    """The kernels an A/B switch selects, at the factor counts where the default run takes others."""
    name, value = switch.split("=")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_solver_routes as t; t.run_switched({switch!r})")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{name: value}), capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "routes ok" in out.stdout, (out.stdout + out.stderr)[-3000:]
