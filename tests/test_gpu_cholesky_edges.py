"""The Cholesky half sweep at its failure paths and operand edges (problems and float64 restatement: tests/cholesky_cases.py,
proved on the CPU by tests/test_cholesky_cases_host.py).

a. The failure contract on every route: a call with rows that are not positive definite raises ValueError, names the SMALLEST
   failing row, solves every other row to the project's gate against the oracle (1e-4 per row, 1e-3 for fp16 storage), leaves the
   failing rows and the rows beyond the matrix bit for bit as they were, zeroes the empty rows -- and leaves nothing behind: the
   routes test's benign sweep on the same solver object right afterwards meets its ordinary gate.
b. The fall-back that succeeds: rows whose matrix-core operands leave the fp16 range are listed by nm_chol and solved by the fp32
   workgroup kernel through the device-side list, alone and beside a row that really fails.
c. The operand edges of tests/test_gpu_nm.py's CG cases on the Cholesky kernels, at f = 128 and on the padded route (f = 100).

A ValueError from a non-positive pivot is an answer of the API, not a fault of the device."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cholesky_cases as cc
import test_gpu_solver_routes as routes

pytestmark = pytest.mark.gpu
ROOT = routes.ROOT
TOL = routes.TOL

# (f, storage): wave <32> with the rows above 256 nonzeros on the unpacked workgroup kernel (16, 32); wave <64> (48); the f = 64
# kernel with its segment partials; padded -> nm -> list -> packed workgroup kernel (100); nm rows / long / finish kernels -> list
# (128); the packed LDS kernel (200); the workspace kernel (320); fp16 storage through the fp32 copies
DEFAULT_ROUTES = [(f, "float32") for f in (16, 32, 48, 64, 100, 128, 200, 320)] + [(64, "float16"), (128, "float16")]
SWITCHED_ROUTES = {"IMP_CHOL_PAD=0": [80, 100], "IMP_CHOL_NM=0": [128]}  # workgroup kernel: unpacked (80), packed (100, 128)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def call(gpu, p, solver=None, C=None):
    """(X after the call, the ValueError or None)."""
    solver = solver or gpu.LeastSquaresSolver()
    Xd, Yd, gram = gpu.Matrix(p.X0), gpu.Matrix(p.Y), gpu.Matrix(p.gram)
    error = None
    try:
        solver.least_squares_cholesky(C if C is not None else gpu.CSRMatrix(p.C), Xd, gram, Yd, p.reg)
    except ValueError as e:
        error = e
    got = Xd.to_numpy()
    assert got.dtype == p.X0.dtype and got.shape == p.X0.shape
    return got, error


@functools.lru_cache(maxsize=None)
def _failing_problem(f, failing, storage):
    return cc.failing_problem(f, failing, storage)


_ORACLE = {}


def oracle_of(oracle, p):
    """(want, named row, float64 rows): once per problem, read-only."""
    if p.name not in _ORACLE:
        want, named = cc.oracle_rows(oracle, p)
        exact, failed = cc.solve_f64(p.C, p.Y.astype(np.float32), p.gram, p.reg)
        assert failed == sorted(p.failing) and named == (min(p.failing) if p.failing else None)
        want.setflags(write=False), exact.setflags(write=False)
        _ORACLE[p.name] = (want, named, exact)
    return _ORACLE[p.name]


def check_untouched(p, got, error):
    """What holds for every call: the error names min(failing) or there is none; empty rows zero; failing rows and the rows
    beyond the matrix bit for bit what they were."""
    n = p.C.shape[0]
    lens = np.diff(p.C.indptr)
    if p.failing:
        first = min(p.failing)
        assert error is not None, "no ValueError"
        assert re.search(rf"cholesky.* row {first}\b", str(error)), str(error)
        assert error.failed_row == first
        bad = np.array(sorted(p.failing))
        assert bits(got[bad]) == bits(p.X0[bad]), "a failing row was written"
    else:
        assert error is None, str(error)
    assert not got[:n][lens == 0].any()
    assert bits(got[n:]) == bits(p.X0[n:])
    return np.array([u for u in range(n) if lens[u] > 0 and u not in p.failing])


def check_failing(gpu, oracle, p, C=None):
    solver = gpu.LeastSquaresSolver()
    got, error = call(gpu, p, solver, C)
    good = check_untouched(p, got, error)
    want, _, _ = oracle_of(oracle, p)
    per_row = cc.row_errors(got[good].astype(np.float32), want[good])
    print(f"{p.name}: named row {error.failed_row}, worst good row {per_row.max():.2e} (row {good[per_row.argmax()]})")
    assert (per_row < TOL[p.storage]).all(), dict(zip(good.tolist(), per_row.tolist()))
    # nothing of the failing call survives it: the failure word, the fix list, the tickets, the padded copies
    routes.check(gpu, oracle, ("cholesky", p.f, p.storage, 3, "all"), solver)


@pytest.mark.parametrize("failing", cc.FAILING_SETS, ids=lambda s: "rows" + "_".join(map(str, s)))
@pytest.mark.parametrize("route", DEFAULT_ROUTES, ids=lambda r: f"f{r[0]}-{r[1]}")
def test_failure_contract(gpu, oracle, route, failing):
    check_failing(gpu, oracle, _failing_problem(route[0], failing, route[1]))


def run_switched(switch):
    """Body of the child process of test_failure_contract_on_switched_routes."""
    import warnings

    warnings.simplefilter("ignore")
    import implicit_amd.gpu as gpu
    from oracle import oracle

    oracle.build()
    for f in SWITCHED_ROUTES[switch]:
        for failing in cc.FAILING_SETS:
            check_failing(gpu, oracle, _failing_problem(f, failing, "float32"))
    print("edges ok")


@pytest.mark.parametrize("switch", list(SWITCHED_ROUTES))
def test_failure_contract_on_switched_routes(gpu, switch):
    """The workgroup kernels where the default process takes the padded and the normal-matrix routes (the switches are read once
    per process)."""
    name, value = switch.split("=")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_cholesky_edges as t; t.run_switched({switch!r})")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{name: value}), capture_output=True, text=True,
                         timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "edges ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


@pytest.mark.parametrize("failing", cc.BLOCK_FAILING_SETS, ids=lambda s: "rows" + "_".join(map(str, s)))
def test_failure_contract_across_row_blocks(gpu, oracle, monkeypatch, failing):
    """The matrix held as four row blocks (rows 0 .. 14, 15, 16 .. 17, 18: test_block_limit_puts_the_failing_rows_in_three_blocks):
    the row a block reports is numbered inside the block, the row the call names is the row of the whole matrix -- row 16 from
    the third block, row 15 from the second before row 16 from the third, row 4 from the first."""
    p = _failing_problem(64, failing, "float32")
    C64 = p.C.copy()
    C64.indptr = C64.indptr.astype(np.int64)
    C64.indices = C64.indices.astype(np.int64)
    monkeypatch.setenv("IMP_CSR_PART_NNZ", str(cc.BLOCK_NNZ))
    blocks = gpu.CSRMatrix(C64)
    monkeypatch.delenv("IMP_CSR_PART_NNZ")
    check_failing(gpu, oracle, p, blocks)


def check_bar(p, rows, got, want, exact, bar):
    """The bars of tests/test_gpu_nm.py's twins over `rows`; prints gpu-vs-f64 and oracle-vs-f64 per row first."""
    got = got.astype(np.float32)
    e_gpu, e_oracle = cc.row_errors(got[rows], exact[rows]), cc.row_errors(want[rows], exact[rows])
    vs_oracle = cc.row_errors(got[rows], want[rows])
    fmt = lambda e: " ".join("%.1e" % v for v in e)  # noqa: E731
    print(f"{p.name} [{bar}] rows {rows.tolist()}: gpu vs f64 {fmt(e_gpu)} | oracle vs f64 {fmt(e_oracle)} | gpu vs oracle {fmt(vs_oracle)}")
    assert np.isfinite(got[rows]).all()
    if bar == "oracle2":
        assert (e_gpu < np.maximum(1e-4, 2.0 * e_oracle)).all()
    elif bar == "gate":
        assert (vs_oracle < 1e-4).all()
    elif bar == "bits":
        assert (e_gpu < np.maximum(1e-6, 1.5 * e_oracle)).all()
    elif bar == "fp16":  # one fp16 rounding of the result: half an ulp of the row's largest element
        half_ulp = np.abs(want[rows]).max(axis=1, keepdims=True) * 2.0 ** -10
        assert (np.abs(got[rows] - want[rows]) <= half_ulp + 1e-4 * np.abs(want[rows])).all()
    elif bar == "cold":
        fro = lambda a: np.linalg.norm(a[rows].astype(np.float64) - exact[rows]) / np.linalg.norm(exact[rows])  # noqa: E731
        print(f"{p.name}: sweep gpu {fro(got):.2e} oracle {fro(want):.2e}")
        assert fro(got) < 10.0 * fro(want)
    else:
        raise AssertionError(bar)


@pytest.mark.parametrize("poison", [False, True], ids=["all-solved", "one-row-fails"])
@pytest.mark.parametrize("f", [128, 100])
def test_rows_beyond_the_fp16_range_are_solved_by_the_fp32_kernel(gpu, oracle, f, poison):
    """Hot rows of 300, 600 and 5000 nonzeros (one per normal-matrix kernel) have operands past 65504
    (test_overflow_problem_operands): nm_chol lists them and the workgroup kernel solves them in fp32, at the oracle's own
    distance from float64; the cool rows of the same call meet the plain gate.  With one cool row made not positive definite
    the list holds a row that fails beside rows that do not: the call names exactly that row and still solves the others.

    Measured, gpu vs f64 | oracle vs f64, hot rows of 300 / 600 / 5000 nonzeros, then the worst cool row:
      f = 128:  3.3e-2 | 3.6e-2,  4.0e-2 | 4.1e-2,  8.6e-7 | 8.3e-7;  cool 5.9e-7 | 1.6e-5 (1.6e-5 from the oracle)
      f = 100:  2.2e-2 | 2.1e-2,  2.0e-2 | 2.5e-2,  7.7e-7 | 7.9e-7;  cool 4.4e-7 | 1.5e-5 (1.5e-5 from the oracle)
    (30 and 60 items of weight 1e6 span a subspace of A: a condition number of about 1e5 in fp32 on either side.)"""
    p = cc.overflow_problem(f, poison)
    got, error = call(gpu, p)
    solved = check_untouched(p, got, error)
    want, _, exact = oracle_of(oracle, p)
    check_bar(p, solved, got, want, exact, "oracle2")
    cool = np.array([u for u in solved if u not in p.hot])
    check_bar(p, cool, got, want, exact, "gate")


@functools.lru_cache(maxsize=None)
def _edge_problems(f):
    return cc.edge_problems(f)


@pytest.mark.parametrize("index", range(len(cc.EDGE_NAMES)), ids=cc.EDGE_NAMES)
@pytest.mark.parametrize("f", [128, 100])
def test_operand_edges(gpu, oracle, f, index):
    """The CG cases of tests/test_gpu_nm.py on rows of 1 .. 2100 nonzeros of the Cholesky half sweep, each under its twin's bar.

    The small-* cases at f = 100 measure what the padded route's operand scale costs: the padded gramian's unit diagonal sets
    k = 9 where f = 128 takes 11 .. 12 from the true diagonal (factors of 0.01 .. 1e-4, 9000 item rows, reg 0.01).  It costs
    nothing that can be measured: with the pad in the scale every row is as close to float64 as at f = 128, and closer than the
    fp32 oracle; the library's scale is left as it is.  Measured, worst row of gpu vs f64 | oracle vs f64:
                         f = 128             f = 100 (k with the pad)
      confidence-range   5.0e-4 | 5.8e-4     2.9e-4 | 5.1e-4
      mixed-magnitudes   6.2e-7 | 2.8e-6     6.5e-7 | 2.7e-6
      small-0.01         5.3e-7 | 1.4e-6     4.7e-7 | 1.3e-6     per row at f = 100: 2.9 3.1 3.0 3.5 3.1 4.7 e-7
      small-0.001        4.1e-7 | 1.6e-6     4.1e-7 | 1.3e-6                         3.4 2.8 3.4 3.3 3.5 4.1 e-7
      small-0.0001       3.6e-7 | 6.4e-6     3.8e-7 | 7.0e-6                         2.7 2.8 2.6 3.1 3.2 3.8 e-7
      cold-start (sweep) 6.4e-6 | 5.1e-5     5.8e-6 | 5.3e-5
      reg-zero           5.5e-7 | 1.6e-6     4.8e-7 | 1.2e-6
      fp16-storage       2.3e-4 | 1.4e-6     2.2e-4 | 1.2e-6     (the one fp16 rounding of the result)"""
    p = _edge_problems(f)[index]
    assert p.name == f"{cc.EDGE_NAMES[index]}-f{f}"
    got, error = call(gpu, p)
    rows = check_untouched(p, got, error)
    want, _, exact = oracle_of(oracle, p)
    check_bar(p, rows, got, want, exact, p.bar)
