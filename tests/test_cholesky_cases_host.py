"""What tests/test_gpu_cholesky_edges.py relies on, proved on the CPU: the problems of tests/cholesky_cases.py fail where they say
they fail and nowhere else, their good rows are well conditioned, the float64 restatement and the oracle agree, the hot rows of
the overflow problem do leave the fp16 range and the cool rows do not, and every edge problem is positive definite."""
import numpy as np
import pytest

import cholesky_cases as cc
import test_gpu_solver_routes as routes
from test_nm_split_model import operand_scale, root_products

FACTORS = [16, 48, 64, 100, 128, 200, 320]
ALL_FAILING_SETS = cc.FAILING_SETS + [s for s in cc.BLOCK_FAILING_SETS if s not in cc.FAILING_SETS]


def test_the_lengths_are_those_of_the_routes_test():
    assert cc.LENGTHS == routes.LENGTHS and cc.COLS == routes.COLS and cc.EXTRA_ROWS == routes.EXTRA_ROWS


@pytest.mark.parametrize("failing", ALL_FAILING_SETS, ids=str)
@pytest.mark.parametrize("f", FACTORS)
def test_failing_problems_fail_where_they_say(oracle, f, failing):
    """Failing rows: lambda_min <= -1.  Every other row: lambda_min >= 0.5 and a condition number of at most 10.  The float64
    restatement and the fp32 oracle both fail on exactly these rows, the oracle names the smallest, and the oracle's good rows
    are within 1e-5 of float64 while its failing rows keep what they held."""
    for storage in ("float32", "float16") if f in (64, 128) else ("float32",):
        p = cc.failing_problem(f, failing, storage)
        lens = np.diff(p.C.indptr)
        assert lens.tolist() == cc.LENGTHS and p.X0.shape == (len(cc.LENGTHS) + cc.EXTRA_ROWS, f) and p.X0.all()
        assert p.Y.dtype == p.X0.dtype == np.dtype(storage)
        Y32 = p.Y.astype(np.float32)
        spectrum = cc.row_spectrum(p.C, Y32, p.gram, p.reg)
        assert sorted(spectrum) == np.flatnonzero(lens).tolist()
        for u, (lo, hi) in spectrum.items():
            if u in failing:
                assert lo <= -1.0, (u, lo)
            else:
                assert lo >= 0.5 and hi / lo <= 10.0, (u, lo, hi)
        exact, failed = cc.solve_f64(p.C, Y32, p.gram, p.reg)
        assert failed == sorted(failing)
        want, named = cc.oracle_rows(oracle, p)
        assert named == min(failing)
        good = np.array([u for u in spectrum if u not in failing])
        assert cc.row_errors(want[good], exact[good]).max() < 1e-5
        bad = np.array(sorted(failing))
        np.testing.assert_array_equal(want[bad], p.X0[bad].astype(np.float32))
        assert not want[lens == 0].any()
        print(p.name, "lambda_min of the failing rows", [round(spectrum[u][0], 2) for u in sorted(failing)],
              "worst good row: lambda_min %.2f, condition %.2f" % (min(spectrum[u][0] for u in good),
                                                                   max(spectrum[u][1] / spectrum[u][0] for u in good)))


def test_block_limit_puts_the_failing_rows_in_three_blocks():
    """The greedy cut of imp_csr_create64 (`while (r1 < rows && indptr[r1 + 1] - indptr[r0] <= part_limit) ++r1;`) at
    BLOCK_NNZ: rows 0 .. 14, row 15, rows 16 .. 17, row 18."""
    indptr = np.concatenate([[0], np.cumsum(cc.LENGTHS)])
    starts, r0 = [], 0
    while r0 < len(cc.LENGTHS):
        r1 = r0
        while r1 < len(cc.LENGTHS) and indptr[r1 + 1] - indptr[r0] <= cc.BLOCK_NNZ:
            r1 += 1
        assert r1 > r0
        starts.append(r0)
        r0 = r1
    assert starts == [0, 15, 16, 18]


@pytest.mark.parametrize("f", [48, 128])
def test_solve_f64_agrees_with_the_oracle_on_a_benign_problem(oracle, f):
    C, X0, Y0 = routes._inputs(f, "float32", "all")
    Yf = Y0.astype(np.float64)
    gram = (Yf.T @ Yf).astype(np.float32)
    exact, failed = cc.solve_f64(C, Y0, gram, routes.REG)
    assert failed == []
    want = np.zeros((C.shape[0], f), np.float32)
    oracle.least_squares(C, want, Y0, routes.REG, YtY=gram)
    lens = np.diff(C.indptr)
    assert cc.row_errors(want[lens > 0], exact[lens > 0]).max() < 1e-5
    assert not exact[lens == 0].any() and not want[lens == 0].any()


def max_operand(C, Y, k):
    """Per row: the largest |z| = sqrt(4^k |w|) |y| over the row's entries, the value root_products splits into fp16 halves."""
    out = np.zeros(C.shape[0])
    for u in range(C.shape[0]):
        lo, hi = C.indptr[u], C.indptr[u + 1]
        w = (np.abs(C.data[lo:hi]) - np.float32(1.0)) * np.float32(4.0 ** k)
        out[u] = (np.sqrt(np.abs(w)).astype(np.float32)[:, None] * np.abs(Y[C.indices[lo:hi]])).max()
    return out


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("f", [100, 128])
def test_overflow_problem_operands(f, poison):
    """A condition on the inputs alone: at the launch's operand scale (f = 100: the scale the padded gramian's unit diagonal
    gives) every hot row has an operand above 65504 -- and a non-finite product of fp16 halves -- and every cool row, the
    poisoned one included, stays below half of that and keeps every product finite."""
    p = cc.overflow_problem(f, poison)
    assert np.diff(p.C.indptr).tolist() == cc.OVERFLOW_LENGTHS
    diag = float(np.diag(p.gram).max())
    k = operand_scale(np.float32(max(diag, 1.0) if f < 128 else diag) + np.float32(p.reg), p.Y.shape[0])
    biggest = max_operand(p.C, p.Y, k)
    print(p.name, "k", k, "largest operand per row", biggest)
    for u in range(p.C.shape[0]):
        lo, hi = p.C.indptr[u], p.C.indptr[u + 1]
        w = np.abs(p.C.data[lo:hi]) - np.float32(1.0)
        y = p.Y[p.C.indices[lo:hi]]
        with np.errstate(over="ignore", invalid="ignore"):
            squares = root_products(w[:, None], y, y, k)     # the diagonal contributions of every entry
        if u in p.hot:
            assert biggest[u] > cc.FP16_MAX and not np.isfinite(squares).all()
        else:
            assert biggest[u] < cc.FP16_MAX / 2 and np.isfinite(squares).all()
    spectrum = cc.row_spectrum(p.C, p.Y, p.gram, p.reg)
    for u, (lo, hi) in spectrum.items():
        assert (lo <= -1.0) if u in p.failing else (lo > 0), (u, lo, hi)
    assert cc.solve_f64(p.C, p.Y, p.gram, p.reg)[1] == list(p.failing)


@pytest.mark.parametrize("f", [100, 128])
def test_edge_problems_are_positive_definite(f):
    problems = cc.edge_problems(f)
    assert len(problems) == 8 and {p.bar for p in problems} == {"oracle2", "gate", "bits", "cold", "fp16"}
    for p in problems:
        assert np.diff(p.C.indptr).tolist() == cc.EDGE_LENGTHS
        Y32 = p.Y.astype(np.float32)
        spectrum = cc.row_spectrum(p.C, Y32, p.gram, p.reg)
        assert len(spectrum) == len(cc.EDGE_LENGTHS)
        print(p.name, "condition numbers", ["%.1e" % (hi / lo) for lo, hi in spectrum.values()])
        assert all(lo > 0 for lo, _ in spectrum.values())
        exact, failed = cc.solve_f64(p.C, Y32, p.gram, p.reg)
        assert failed == [] and np.isfinite(exact).all() and (np.linalg.norm(exact, axis=1) > 0).all()
