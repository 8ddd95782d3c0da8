"""The chained launch of the three 512-thread CG classes -- (128,256], (64,128], (32,64], team widths 8, 4, 2 -- which fp32
storage takes at f = 128 (als_cg_qfteam_chain_kernel): one persistent grid, the gramian staged once, rows drawn by ticket.

Inputs as in test_gpu_solver_routes.py: integer confidences 1 .. 5 with one negated entry per row of two or more entries, a
Y of 2000 rows, an X with three rows more than the matrix, reg = 0.05.  Every case is held to the project's parity gate
against the CPU oracle -- relative distance below 1e-4 for the sweep and for every non-empty row on its own -- rows beyond
the matrix come back bit for bit, empty rows are zero, and two calls on the same inputs agree bit for bit although their
ticket orders differ.

A launch deals the first four tickets of every team out statically (csrc/team_tickets.h): on a 256-CU device the grid holds
512 / 1024 / 2048 teams of width 8 / 4 / 2, so the shapes the chain was specified with (`several`: 1200 / 2500 / 5000 rows) are
served by static tickets alone and `drawn` (2300 / 4500 / 9000 rows: more than four per team) is the one in which tickets are
drawn from the device counters as well.  f = 64 keeps its per-class launches and is held to the same checks."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

COLS, EXTRA_ROWS, REG, TOL = 2000, 3, 0.05, 1e-4
CUTS = [32, 33, 64, 65, 128, 129, 256, 257]
CLASSES = {"team8": (129, 256), "team4": (65, 128), "team2": (33, 64)}


def _lengths(shape):
    """Row lengths of a shape, and which rows are all-negative (their solve ends at rsold < 1e-20)."""
    rng = np.random.default_rng(7)
    draw = lambda n, lo, hi: rng.integers(lo, hi + 1, size=n)
    if shape in ("several", "no-team4", "early-out", "fifth", "drawn"):
        n2, n4, n8 = {"fifth": (1000, 500, 240), "drawn": (9000, 4500, 2300)}.get(shape, (5000, 2500, 1200))
        if shape == "no-team4":
            n4 = 0
        parts = [draw(n2, 33, 64), draw(n4, 65, 128), draw(n8, 129, 256), np.repeat(CUTS, 2), [0, 0, 5]]
        if shape == "no-team4":
            parts[3] = np.repeat([32, 33, 64, 129, 256, 257], 2)
        lengths = np.concatenate(parts).astype(np.int64)
        rng.shuffle(lengths)
    elif shape == "seven":
        lengths = np.array([33, 64, 40, 0, 51, 47, 63, 34], dtype=np.int64)
    else:
        raise ValueError(shape)
    negative = np.zeros(len(lengths), dtype=bool)
    if shape == "early-out":  # every 9th row of every class, the rows at the cuts included
        for lo, hi in CLASSES.values():
            rows = np.flatnonzero((lengths >= lo) & (lengths <= hi))
            negative[rows[::9]] = True
            negative[rows[(lengths[rows] == lo) | (lengths[rows] == hi)][:2]] = True
    return lengths, negative


@functools.lru_cache(maxsize=None)
def _inputs(shape, f):
    lengths, negative = _lengths(shape)
    rng = np.random.default_rng(len(lengths) + f)
    indices, data = [], []
    for n, neg in zip(lengths, negative):
        indices.append(np.sort(rng.choice(COLS, size=n, replace=False)))
        c = rng.integers(1, 6, size=n).astype(np.float32)
        if neg:
            c = -c
        elif n >= 2:
            c[rng.integers(n)] *= -1
        data.append(c)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    C = sp.csr_matrix((np.concatenate(data), np.concatenate(indices).astype(np.int32), indptr), shape=(len(lengths), COLS))
    X0 = rng.random((C.shape[0] + EXTRA_ROWS, f), dtype=np.float32) * 0.2 - 0.1
    X0[: C.shape[0]][negative] = 0.0
    Y0 = rng.random((COLS, f), dtype=np.float32) * 0.2 - 0.1
    for a in (X0, Y0):
        a.setflags(write=False)
    return C, X0, Y0, negative


def solve(gpu, C, X0, Y0, steps):
    solver = gpu.LeastSquaresSolver()
    f = X0.shape[1]
    Xd, Yd, gram = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix.zeros(f, f)
    solver.calculate_yty(Yd, gram, REG)
    solver.least_squares(gpu.CSRMatrix(C), Xd, gram, Yd, steps)
    return Xd.to_numpy(), gram.to_numpy()


_GOT, _WANT = {}, {}


def solved(gpu, shape, f, steps):
    """Two consecutive half sweeps on the same inputs, computed once per case: (first, second, gramian)."""
    key = (shape, f, steps)
    if key not in _GOT:
        C, X0, Y0, _ = _inputs(shape, f)
        first, gram = solve(gpu, C, X0, Y0, steps)
        second, _ = solve(gpu, C, X0, Y0, steps)
        for a in (first, second, gram):
            a.setflags(write=False)
        _GOT[key] = (first, second, gram)
    return _GOT[key]


def expected(oracle, shape, f, steps, gram):
    key = (shape, f, steps)
    if key not in _WANT:
        C, X0, Y0, _ = _inputs(shape, f)
        want = X0[: C.shape[0]].copy()
        oracle.least_squares_cg(C, want, Y0, REG, cg_steps=steps, YtY=gram)
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def check(gpu, oracle, shape, f, steps=3):
    C, X0, _, negative = _inputs(shape, f)
    got, again, gram = solved(gpu, shape, f, steps)
    want = expected(oracle, shape, f, steps, gram)
    n = C.shape[0]
    lens = np.diff(C.indptr)
    assert got.dtype == np.float32 and got.shape == X0.shape
    np.testing.assert_array_equal(got[n:], X0[n:])  # rows beyond the matrix: untouched, bit for bit
    assert not got[:n][lens == 0].any()  # empty rows: zero
    np.testing.assert_array_equal(got.view(np.uint32), again.view(np.uint32))  # whatever the ticket order
    assert np.isfinite(want).all()
    # an all-negative row with x0 = 0 has a zero residual: the oracle leaves it at zero, and so must the kernel, exactly
    assert not want[negative].any() and not got[:n][negative].any()
    rows = (lens > 0) & ~negative
    diff = np.linalg.norm(got[:n].astype(np.float64) - want, axis=1)
    norm = np.linalg.norm(want.astype(np.float64), axis=1)
    per_row = diff[rows] / np.maximum(norm[rows], 1e-30)
    whole = float(np.linalg.norm(diff) / max(np.linalg.norm(norm), 1e-30))
    print(f"{shape}-f{f}-steps{steps}: sweep {whole:.2e}, worst row {per_row.max():.2e} (nnz {lens[rows][per_row.argmax()]})")
    assert whole < TOL, (shape, f, steps, whole)
    assert (per_row < TOL).all(), (shape, f, steps, float(per_row.max()), int(lens[rows][per_row.argmax()]))


@pytest.mark.parametrize("shape,f", [("several", 128), ("several", 64), ("no-team4", 128), ("seven", 128), ("early-out", 128),
                                     ("drawn", 128)], ids=lambda v: str(v))
def test_chain_parity(gpu, oracle, shape, f):
    if shape == "early-out":
        assert _inputs(shape, f)[3].sum() > 300
    check(gpu, oracle, shape, f)


@pytest.mark.parametrize("steps", [0, 1, 3])
def test_chain_cg_steps(gpu, oracle, steps):
    check(gpu, oracle, "fifth", 128, steps)


@pytest.mark.parametrize("name", list(CLASSES))
@pytest.mark.parametrize("shape", ["several", "drawn"])
def test_class_alone_is_bitwise_equal(gpu, shape, name):
    """The rows of one class in a matrix of their own -- the chain with the other two classes empty -- against the same rows
    in the full matrix: neither the company nor the order in which a row is solved may show in its bits."""
    C, X0, Y0, _ = _inputs(shape, 128)
    full = solved(gpu, shape, 128, 3)[0]
    lens = np.diff(C.indptr)
    lo, hi = CLASSES[name]
    rows = np.flatnonzero((lens >= lo) & (lens <= hi))
    assert len(rows) > 1000 and lens[rows].min() == lo and lens[rows].max() == hi
    alone, _ = solve(gpu, C[rows], np.concatenate([X0[rows], X0[-EXTRA_ROWS:]]), Y0, 3)
    np.testing.assert_array_equal(alone[: len(rows)].view(np.uint32), full[rows].view(np.uint32))
    np.testing.assert_array_equal(alone[len(rows):], X0[-EXTRA_ROWS:])
