"""The inputs of the Cholesky half sweep's edge tests (tests/test_gpu_cholesky_edges.py) and the float64 restatement they are
judged by.  tests/test_cholesky_cases_host.py proves on the CPU that every problem is what it claims to be: which rows are not
positive definite and by how much, which rows' matrix-core operands leave the fp16 range, how well conditioned the rest is.
Test infrastructure only; nothing here touches a GPU.

failing_problem: the 19 row lengths of the routes test, the identity as the caller's gramian, reg = 0, and in every row of
`failing` one entry of confidence 0.25 (weight -0.75) on an item row of norm 3 -- an eigenvalue of about 1 - 0.75 * 9.
overflow_problem: confidences of 1e6 on item rows of magnitude 40 in the "hot" rows: the fp16-split operands of nm_build
(csrc/als_cg_nm.hip) leave the fp16 range, nm_chol meets a non-finite pivot, and the row is left to the fp32 workgroup kernel.
edge_problems: the Cholesky twins of the CG cases of tests/test_gpu_nm.py."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

LENGTHS = [0, 1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1100, 2100, 0, 5]  # test_gpu_solver_routes.LENGTHS
COLS, N_POISON, POISON_NORM = 2400, 8, 3.0
EXTRA_ROWS = 3
# {4, 9, 13, 16}: 17, 128, 512 and 2100 nonzeros, one row per length class, the last one cut into segments; the longest row
# alone; and two rows named in descending order (the smaller index still wins)
FAILING_SETS = [(4, 9, 13, 16), (16,), (13, 4)]
# for the matrix held as row blocks: with the 2100-nonzero row a block holds at least 2100 nonzeros, and rows 0 .. 14 hold 2025,
# so the first failing row beyond the first block is row 15 (a block of its own at a limit of 2100; row 16 opens the third)
BLOCK_NNZ, BLOCK_FAILING_SETS = 2100, [(16,), (15, 16), (13, 4)]

OVERFLOW_LENGTHS, OVERFLOW_HOT, OVERFLOW_ITEMS = [40, 300, 512, 600, 2500, 5000], (1, 3, 5), 6000
OVERFLOW_POISON_ROW, OVERFLOW_POISON_NORM = 4, 3000.0
EDGE_LENGTHS = [1, 17, 200, 512, 513, 2100]
EDGE_NAMES = ["confidence-range", "mixed-magnitudes", "small-0.01", "small-0.001", "small-0.0001", "cold-start", "reg-zero",
              "fp16-storage"]
FP16_MAX = 65504.0


def _normal_parts(C, Y, gram, reg):
    """(u, A, b) in float64 for every non-empty row: A = gram + reg I + sum (|c| - 1) y y^T, b = sum_{c > 0} c y
    (implicit/cpu/_als.pyx:75-142)."""
    f = Y.shape[1]
    A0 = np.asarray(gram, np.float64) + float(reg) * np.eye(f)
    Y64 = np.asarray(Y, np.float64)
    for u in range(C.shape[0]):
        lo, hi = C.indptr[u], C.indptr[u + 1]
        if lo == hi:
            continue
        c = C.data[lo:hi].astype(np.float64)
        y = Y64[C.indices[lo:hi]]
        yield u, A0 + (y.T * (np.abs(c) - 1.0)) @ y, (np.where(c > 0, c, 0.0)[:, None] * y).sum(axis=0)


def solve_f64(C, Y, gram, reg):
    """(X64, failing_rows): the Cholesky half sweep in float64 from the fp32 inputs.  A row fails iff np.linalg.cholesky raises
    on its A; failing and empty rows are zero in X64."""
    X = np.zeros((C.shape[0], Y.shape[1]))
    failing = []
    for u, A, b in _normal_parts(C, Y, gram, reg):
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            failing.append(u)
            continue
        X[u] = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return X, failing


def row_spectrum(C, Y, gram, reg):
    """{row: (lambda_min, lambda_max)} of every non-empty row's A in float64."""
    out = {}
    for u, A, _ in _normal_parts(C, Y, gram, reg):
        ev = np.linalg.eigvalsh(A)
        out[u] = (float(ev[0]), float(ev[-1]))
    return out


def row_errors(got, want):
    """Relative distance of every row of `got` from the same row of `want`."""
    num = np.linalg.norm(np.asarray(got, np.float64) - want, axis=1)
    return num / np.maximum(np.linalg.norm(np.asarray(want, np.float64), axis=1), 1e-30)


def oracle_rows(oracle, p):
    """(want, named row or None): oracle.least_squares on the problem's inputs as float32, started from the problem's X0 -- the
    oracle, as the kernels, stores nothing in a failing row."""
    n = p.C.shape[0]
    want = p.X0[:n].astype(np.float32)
    named = None
    try:
        oracle.least_squares(p.C, want, p.Y.astype(np.float32), p.reg, YtY=p.gram)
    except ValueError as e:
        named = int(str(e).split(" on row ")[1].split(".")[0])
    return want, named


def _csr(rows, cols):
    """rows: a list of (column ids, confidences)."""
    indptr = np.concatenate([[0], np.cumsum([len(i) for i, _ in rows])])
    return sp.csr_matrix((np.concatenate([c for _, c in rows]).astype(np.float32),
                          np.concatenate([i for i, _ in rows]).astype(np.int32), indptr), shape=(len(rows), cols))


def _unit_rows(rng, n, f):
    d = rng.standard_normal((n, f))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def failing_problem(f, failing, storage="float32"):
    """C (19 x 2400), Y, X0 (three rows more than C) in `storage`, the identity as gramian, reg 0.  The last N_POISON item rows
    have norm 3; row r of `failing` has one entry of confidence 0.25 on poison item r % 8, in place of an entry that is not the
    row's negated one.  Every other confidence is an integer 1 .. 5, one entry per row of two or more negated (the routes test)."""
    failing = tuple(failing)
    assert len({r % N_POISON for r in failing}) == len(failing) and all(LENGTHS[r] >= 2 for r in failing)
    rng = np.random.default_rng(1000 + f)
    Y = (rng.random((COLS, f), dtype=np.float32) - np.float32(0.5)) * np.float32(0.04)
    first_poison = COLS - N_POISON
    Y[first_poison:] = (POISON_NORM * _unit_rows(rng, N_POISON, f)).astype(np.float32)
    rows = []
    for r, n in enumerate(LENGTHS):
        cols = np.sort(rng.choice(first_poison, size=n, replace=False))
        c = rng.integers(1, 6, size=n).astype(np.float32)
        negated = int(rng.integers(n)) if n >= 2 else -1
        if n >= 2:
            c[negated] *= -1
        if r in failing:
            at = n - 1 if negated != n - 1 else n - 2
            cols[at], c[at] = first_poison + r % N_POISON, 0.25
            order = np.argsort(cols)
            cols, c = cols[order], c[order]
        rows.append((cols, c))
    X0 = rng.random((len(LENGTHS) + EXTRA_ROWS, f), dtype=np.float32) * np.float32(0.2) + np.float32(0.05)
    return SimpleNamespace(name=f"failing-f{f}-{storage}-" + "_".join(map(str, failing)), f=f, storage=storage, C=_csr(rows, COLS),
                           Y=Y.astype(storage), X0=X0.astype(storage), gram=np.eye(f, dtype=np.float32), reg=0.0,
                           failing=failing)


def overflow_problem(f, poison=False):
    """The construction of test_gpu_nm.test_operands_beyond_the_fp16_range_are_resolved_in_fp32 with short rows added: rows of
    40 .. 5000 nonzeros, every tenth item row of magnitude 40, and in the hot rows (300, 600, 5000 nonzeros: the rows kernel, the
    single-segment kernel, the finishing kernel) confidence 1e6 on those items; the cool rows hold them with confidence 1
    (weight 0).  The genuine gramian, in float32 from a float64 sum, reg 0.01.

    poison: the cool 2500-nonzero row also gets confidence 0.25 on one more item row of norm 3000, which the gramian the caller
    hands over does NOT contain (it is the gramian of the other rows): that row is not positive definite."""
    items = OVERFLOW_ITEMS
    rng = np.random.default_rng(2000 + f)
    Y = np.zeros((items + 1, f), np.float32)                # the last row: the poison item (zero unless `poison`)
    Y[:items] = (rng.standard_normal((items, f)) * 0.1).astype(np.float32)
    hot_items = np.arange(0, items, 10)
    Y[hot_items] = (rng.standard_normal((len(hot_items), f)) * 40).astype(np.float32)
    rows = []
    for r, n in enumerate(OVERFLOW_LENGTHS):
        cols = np.sort(rng.choice(items, size=n, replace=False))
        c = (1 + 4 * rng.random(n)).astype(np.float32)
        c[np.isin(cols, hot_items)] = 1e6 if r in OVERFLOW_HOT else 1.0
        rows.append((cols, c))
    gram = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32)
    failing = ()
    if poison:
        Y[items] = (OVERFLOW_POISON_NORM * _unit_rows(rng, 1, f)[0]).astype(np.float32)
        cols, c = rows[OVERFLOW_POISON_ROW]
        cols[-1], c[-1] = items, 0.25                       # the largest column id: still sorted
        failing = (OVERFLOW_POISON_ROW,)
    X0 = rng.random((len(rows) + EXTRA_ROWS, f), dtype=np.float32) + np.float32(0.5)
    return SimpleNamespace(name=f"overflow-f{f}" + ("-poison" if poison else ""), f=f, storage="float32", C=_csr(rows, items + 1),
                           Y=Y, X0=X0, gram=gram, reg=0.01, failing=failing, hot=OVERFLOW_HOT)


def _edge(name, f, items, Y, reg, bar, conf=lambda rng, n: 1 + 4 * rng.random(n), storage="float32", seed=0):
    rng = np.random.default_rng(seed)
    rows = []
    for n in EDGE_LENGTHS:
        rows.append((np.sort(rng.choice(items, size=n, replace=False)), conf(rng, n)))
    Y = Y.astype(np.float32).astype(storage)
    X0 = (rng.random((len(rows) + EXTRA_ROWS, f), dtype=np.float32) + np.float32(0.5)).astype(storage)
    Yf = Y.astype(np.float64)
    return SimpleNamespace(name=f"{name}-f{f}", f=f, storage=storage, C=_csr(rows, items), Y=Y, X0=X0,
                           gram=(Yf.T @ Yf).astype(np.float32), reg=reg, failing=(), bar=bar)


def _confidence_range(rng, n):
    c = 1 + 4 * rng.random(n)
    c[::7] = 1e5 * (1 + rng.random(len(c[::7])))
    c[1::7] = 0.25
    c[2::7] = -3.0
    c[3::7] = 1.0
    return c


def edge_problems(f):
    """The Cholesky twins of the CG cases of tests/test_gpu_nm.py, each on rows of 1, 17, 200, 512, 513 and 2100 nonzeros (the
    rows kernel up to 512, the long-row kernels beyond, the last row in two segments).  `bar` names the rule the GPU test holds
    the case to: "oracle2" max(1e-4, 2 oracle-vs-f64) per row, "gate" 1e-4 per row against the oracle, "fp16" one fp16 rounding
    of the oracle's answer, "bits" max(1e-6, 1.5 oracle-vs-f64) per row, "cold" the sweep within 10 x the oracle's distance."""
    rng = np.random.default_rng(3000 + f)
    normal = lambda items, scale=0.1: rng.standard_normal((items, f)) * scale  # noqa: E731
    out = [
        _edge("confidence-range", f, 8000, normal(8000), 0.01, "oracle2", conf=_confidence_range, seed=9),
        _edge("mixed-magnitudes", f, 6000, normal(6000, 1.0) * 10.0 ** rng.integers(-6, 1, size=(6000, 1)), 0.1, "gate", seed=4),
    ]
    for scale in (0.01, 1e-3, 1e-4):
        out.append(_edge(f"small-{scale:g}", f, 9000, (rng.random((9000, f)) - 0.5) * scale, 0.01, "bits", seed=21))
    out += [
        _edge("cold-start", f, 9000, rng.random((9000, f)) * 0.01, 0.01, "cold", seed=21),
        _edge("reg-zero", f, 6000, normal(6000), 0.0, "gate", seed=5),
        _edge("fp16-storage", f, 7000, normal(7000), 0.05, "fp16", storage="float16", seed=6),
    ]
    return out
