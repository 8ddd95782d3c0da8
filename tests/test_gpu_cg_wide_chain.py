"""The chained launch of the two 1024-thread CG classes -- (256,512], a team of 16 wavefronts per row, and the short rows (1 .. 32
nonzeros), 16 rows per workgroup in lock step -- which fp32 storage takes at f = 128 (als_cg_qfwide_chain_kernel): one
persistent grid of one workgroup per CU, rows and groups of 16 short rows drawn by ticket.

Inputs and gate as in test_gpu_cg_class_chain.py: integer confidences 1 .. 5 with one negated entry per row of two or more
entries, a Y of 2000 rows, an X with three rows more than the matrix, reg = 0.05; relative distance to the CPU oracle below 1e-4
for the sweep and for every non-empty row on its own (float16 storage: the project's 1e-3, against the oracle on the rounded
inputs), rows beyond the matrix bit for bit, empty rows zero, two calls on the same inputs bitwise equal although their ticket
orders differ.

A launch deals the first four tickets of every workgroup out statically (csrc/team_tickets.h): on a 256-CU device these are the
first 1024 rows of (256,512] and the first 1024 groups = 16 384 short rows.  `static` stays below both, `drawn` goes past both.
f = 64 and float16 storage keep their per-class launches and are held to the same checks on the same shapes."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

COLS, EXTRA_ROWS, REG = 2000, 3, 0.05
TOL = {"float32": 1e-4, "float16": 1e-3}
CUTS = [16, 17, 32, 33, 256, 257, 512, 513]
CLASSES = {"team16": (257, 512), "short": (1, 32)}
SHAPES = ["static", "drawn", "team16-only", "short-only", "mod1", "mod15", "few", "early-out"]
WIDE, TEAM16, SHORT = "als_cg_wide_chain_rows", "als_cg_team16_rows", "als_cg_short_rows"


def _lengths(shape):
    """Row lengths of a shape, and which rows are all-negative (their solve ends at rsold < 1e-20)."""
    rng = np.random.default_rng(11)
    draw = lambda n, lo, hi: rng.integers(lo, hi + 1, size=n)
    cuts = np.repeat(CUTS, 2)
    if shape in ("static", "early-out"):
        parts = [draw(6000, 1, 32), draw(600, 257, 512), cuts, [0, 0, 40, 100, 200]]
        if shape == "early-out":
            parts.append(np.full(48, 20))  # with the drawn ones: more than 31 rows of one length, so a whole group of them
    elif shape == "drawn":
        parts = [draw(20000, 1, 32), draw(1300, 257, 512), cuts, [0, 0, 40, 100, 200]]
    elif shape == "team16-only":
        parts = [draw(300, 257, 512), [257, 512, 0]]
    elif shape == "short-only":
        parts = [draw(3000, 1, 32), [1, 16, 17, 32, 0]]
    elif shape in ("mod1", "mod15"):  # the last group of the short class holds 1 / 15 rows
        parts = [draw(16 * 70 + (1 if shape == "mod1" else 15), 1, 32), draw(40, 257, 512), [0, 64]]
    elif shape == "few":  # fewer rows / groups than queues in both classes
        parts = [[300, 512, 257, 400, 480], draw(16 * 2 + 5, 1, 32), [0]]
    else:
        raise ValueError(shape)
    lengths = np.concatenate(parts).astype(np.int64)
    rng.shuffle(lengths)
    negative = np.zeros(len(lengths), dtype=bool)
    if shape == "early-out":  # every 9th row of both classes, the rows at their ends, and every row of 20 nonzeros
        for lo, hi in CLASSES.values():
            rows = np.flatnonzero((lengths >= lo) & (lengths <= hi))
            negative[rows[::9]] = True
            negative[rows[(lengths[rows] == lo) | (lengths[rows] == hi)][:2]] = True
        negative[lengths == 20] = True
    return lengths, negative


def short_groups(lengths):
    """Schedule positions of the short class cut into its groups of 16: rows by descending length, ascending id within one."""
    order = np.argsort(-lengths, kind="stable")
    order = order[(lengths[order] >= 1) & (lengths[order] <= 32)]
    return [order[k:k + 16] for k in range(0, len(order), 16)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, f, storage="float32"):
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
    X0, Y0 = X0.astype(storage), Y0.astype(storage)
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


def launches(gpu, name, C, X0, Y0, steps=3):
    """One half sweep with the library profiler filtered to `name` (a filtered profiler leaves the routes as they are):
    (result, launches under that scope)."""
    gpu.Profiler.reset()
    gpu.Profiler.enable(True, only=name)
    try:
        got, _ = solve(gpu, C, X0, Y0, steps)
        count = gpu.Profiler.get(name)[1]
    finally:
        gpu.Profiler.enable(False)
        gpu.Profiler.reset()
    return got, count


_GOT, _WANT = {}, {}


def solved(gpu, shape, f, steps, storage="float32"):
    """Two consecutive half sweeps on the same inputs, computed once per case: (first, second, gramian)."""
    key = (shape, f, steps, storage)
    if key not in _GOT:
        C, X0, Y0, _ = _inputs(shape, f, storage)
        first, gram = solve(gpu, C, X0, Y0, steps)
        second, _ = solve(gpu, C, X0, Y0, steps)
        for a in (first, second, gram):
            a.setflags(write=False)
        _GOT[key] = (first, second, gram)
    return _GOT[key]


def expected(oracle, shape, f, steps, storage, gram):
    key = (shape, f, steps, storage)
    if key not in _WANT:
        C, X0, Y0, _ = _inputs(shape, f, storage)
        want = X0[: C.shape[0]].astype(np.float32)
        oracle.least_squares_cg(C, want, Y0.astype(np.float32), REG, cg_steps=steps, YtY=gram)
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def check(gpu, oracle, shape, f, steps=3, storage="float32"):
    C, X0, _, negative = _inputs(shape, f, storage)
    got, again, gram = solved(gpu, shape, f, steps, storage)
    want = expected(oracle, shape, f, steps, storage, gram)
    n = C.shape[0]
    lens = np.diff(C.indptr)
    word = np.uint32 if storage == "float32" else np.uint16
    assert got.dtype == X0.dtype and got.shape == X0.shape
    np.testing.assert_array_equal(got[n:].view(word), X0[n:].view(word))  # rows beyond the matrix: untouched, bit for bit
    assert not got[:n][lens == 0].any()  # empty rows: zero
    np.testing.assert_array_equal(got.view(word), again.view(word))  # whatever the ticket order
    assert np.isfinite(want).all()
    # an all-negative row with x0 = 0 has a zero residual: the oracle leaves it at zero, and so must the kernel, exactly
    assert not want[negative].any() and not got[:n][negative].any()
    rows = (lens > 0) & ~negative
    diff = np.linalg.norm(got[:n].astype(np.float64) - want, axis=1)
    norm = np.linalg.norm(want.astype(np.float64), axis=1)
    per_row = diff[rows] / np.maximum(norm[rows], 1e-30)
    whole = float(np.linalg.norm(diff) / max(np.linalg.norm(norm), 1e-30))
    print(f"{shape}-f{f}-{storage}-steps{steps}: sweep {whole:.2e}, worst row {per_row.max():.2e} (nnz {lens[rows][per_row.argmax()]})")
    assert whole < TOL[storage], (shape, f, storage, steps, whole)
    assert (per_row < TOL[storage]).all(), (shape, f, storage, steps, float(per_row.max()), int(lens[rows][per_row.argmax()]))


def test_shapes_are_what_they_claim():
    """No GPU work: the class sizes the cases are named for."""
    count = lambda shape, name: int(((_lengths(shape)[0] >= CLASSES[name][0]) & (_lengths(shape)[0] <= CLASSES[name][1])).sum())
    assert 8 <= count("static", "team16") <= 1024 and 8 * 16 <= count("static", "short") <= 16384
    assert count("drawn", "team16") > 1024 and count("drawn", "short") > 16384
    assert count("team16-only", "short") == 0 and count("short-only", "team16") == 0
    assert count("mod1", "short") % 16 == 1 and count("mod15", "short") % 16 == 15
    assert 0 < count("few", "team16") < 8 and 0 < -(-count("few", "short") // 16) < 8
    for cut in CUTS:
        assert (_lengths("static")[0] == cut).sum() >= 2
    lengths, negative = _lengths("early-out")
    groups = short_groups(lengths)
    full = [g for g in groups if negative[g].all()]
    mixed = [g for g in groups if negative[g].any() and not negative[g].all()]
    assert full and len(full[0]) == 16 and len(mixed) > 100  # a whole group of early exits, and many scattered ones
    assert negative[(lengths >= 257) & (lengths <= 512)].sum() > 50


@pytest.mark.parametrize("shape", SHAPES)
def test_wide_chain_parity(gpu, oracle, shape):
    check(gpu, oracle, shape, 128)


@pytest.mark.parametrize("steps", [0, 1, 3])
def test_wide_chain_cg_steps(gpu, oracle, steps):
    check(gpu, oracle, "mod15", 128, steps)


@pytest.mark.parametrize("f,storage", [(64, "float32"), (128, "float16"), (64, "float16")])
@pytest.mark.parametrize("shape", SHAPES)
def test_other_routes_parity(gpu, oracle, shape, f, storage):
    check(gpu, oracle, shape, f, 3, storage)


@pytest.mark.parametrize("f,storage,chained", [(128, "float32", True), (64, "float32", False), (128, "float16", False),
                                               (64, "float16", False)])
def test_routes(gpu, f, storage, chained):
    """fp32 storage at f = 128 takes the chain; f = 64 and float16 storage keep the launch per class."""
    C, X0, Y0, _ = _inputs("mod1", f, storage)
    word = np.uint32 if storage == "float32" else np.uint16
    plain = solved(gpu, "mod1", f, 3, storage)[0]
    for name, want in ((WIDE, chained), (SHORT, not chained)):
        got, count = launches(gpu, name, C, X0, Y0)
        assert (count > 0) == want, (name, count)
        np.testing.assert_array_equal(got.view(word), plain.view(word))
    if storage == "float32":  # (float16 storage runs (256,512] on the packed tiles, under the same scope name)
        assert (launches(gpu, TEAM16, C, X0, Y0)[1] > 0) == (not chained)


@pytest.mark.parametrize("name", list(CLASSES))
@pytest.mark.parametrize("shape", ["static", "drawn"])
def test_class_alone_is_bitwise_equal(gpu, shape, name):
    """The rows of one class in a matrix of their own -- the chain with the other class empty -- against the same rows in the
    full matrix: neither the company nor the order in which a row is solved may show in its bits.  (The short rows keep their
    schedule order, hence their groups.)"""
    C, X0, Y0, _ = _inputs(shape, 128)
    full = solved(gpu, shape, 128, 3)[0]
    lens = np.diff(C.indptr)
    lo, hi = CLASSES[name]
    rows = np.flatnonzero((lens >= lo) & (lens <= hi))
    assert len(rows) > 500 and lens[rows].min() == lo and lens[rows].max() == hi
    alone, _ = solve(gpu, C[rows], np.concatenate([X0[rows], X0[-EXTRA_ROWS:]]), Y0, 3)
    np.testing.assert_array_equal(alone[: len(rows)].view(np.uint32), full[rows].view(np.uint32))
    np.testing.assert_array_equal(alone[len(rows):], X0[-EXTRA_ROWS:])


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_equals_per_class_launches(gpu, shape):
    """The chained run against the per-class launches, which the library profiler with no name filter forces: bitwise equal."""
    C, X0, Y0, _ = _inputs(shape, 128)
    chained = solved(gpu, shape, 128, 3)[0]
    gpu.Profiler.reset()
    gpu.Profiler.enable(True)
    try:
        per_class, _ = solve(gpu, C, X0, Y0, 3)
        scopes = {n for n in gpu.Profiler.names() if gpu.Profiler.get(n)[1] > 0}
    finally:
        gpu.Profiler.enable(False)
        gpu.Profiler.reset()
    assert WIDE not in scopes and (TEAM16 in scopes or SHORT in scopes)
    np.testing.assert_array_equal(per_class.view(np.uint32), chained.view(np.uint32))
