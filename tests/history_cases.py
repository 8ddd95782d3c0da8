"""Probes and predecessors of tests/test_gpu_call_history.py: does an entry point's answer depend on the calls before it?
tests/test_history_cases_host.py proves on the CPU that the inputs are what they claim to be.  Test infrastructure only; nothing
here touches a GPU at import.

A PROBE is a named small call with fixed inputs, built from the case modules the kernel families already have, with their
references and their bars: run(gpu) returns every array the call can write (outputs, the rows of X beyond the matrix, Y and the
gramian it was handed, the failed row where there is one) as a dict of numpy arrays, gate(gpu, oracle, out) holds them to the
bar of the probe's own test file, reference(oracle) is that file's expected answer computed without a device.  `exact`: the
same inputs give the same bytes every time -- true for everything here; `why` says what was read to know it ("State
kept between calls").  No number in this file is a tolerance of its own.  Where the owning file keeps its bar in a constant or a
function, that is imported (routes.TOL, chain.TOL, test_gpu_subspace.judge, test_gpu_explain.check, test_gpu_topk_routes.judge,
test_gpu_ease.FLOOR, test_gpu_eval.check_sums, lmf_reference.within, svd_reference.multiply_bound).  Three owners write their bar
inline in a test body, which cannot be imported and may not be edited here; the anchors of three probes restate those
expressions word for word, and they have to follow if the owner ever changes: d_gpu <= max(2 d_ref, FLOOR)
(test_gpu_ease.test_spd_inverse_accuracy, in _spd_gate), |s - s64| <= width 2^-23 m (test_gpu_rank.test_scores_against_float64,
in _rank_gate) and rtol = K 2^-52 (test_gpu_eval.test_kernel_equals_numpy, in _eval_gate).  The cells compare bytes only.

A PREDECESSOR is what runs immediately before the probe: PREDECESSORS[name](gpu, probe), or "cross:<probe>" -- another probe
that shares a piece of scratch with this one.  probe.before lists the predecessors of a probe.

SEQUENCES: about a dozen half sweeps on one solver over matrices whose class counts sit on both sides of the static-ticket cut
of csrc/team_tickets.h, then the probe."""
import functools
import hashlib
import json
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import cholesky_cases as cc
import dense_reference as dref
import ease_reference as eref
import evaluation_reference as evref
import explain_cases as xc
import ivf_cases as ic
import knn_cases as kc
import knn_reference as kr
import lmf_reference as lref
import rank_cases as rc
import rank_reference as rref
import sgd_cases as sgd
import subspace_cases as sc
import svd_reference as sref
import warp_reference as wref

FLT_MAX = rref.FLT_MAX
SCALE = 64.0  # the `bigger` predecessors' factors: another seed, 64 times the magnitude
PRIMES = np.array([7, 11, 13, 17, 19, 23, 29, 31])  # coprime to 2000, 2400 and 6000: (start + p t) mod cols never repeats

# schedule classes of csrc/common.h (imp_csr), by the name a probe uses for them -> index into bin_start
CLASS_BINS = {"long": 0, "team16": 1, "team8": 2, "team4": 3, "team2": 4, "short32": 5, "short16": 6, "empty": 7}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def digest(out):
    """sha256 over the arrays of a probe's answer in key order, their names, dtypes and shapes included."""
    h = hashlib.sha256()
    for key in sorted(out):
        a = np.ascontiguousarray(out[key])
        h.update(f"{key}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def differing(a, b):
    """The keys whose bytes differ between two answers of a probe, with the first differing position of each (a key one answer
    lacks -- the outputs of a call that was refused -- differs too)."""
    out = {key: "only in the " + ("first" if key in a else "second") + " answer" for key in set(a) ^ set(b)}
    for key in sorted(set(a) & set(b)):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.shape != y.shape or x.dtype != y.dtype:
            out[key] = f"{x.dtype}{x.shape} against {y.dtype}{y.shape}"
        elif x.tobytes() != y.tobytes():
            raw = np.flatnonzero(np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8))
            at = np.unravel_index(int(raw[0]) // x.dtype.itemsize, x.shape) if x.ndim else ()
            out[key] = f"{len(raw)} bytes differ, first at {tuple(int(i) for i in at)}: {x[at]!r} against {y[at]!r}"
    return out


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def fast_matrix(lengths, cols, seed, integer=True):
    """Rows of the given lengths without a per-row draw: row r holds the columns (start_r + p_r t) mod cols, t < n_r, sorted;
    confidences are integers 1 .. 5 (or uniform in [1, 40)) and the first stored entry of every row of two or more is negated,
    as in the case modules."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.max(initial=0) <= cols
    rng = np.random.default_rng(seed)
    start, step = rng.integers(0, cols, len(lengths)), PRIMES[rng.integers(0, len(PRIMES), len(lengths))]
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    row = np.repeat(np.arange(len(lengths)), lengths)
    t = np.arange(indptr[-1]) - indptr[row]
    col = (start[row] + step[row] * t) % cols
    order = np.lexsort((col, row))
    data = rng.integers(1, 6, len(col)).astype(np.float32) if integer else (1 + 39 * rng.random(len(col))).astype(np.float32)
    first = indptr[:-1][lengths >= 2]
    data[first] *= -1
    return sp.csr_matrix((data, col[order].astype(np.int32), indptr.astype(np.int32)), shape=(len(lengths), cols))


def class_counts(m, num_cus=256):
    """{class name: rows} of a matrix under the schedule CSRMatrix builds (imp_host_csr_plan, host code), with "chol_long" (rows
    of the f = 64 Cholesky's segment plan), "nm_multi" (rows the normal-matrix plan cuts into several segments) and "sub_long"
    (rows of the subspace sweep's segment kernels: the same plan as chol_long)."""
    from implicit_amd.utils import csr_schedule

    p = csr_schedule(m, 2, num_cus=num_cus)
    b = p["bin_start"]
    out = {name: int(b[i + 1] - b[i]) for name, i in CLASS_BINS.items()}
    out["chol_long"] = out["sub_long"] = int(p["n_chol_long"])
    out["nm_multi"] = int(p["nm_multi_rows"])
    return out


# ---- the probe table --------------------------------------------------------------------------------------------------------------
# the predecessors every probe has after its own: the workspaces released, the block pool under each loud pattern
ALWAYS = ("released", "pool_nan", "pool_finite", "released_pool_nan")
PROBES = {}


def add(name, family, owner, run, gate, reference, before, why, size, bigger_size, matrix=None, classes=(), exact=True):
    """size / bigger_size: callables giving (rows, nonzeros or elements) of the probe's and of its `bigger` predecessor's input."""
    assert name not in PROBES
    PROBES[name] = SimpleNamespace(name=name, family=family, owner=owner, run=run, gate=gate, reference=reference, before=tuple(before),
                                   why=why, exact=exact, size=size, bigger_size=bigger_size, matrix=matrix, classes=tuple(classes))


def _sizes(m):
    return int(m.shape[0]), int(m.nnz)


# =================================================================================================================================
# 1. gramian and loss (gram_ws, loss_buf)
# =================================================================================================================================
GRAM_REG = 0.25  # test_gpu_dense.REG
GRAM_SHAPES = {"splitk": {64: 529, 100: 3001}, "single": {64: 25, 100: 17}}  # 3 / 12 chunks against one (gramian_t, 256 CUs)
GRAM_BIGGER_ROWS = dref.VEC_ROWS_56_CHUNKS


def _gramian(gpu, y, reg):
    f = y.shape[1]
    yd, out = gpu.Matrix(y), gpu.Matrix.zeros(f, f)
    gpu.LeastSquaresSolver().calculate_yty(yd, out, reg)
    return {"gram": out.to_numpy(), "Y": yd.to_numpy()}


def _add_gramian(route, f):
    n = GRAM_SHAPES[route][f]
    y = functools.lru_cache(maxsize=None)(lambda: dref.int_factors(n, f, seed=4))

    def gate(gpu, oracle, out):
        want = dref.gramian_exact(y(), GRAM_REG)  # zero tolerance: test_gpu_dense._check_exact
        assert np.array_equal(out["gram"], want) and bits(out["Y"]) == bits(y())

    name = f"gramian-{route}-f{f}"
    add(name, "gramian", "gram_ws", lambda gpu: _gramian(gpu, y(), GRAM_REG), gate, lambda oracle: [dref.gramian_exact(y(), GRAM_REG)],
        ["quiet", "bigger", "other_width", "cross:loss", "refused_args", *ALWAYS],
        "gramian.hip: partial tiles per chunk, reduced in a fixed order by gramian_reduce_kernel; no atomics", lambda: (n, n * f),
        lambda: (GRAM_BIGGER_ROWS, GRAM_BIGGER_ROWS * f))


def _gramian_bigger(gpu, p):
    f = p.extra["f"]
    _gramian(gpu, dref.int_factors(GRAM_BIGGER_ROWS, f, seed=5) * np.float32(SCALE), 1.0)


def _gramian_other_width(gpu, p):
    f = {64: 128, 100: 320}[p.extra["f"]]  # another tile layout of gram_ws: the vector kernels' / the generic kernel's
    _gramian(gpu, dref.int_factors(dref.GENERIC_ROWS_66_CHUNKS, f, seed=6) * np.float32(SCALE), 1.0)


def _gramian_refused(gpu, p):
    y, out_shape = p.extra["refused_args_operands"]()
    return lambda: gpu.LeastSquaresSolver().calculate_yty(gpu.Matrix(y), gpu.Matrix.zeros(*out_shape), 0.0)


for _route in GRAM_SHAPES:
    for _f in (64, 100):
        _add_gramian(_route, _f)
        PROBES[f"gramian-{_route}-f{_f}"].extra = {"f": _f, "bigger": _gramian_bigger, "other_width": _gramian_other_width,
                                                   "refused_args": _gramian_refused,
                                                   "refused_args_operands": lambda _f=_f: (dref.int_factors(9, _f), (_f + 1, _f + 1)),
                                                   "refused_args_reason": "YtY has one column more than Y"}

LOSS_F = 129


@functools.lru_cache(maxsize=None)
def _loss_problem(users=dref.LOSS_USERS, items=dref.LOSS_ITEMS):
    return dref.loss_problem(users, items, LOSS_F)


def _loss(gpu, c, x, y, reg=dref.LOSS_REG):
    xd, yd = gpu.Matrix(x), gpu.Matrix(y)
    loss = gpu.LeastSquaresSolver().calculate_loss(gpu.CSRMatrix(c), xd, yd, reg)
    return {"loss": np.array([loss], dtype=np.float32), "X": xd.to_numpy(), "Y": yd.to_numpy()}


def _loss_gate(gpu, oracle, out):
    c, x, y = _loss_problem()
    assert out["loss"][0] == dref.loss_ref(c, x, y, dref.LOSS_REG), out["loss"]  # test_gpu_dense.test_loss_exact: equality
    assert bits(out["X"]) == bits(x) and bits(out["Y"]) == bits(y)


def _loss_bigger(gpu, p):
    c, x, y = _loss_problem(4 * dref.LOSS_USERS, 4 * dref.LOSS_ITEMS)
    _loss(gpu, c, x * np.float32(SCALE), y * np.float32(SCALE))


add("loss", "loss", "loss_buf, gram_ws", lambda gpu: _loss(gpu, *_loss_problem()), _loss_gate,
    lambda oracle: [np.array([dref.loss_ref(*_loss_problem(), dref.LOSS_REG)])],
    ["quiet", "bigger", "other_width", "cross:gramian-splitk-f100", "refused_args", *ALWAYS],
    "solver.hip:57-59, 77 add doubles with atomicAdd; on the exact integer case every term and every partial sum is an integer "
    "below 2^53, so the sums are exact in any order (test_dense_host.py asserts the magnitudes)", lambda: _sizes(_loss_problem()[0]),
    lambda: _sizes(_loss_problem(4 * dref.LOSS_USERS, 4 * dref.LOSS_ITEMS)[0]))
PROBES["loss"].extra = {
    "bigger": _loss_bigger,
    "other_width": lambda gpu, p: _loss(gpu, *dref.loss_problem(dref.LOSS_USERS, dref.LOSS_ITEMS, 513)),
    "refused_args": lambda gpu, p: (lambda: _loss(gpu, *p.extra["refused_args_operands"]())),
    "refused_args_operands": lambda: (_loss_problem()[0], np.zeros((dref.LOSS_USERS, 1025), np.float32),
                                      np.zeros((dref.LOSS_ITEMS, 1025), np.float32)),
    "refused_args_reason": "1025 factors: calculate_loss takes at most 1024",
}


# =================================================================================================================================
# 2. the three solver families (long_ws, pad, w256_ws, nm_ticket, nm_fix_rows, chain / wide counters, fail_word, subspace_*)
# =================================================================================================================================
def _sweep(gpu, kind, C, X0, Y0, gram, reg, arg=None, gram_reg=None):
    """One half sweep: (X, Y and gramian after the call, the failed row or -1).  gram None: the library's gramian of Y0 with
    gram_reg on its diagonal, computed first, as the case modules' own solve() does."""
    solver = gpu.LeastSquaresSolver()
    f = X0.shape[1]
    Xd, Yd = gpu.Matrix(X0), gpu.Matrix(Y0)
    if gram is None:
        G = gpu.Matrix.zeros(f, f)
        solver.calculate_yty(Yd, G, gram_reg)
    else:
        G = gpu.Matrix(gram)
    failed = -1
    try:
        if kind == "cg":
            solver.least_squares(gpu.CSRMatrix(C), Xd, G, Yd, arg)
        elif kind == "cholesky":
            solver.least_squares_cholesky(gpu.CSRMatrix(C), Xd, G, Yd, reg)
        else:
            solver.least_squares_subspace(gpu.CSRMatrix(C), Xd, G, Yd, reg, arg[0], arg[1])
    except ValueError as e:
        failed = e.failed_row if kind != "cg" else -2
        if failed < 0:
            raise
    return {"X": Xd.to_numpy(), "Y": Yd.to_numpy(), "gram": G.to_numpy(), "failed_row": np.array([failed], dtype=np.int64)}


def _routes():
    import test_gpu_solver_routes as routes

    return routes


def _route_case(kind, f, storage):
    return (kind, f, storage, 3, "all")


def _route_run(gpu, case):
    routes = _routes()
    kind, f, storage, steps, rows = case
    C, X0, Y0 = routes._inputs(f, storage, rows)
    if kind == "cg":
        return _sweep(gpu, "cg", C, X0, Y0, None, routes.REG, steps, gram_reg=routes.REG)
    return _sweep(gpu, "cholesky", C, X0, Y0, None, routes.REG, gram_reg=0.0)


def _route_want(oracle, case, gram):
    """routes.expected without its cache (the cache is keyed by the case alone, and the GPU suite fills it from the device's
    gramian: a host-side gramian must not land in it)."""
    routes = _routes()
    kind, f, storage, steps, rows = case
    C, X0, Y0 = routes._inputs(f, storage, rows)
    Y32 = Y0.astype(np.float32)
    if kind == "cg":
        want = X0[: C.shape[0]].astype(np.float32)
        oracle.least_squares_cg(C, want, Y32, routes.REG, cg_steps=steps, YtY=gram)
    else:
        want = np.zeros((C.shape[0], f), dtype=np.float32)
        oracle.least_squares(C, want, Y32, routes.REG, YtY=gram)
    return want


def _host_gram(Y, reg):
    Y64 = np.asarray(Y, np.float64)
    return (Y64.T @ Y64 + reg * np.eye(Y.shape[1])).astype(np.float32)


def _route_gate(gpu, oracle, case, out):
    """test_gpu_solver_routes.check on an answer already computed."""
    routes = _routes()
    kind, f, storage, steps, rows = case
    C, X0, Y0 = routes._inputs(f, storage, rows)
    got, n, lens = out["X"], C.shape[0], np.diff(C.indptr)
    assert out["failed_row"][0] == -1
    assert got.dtype == X0.dtype and got.shape == X0.shape and bits(out["Y"]) == bits(Y0)
    assert bits(got[n:]) == bits(X0[n:]) and not got[:n][lens == 0].any()
    want = _route_want(oracle, case, out["gram"])
    assert np.isfinite(want).all()
    diff = np.linalg.norm(got[:n].astype(np.float64) - want, axis=1)
    norm = np.linalg.norm(want.astype(np.float64), axis=1)
    per_row = diff[lens > 0] / np.maximum(norm[lens > 0], 1e-30)
    whole = float(np.linalg.norm(diff) / max(np.linalg.norm(norm), 1e-30))
    print(f"{routes.case_id(case)}: sweep {whole:.2e}, worst row {per_row.max():.2e}")
    assert whole < routes.TOL[storage] and (per_row < routes.TOL[storage]).all(), (whole, per_row.max())


@functools.lru_cache(maxsize=None)
def _routes_bigger(kind, f, storage, seed=77):
    """Four times the rows and nonzeros of the routes matrix (every length four times), factors of another seed times 64."""
    routes = _routes()
    C = fast_matrix(routes.LENGTHS * 4, routes.COLS, seed)
    rng = np.random.default_rng(seed + f)
    X0 = ((rng.random((C.shape[0] + routes.EXTRA_ROWS, f), dtype=np.float32) * 0.2 - 0.1) * np.float32(SCALE)).astype(storage)
    Y0 = ((rng.random((routes.COLS, f), dtype=np.float32) * 0.2 - 0.1) * np.float32(SCALE)).astype(storage)
    return C, X0, Y0


def _routes_bigger_run(gpu, kind, f, storage):
    C, X0, Y0 = _routes_bigger(kind, f, storage)
    if kind == "cg":
        _sweep(gpu, "cg", C, X0, Y0, None, 0.05, 3, gram_reg=0.05)
    else:
        _sweep(gpu, "cholesky", C, X0, Y0, None, 0.05, gram_reg=0.0)


def _solver_refused_operands(f, storage):
    """(C, X, Y, gramian) of a half sweep check_solver_args stops: X has one column more than Y."""
    C, X0, Y0 = _routes()._inputs(f, storage, "all")
    return C, np.zeros((X0.shape[0], f + 1), X0.dtype), Y0, np.eye(f, dtype=np.float32)


def _solver_refused_args(gpu, kind, p):
    return lambda: _sweep(gpu, kind, *p.extra["refused_args_operands"](), 0.05, 3)


def _chol_failing(f, storage="float32"):
    return cc.failing_problem(f, cc.FAILING_SETS[0], storage)


def _chol_refused_pivot(gpu, f, storage="float32"):
    """A call the Cholesky half sweep refuses with a non-positive pivot: cholesky_cases.failing_problem, rows 4, 9, 13, 16."""
    p = _chol_failing(f, storage)

    def call():
        out = _sweep(gpu, "cholesky", p.C, p.X0, p.Y, p.gram, p.reg)
        assert out["failed_row"][0] == min(p.failing), out["failed_row"]
        raise ValueError(f"cholesky failed on row {out['failed_row'][0]}")

    return call


# which Cholesky route a CG probe's neighbours take: the same factor count where the routes test runs it
CG_ROUTES = [
    # name, f, storage, other width, cross Cholesky f, classes, owner, route
    ("cg-f128", 128, "float32", 64, 128, ("long", "nm_multi", "team16", "team8", "team4", "team2", "short32", "short16", "empty"),
     "long_ws, nm_ticket, nm_fix_rows, chain_counters, wide_counters", "chain, wide chain, short rows, normal-matrix long rows"),
    ("cg-f64-fp16", 64, "float16", 128, 64, ("long", "nm_multi", "team16", "team2", "short16", "empty"),
     "long_ws, nm_ticket, nm_fix_rows", "packed-fp16 tiles, normal-matrix long rows"),
    ("cg-f100", 100, "float32", 200, 100, ("long", "team8", "short32", "empty"), "pad.{x,y,gram,same}, long_ws", "padded onto f = 128"),
    ("cg-f256", 256, "float32", 320, 200, ("long", "team16", "short16", "empty"), "w256_ws, long_ws", "w256 resident kernels"),
    ("cg-f320", 320, "float32", 256, 260, ("long", "team16", "short16", "empty"), "long_ws", "generic kernels"),
]
CHOL_ROUTES = [
    ("chol-f64", 64, 128, ("chol_long", "long", "team16", "short16", "empty"), "long_ws, fail_word", "f = 64 kernel, segment plan above 1024"),
    ("chol-f128", 128, 64, ("long", "nm_multi", "team16", "short16", "empty"), "long_ws, nm_ticket, nm_fix_rows, fail_word",
     "normal matrices on the matrix cores"),
    ("chol-f100", 100, 200, ("long", "team16", "short16", "empty"), "pad.{x,y,gram}, long_ws, nm_ticket, nm_fix_rows, fail_word",
     "padded onto f = 128"),
    ("chol-f200", 200, 100, ("long", "team16", "short16", "empty"), "fail_word", "workgroup kernel, triangle in the LDS"),
    ("chol-f260", 260, 200, ("long", "team16", "short16", "empty"), "long_ws, fail_word", "workgroup kernel, triangle in the device workspace"),
]
DETERMINISTIC_SOLVER = ("every row is solved by one team / workgroup from its own inputs; long rows add their segments' partial vectors "
                        "or images in segment order; tickets and the fix-up list only decide WHO solves a row "
                        "(test_gpu_cg_class_chain.py asserts equal bits under different ticket orders); no floating-point atomics")


def _add_route(name, kind, f, storage, other, cross, classes, owner, sequence=False):
    case = _route_case(kind, f, storage)
    C = _routes()._matrix()

    def reference(oracle):
        routes = _routes()
        _, _, Y0 = routes._inputs(f, storage, "all")
        return [_route_want(oracle, case, _host_gram(Y0.astype(np.float32), routes.REG if kind == "cg" else 0.0))]

    add(name, kind, owner, lambda gpu: _route_run(gpu, case), lambda gpu, oracle, out: _route_gate(gpu, oracle, case, out), reference,
        ["quiet", "bigger", "other_width"] + [f"cross:{c}" for c in cross] + ["refused_args", "refused_pivot", *ALWAYS]
        + (["sequence"] if sequence else []), DETERMINISTIC_SOLVER, lambda: _sizes(C), lambda: _sizes(_routes_bigger(kind, f, storage)[0]),
        matrix=lambda: C, classes=classes)
    PROBES[name].extra = {
        "bigger": lambda gpu, p: _routes_bigger_run(gpu, kind, f, storage),
        "other_width": lambda gpu, p: _route_run(gpu, _route_case(kind, other, storage if kind == "cg" else "float32")),
        "refused_args": lambda gpu, p: _solver_refused_args(gpu, kind, p),
        "refused_args_operands": lambda: _solver_refused_operands(f, storage),
        "refused_args_reason": "X has one column more than Y",
        # a CG probe takes the failing Cholesky call of the route that shares its scratch
        "refused_pivot": lambda gpu, p: _chol_refused_pivot(gpu, f if kind == "cholesky" else {320: 260, 256: 200}.get(f, f),
                                                             storage if f == 64 else "float32"),
        "refused_pivot_problem": lambda: _chol_failing(f if kind == "cholesky" else {320: 260, 256: 200}.get(f, f),
                                                        storage if f == 64 else "float32"),
        "kind": kind, "f": f,
    }


for _name, _f, _st, _other, _cross, _classes, _owner, _route in CG_ROUTES:
    _add_route(_name, "cg", _f, _st, _other, [f"chol-f{_cross}", "subspace"], _classes, _owner)
for _name, _f, _other, _classes, _owner, _route in CHOL_ROUTES:
    _cg = {64: "cg-f64-fp16", 128: "cg-f128", 100: "cg-f100", 200: "cg-f256", 260: "cg-f320"}[_f]
    _add_route(_name, "cholesky", _f, "float32", _other, [_cg, "subspace", "explain", "spd-inverse"], _classes, _owner,
               sequence=_f == 128)


# ---- CG at f = 128 on the two `drawn` shapes: tickets from the device counters -------------------------------------------------------
def _chain(which="chain"):
    if which == "chain":
        import test_gpu_cg_class_chain as mod
    else:
        import test_gpu_cg_wide_chain as mod
    return mod


def _drawn_inputs(which):
    return _chain(which)._inputs("drawn", 128)


def _drawn_run(gpu, which):
    C, X0, Y0, _ = _drawn_inputs(which)
    return _sweep(gpu, "cg", C, X0, Y0, None, _chain(which).REG, 3, gram_reg=_chain(which).REG)


def _drawn_want(oracle, which, gram):
    C, X0, Y0, _ = _drawn_inputs(which)
    want = X0[: C.shape[0]].copy()
    oracle.least_squares_cg(C, want, Y0, _chain(which).REG, cg_steps=3, YtY=gram)
    return want


def _drawn_gate(gpu, oracle, which, out):
    """check() of test_gpu_cg_class_chain.py / test_gpu_cg_wide_chain.py on an answer already computed."""
    mod = _chain(which)
    tol = mod.TOL["float32"] if isinstance(mod.TOL, dict) else mod.TOL
    C, X0, Y0, negative = _drawn_inputs(which)
    got, n, lens = out["X"], C.shape[0], np.diff(C.indptr)
    assert got.dtype == np.float32 and got.shape == X0.shape and bits(out["Y"]) == bits(Y0)
    assert bits(got[n:]) == bits(X0[n:]) and not got[:n][lens == 0].any()
    want = _drawn_want(oracle, which, out["gram"])
    assert np.isfinite(want).all()
    rows = (lens > 0) & ~negative
    diff = np.linalg.norm(got[:n].astype(np.float64) - want, axis=1)
    norm = np.linalg.norm(want.astype(np.float64), axis=1)
    per_row = diff[rows] / np.maximum(norm[rows], 1e-30)
    whole = float(np.linalg.norm(diff) / max(np.linalg.norm(norm), 1e-30))
    print(f"{which} drawn-f128: sweep {whole:.2e}, worst row {per_row.max():.2e}")
    assert whole < tol and (per_row < tol).all(), (whole, per_row.max())


# rows of (32,64], (64,128], (128,256], (256,512], [1,32]: four times the `drawn` of the probe's own chain, beside the `drawn` of the other
DRAWN_BIGGER = {"chain": (36000, 18000, 9200, 1300, 20000), "wide": (9000, 4500, 2300, 5200, 80000)}


@functools.lru_cache(maxsize=None)
def class_matrix(counts, seed, cols=2000, extra=(0, 0, 5, 513, 1100, 1900)):
    """A matrix with counts = (team2, team4, team8, team16, short) rows in the five ticketed classes of the f = 128 CG half sweep
    (lengths uniform inside each class, both ends present where the class has two rows or more), then the rows of `extra`."""
    rng = np.random.default_rng(seed)
    parts = []
    for n, (lo, hi) in zip(counts, ((33, 64), (65, 128), (129, 256), (257, 512), (1, 32))):
        lens = rng.integers(lo, hi + 1, size=n)
        lens[:2] = (lo, hi)[:len(lens[:2])]
        parts.append(lens)
    lengths = np.concatenate(parts + [np.asarray(extra, dtype=np.int64)])
    rng.shuffle(lengths)
    return fast_matrix(lengths, cols, seed)


def _class_inputs(counts, seed, f, scale=1.0, cols=2000):
    C = class_matrix(tuple(counts), seed, cols)
    rng = np.random.default_rng(seed + f)
    X0 = (rng.random((C.shape[0] + 3, f), dtype=np.float32) * 0.2 - 0.1) * np.float32(scale)
    Y0 = (rng.random((cols, f), dtype=np.float32) * 0.2 - 0.1) * np.float32(scale)
    return C, X0, Y0


def _drawn_bigger(gpu, which):
    C, X0, Y0 = _class_inputs(DRAWN_BIGGER[which], 31, 128, SCALE)
    _sweep(gpu, "cg", C, X0, Y0, None, 0.05, 3, gram_reg=0.05)


def _add_drawn(name, which, owner, classes):
    add(name, "cg", owner, lambda gpu: _drawn_run(gpu, which), lambda gpu, oracle, out: _drawn_gate(gpu, oracle, which, out),
        lambda oracle: [_drawn_want(oracle, which, _host_gram(_drawn_inputs(which)[2], _chain(which).REG))],
        ["quiet", "bigger", "other_width", "cross:chol-f128", "cross:subspace", "refused_args", "refused_pivot", *ALWAYS,
         "sequence"],
        DETERMINISTIC_SOLVER, lambda: _sizes(_drawn_inputs(which)[0]), lambda: _sizes(class_matrix(DRAWN_BIGGER[which], 31)),
        matrix=lambda: _drawn_inputs(which)[0], classes=classes)
    PROBES[name].extra = {
        "bigger": lambda gpu, p: _drawn_bigger(gpu, which),
        "other_width": lambda gpu, p: _route_run(gpu, _route_case("cg", 64, "float32")),
        "refused_args": lambda gpu, p: _solver_refused_args(gpu, "cg", p),
        "refused_args_operands": lambda: _solver_refused_operands(128, "float32"),
        "refused_args_reason": "X has one column more than Y",
        "refused_pivot": lambda gpu, p: _chol_refused_pivot(gpu, 128),
        "refused_pivot_problem": lambda: _chol_failing(128),
        "kind": "cg", "f": 128,
    }


# more than four rows per team in the three 512-thread classes / in the two 1024-thread classes (on 256 CUs)
_add_drawn("cg-drawn-f128", "chain", "chain_counters, chain_tickets", ("team8", "team4", "team2", "short32", "empty"))
_add_drawn("cg-wide-drawn-f128", "wide", "wide_counters, wide_tickets", ("team16", "short32", "short16", "empty"))


# ---- subspace half sweep ------------------------------------------------------------------------------------------------------------
SUB_F, SUB_K, SUB_SWEEPS = 130, 32, 2


def _subspace_run(gpu):
    p = sc.routes_problem(SUB_F)
    return _sweep(gpu, "subspace", p.C, p.X0, p.Y, p.gram, p.reg, (SUB_K, SUB_SWEEPS))


def _subspace_gate(gpu, oracle, out):
    import test_gpu_subspace as tsub

    p = sc.routes_problem(SUB_F)
    x64, x32, _ = sc.reference("routes", SUB_F, SUB_K, max(sc.SWEEPS))
    n = p.C.shape[0]
    assert out["failed_row"][0] == -1 and bits(out["X"][n:]) == bits(p.X0[n:])
    assert bits(out["Y"]) == bits(p.Y) and bits(out["gram"]) == bits(p.gram)
    tsub.judge(f"f={SUB_F} k={SUB_K} sweeps={SUB_SWEEPS}", out["X"], x64[SUB_SWEEPS - 1], x32[SUB_SWEEPS - 1])


@functools.lru_cache(maxsize=None)
def _subspace_bigger_inputs():
    C = fast_matrix(sc.LENGTHS * 4, sc.COLS, 41, integer=False)
    rng = np.random.default_rng(42)
    Y = (rng.random((sc.COLS, SUB_F), dtype=np.float32) - np.float32(0.5)) * np.float32(0.3 * SCALE)
    X0 = rng.random((C.shape[0] + sc.EXTRA_ROWS, SUB_F), dtype=np.float32) * np.float32(0.01 * SCALE)
    return C, X0, Y, _host_gram(Y, 0.0)


def _subspace_refused_pivot(gpu, f=64, k=16):
    p = sc.failing_problem(f, sc.FAILING_SETS[0])

    def call():
        out = _sweep(gpu, "subspace", p.C, p.X0, p.Y, p.gram, p.reg, (k, 1))
        assert out["failed_row"][0] == min(p.failing), out["failed_row"]
        raise ValueError(f"subspace step failed on row {out['failed_row'][0]}")

    return call


add("subspace", "subspace", "subspace_pred, subspace_ws, fail_word", _subspace_run, _subspace_gate,
    lambda oracle: [sc.reference("routes", SUB_F, SUB_K, max(sc.SWEEPS))[0][SUB_SWEEPS - 1]],
    ["quiet", "bigger", "other_width", "cross:cg-f128", "cross:chol-f128", "cross:explain", "cross:spd-inverse", "refused_args",
     "refused_pivot", *ALWAYS, "sequence"],
    "als_subspace.hip: one wavefront per row; a long row's segment partials are added in segment order by its own wavefront; "
    "atomicMin on the failure word only (test_equal_inputs_give_equal_bits)", lambda: _sizes(sc.routes_problem(SUB_F).C),
    lambda: _sizes(_subspace_bigger_inputs()[0]), matrix=lambda: sc.routes_problem(SUB_F).C,
    classes=("sub_long", "long", "team16", "short16", "empty"))
PROBES["subspace"].extra = {
    "bigger": lambda gpu, p: _sweep(gpu, "subspace", *_subspace_bigger_inputs()[:3], _subspace_bigger_inputs()[3], 0.01, (SUB_K, SUB_SWEEPS)),
    "other_width": lambda gpu, p: _sweep(gpu, "subspace", sc.routes_problem(20).C, sc.routes_problem(20).X0, sc.routes_problem(20).Y,
                                          sc.routes_problem(20).gram, sc.REG, (8, 1)),
    "refused_args": lambda gpu, p: (lambda: _sweep(gpu, "subspace", sc.routes_problem(SUB_F).C, sc.routes_problem(SUB_F).X0,
                                                    sc.routes_problem(SUB_F).Y, sc.routes_problem(SUB_F).gram, sc.REG,
                                                    p.extra["refused_args_operands"]())),
    "refused_args_operands": lambda: (33, 1),  # (block_size, sweeps)
    "refused_args_reason": "block_size 33: the subspace sweep takes 1 .. 32",
    "refused_pivot": lambda gpu, p: _subspace_refused_pivot(gpu),
    "refused_pivot_problem": lambda: sc.failing_problem(64, sc.FAILING_SETS[0]),
    "kind": "subspace", "f": SUB_F,
}


# ---- explain ------------------------------------------------------------------------------------------------------------------------
EXPLAIN_F, EXPLAIN_M, EXPLAIN_N = 100, 10, 300


def _explain(gpu, Y, user_items, itemids, n, reg=xc.REG):
    """explain_factor + explain at the solver level: the totals, ids and scores, the factors W, and the failed row of a factorisation
    that was refused (then nothing else: the contributions are not asked for)."""
    solver = gpu.LeastSquaresSolver()
    f = Y.shape[1]
    C = gpu.CSRMatrix(user_items.astype(np.float32))
    Yd, G = gpu.Matrix(Y), gpu.Matrix.zeros(f, f)
    solver.calculate_yty(Yd, G, 0.0)
    W = gpu.Matrix.zeros(user_items.shape[0] * f, f)
    itemids = np.ascontiguousarray(itemids, dtype=np.int32)
    out = {"failed_row": np.array([-1], dtype=np.int64)}
    try:
        solver.explain_factor(C, G, Yd, reg, W)
        total, ids, scores = solver.explain(C, Yd, W, gpu.IntVector(itemids.reshape(-1)), itemids.shape[1], n)
        out.update(total=total.reshape(itemids.shape), ids=ids.reshape(itemids.shape + (n,)), scores=scores.reshape(itemids.shape + (n,)))
    except ValueError as e:
        if getattr(e, "failed_row", -1) < 0:
            raise
        out["failed_row"][0] = e.failed_row
    out.update(W=W.to_numpy(), Y=Yd.to_numpy(), gram=G.to_numpy())
    return out


def _explain_run(gpu):
    return _explain(gpu, xc.factors(EXPLAIN_F, xc.EDGE_ITEMS), xc.edge_matrix()[0], xc.edge_items(EXPLAIN_M), EXPLAIN_N)


def _explain_gate(gpu, oracle, out):
    import test_gpu_explain as texp

    assert out["failed_row"][0] == -1, f"explain_factor named row {out['failed_row'][0]} of a batch whose matrices are all positive definite"
    texp.check((out["total"], out["ids"], out["scores"]), xc.edge_reference(EXPLAIN_F, EXPLAIN_M, EXPLAIN_N), "history edges")
    assert bits(out["Y"]) == bits(xc.factors(EXPLAIN_F, xc.EDGE_ITEMS))


EXPLAIN_FAILING_USERS = np.array([250, 251, 252])  # test_gpu_explain.test_non_positive_pivot_names_the_user
EXPLAIN_FAILING_REG = -1000.0


def _explain_refused_pivot(gpu):
    def call():
        out = _explain(gpu, xc.factors(16), xc.accuracy_matrix()[EXPLAIN_FAILING_USERS], [[1], [2], [3]], 10, reg=EXPLAIN_FAILING_REG)
        assert out["failed_row"][0] == 0, out["failed_row"]
        raise ValueError("explain_factor failed on row 0")

    return call


@functools.lru_cache(maxsize=None)
def _explain_bigger_inputs():
    m, _ = xc.edge_matrix()
    big = sp.vstack([m] * 4).tocsr()
    ids = np.tile(xc.edge_items(EXPLAIN_M), (4, 1))
    Y = np.random.default_rng(3).uniform(-0.05 * SCALE, 0.05 * SCALE, size=(xc.EDGE_ITEMS, EXPLAIN_F)).astype(np.float32)
    return Y, big, ids


def _explain_refused_args(gpu, user_items, Y, weights_shape):
    f = Y.shape[1]
    return lambda: gpu.LeastSquaresSolver().explain_factor(gpu.CSRMatrix(user_items), gpu.Matrix.zeros(f, f), gpu.Matrix(Y), xc.REG,
                                                           gpu.Matrix.zeros(*weights_shape))


add("explain", "explain", "fail_word, the key workspace (a pool block)", _explain_run, _explain_gate,
    lambda oracle: [xc.edge_reference(EXPLAIN_F, EXPLAIN_M, EXPLAIN_N)[0]],
    ["quiet", "bigger", "other_width", "cross:chol-f100", "cross:subspace", "cross:spd-inverse", "refused_args", "refused_pivot",
     *ALWAYS],
    "explain.hip: one workgroup per row / pair, fixed reduction trees; the atomicAdd of line 267 counts integers in the LDS "
    "(test_same_call_twice_is_bit_identical)", lambda: _sizes(xc.edge_matrix()[0]), lambda: _sizes(_explain_bigger_inputs()[1]))
PROBES["explain"].extra = {
    "bigger": lambda gpu, p: _explain(gpu, *_explain_bigger_inputs(), EXPLAIN_N),
    "other_width": lambda gpu, p: _explain(gpu, xc.factors(256, xc.EDGE_ITEMS), xc.edge_matrix()[0], xc.edge_items(1), 10),
    "refused_args": lambda gpu, p: _explain_refused_args(gpu, *p.extra["refused_args_operands"]()),
    "refused_args_operands": lambda: (xc.accuracy_matrix()[:3], xc.factors(16), (16, 16)),  # user rows, Y, shape of `weights`
    "refused_args_reason": "weights is 16 x 16 for three users of 16 factors: it must have 48 rows",
    "refused_pivot": lambda gpu, p: _explain_refused_pivot(gpu),
    "kind": "explain",
}


# =================================================================================================================================
# 3. EASE fit kernels and PureSVD kernels
# =================================================================================================================================
SPD_N = 300
SPD_FAILING = (300, 257)  # test_gpu_ease.test_spd_inverse_failed_pivot: order, failing pivot


def _spd(gpu, G32):
    A = np.tril(G32).astype(np.float32)
    M = gpu.Matrix(A)
    failed = -1
    try:
        gpu.spd_inverse(M)
    except ValueError as e:
        failed = e.failed_pivot
        if failed < 0:
            raise
    return {"P": M.to_numpy(), "failed_pivot": np.array([failed], dtype=np.int64)}


def _spd_gate(gpu, oracle, out):
    import test_gpu_ease as tease

    G32, P64 = eref.spd_case(SPD_N)
    d_ref, d_gpu = eref.rel_distance(eref.lapack32_inverse(G32), P64), eref.rel_distance(out["P"], P64)
    assert out["failed_pivot"][0] == -1 and np.array_equal(out["P"], out["P"].T)
    assert d_gpu <= max(2 * d_ref, tease.FLOOR), (d_gpu, d_ref)


def _spd_failing_matrix():
    n, bad = SPD_FAILING
    A = 2.0 * np.eye(n, dtype=np.float32)
    A[bad, bad] = -1.0
    return A


def _spd_refused_pivot(gpu):
    def call():
        out = _spd(gpu, _spd_failing_matrix())
        assert out["failed_pivot"][0] == SPD_FAILING[1], out["failed_pivot"]
        raise ValueError(f"spd_inverse failed at pivot {out['failed_pivot'][0]}")

    return call


add("spd-inverse", "ease", "fail_word, the factor workspace (a pool block)", lambda gpu: _spd(gpu, eref.spd_case(SPD_N)[0]), _spd_gate,
    lambda oracle: [eref.spd_case(SPD_N)[1]],
    ["quiet", "bigger", "other_width", "cross:chol-f128", "cross:subspace", "cross:explain", "refused_args", "refused_pivot", *ALWAYS],
    "spd_inverse.hip: blocked products in a fixed order, atomicMin on the failure word only", lambda: (SPD_N, SPD_N * SPD_N),
    lambda: (1200, 1200 * 1200))
PROBES["spd-inverse"].extra = {
    "bigger": lambda gpu, p: _spd(gpu, np.asarray(eref.spd_case(1200)[0]) * np.float32(SCALE)),
    "other_width": lambda gpu, p: _spd(gpu, eref.spd_case(129)[0]),
    "refused_args": lambda gpu, p: (lambda: gpu.spd_inverse(gpu.Matrix.zeros(*p.extra["refused_args_operands"]()))),
    "refused_args_operands": lambda: (4, 5),
    "refused_args_reason": "a 4 x 5 matrix is not square",
    "refused_pivot": lambda gpu, p: _spd_refused_pivot(gpu),
    "kind": "spd",
}

EASE_ITEMS = 257


def _ease_gram(gpu, X, reg):
    from implicit_amd.utils import transpose_csr

    X = X.astype(np.float32)
    X.sum_duplicates()
    return {"G": gpu.ease_gram(gpu.CSRMatrix(transpose_csr(X)), gpu.CSRMatrix(X), reg).to_numpy()}


def _ease_gram_gate(gpu, oracle, out):
    X = eref.gram_exact_case(EASE_ITEMS)
    assert np.array_equal(out["G"], out["G"].T) and np.array_equal(out["G"].astype(np.float64), eref.gram64(X, eref.GRAM_REG))


@functools.lru_cache(maxsize=None)
def _ease_gram_bigger():
    from implicit_amd.synthetic import synthetic_csr

    return synthetic_csr(4 * (4 * EASE_ITEMS + 3), 2 * EASE_ITEMS, 4 * eref.gram_exact_case(EASE_ITEMS).nnz + 1000, seed=9) * SCALE


add("ease-gram", "ease", "none kept (the LDS slab)", lambda gpu: _ease_gram(gpu, eref.gram_exact_case(EASE_ITEMS), eref.GRAM_REG), _ease_gram_gate,
    lambda oracle: [eref.gram64(eref.gram_exact_case(EASE_ITEMS), eref.GRAM_REG)],
    ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "ease.hip: every entry is one thread's sum in item_users' stored order", lambda: _sizes(eref.gram_exact_case(EASE_ITEMS)),
    lambda: _sizes(_ease_gram_bigger()))
PROBES["ease-gram"].extra = {
    "bigger": lambda gpu, p: _ease_gram(gpu, _ease_gram_bigger(), 1.0),
    "other_width": lambda gpu, p: _ease_gram(gpu, eref.gram_exact_case(70), eref.GRAM_REG),
    "refused_args": lambda gpu, p: (lambda: gpu.ease_gram(*(gpu.CSRMatrix(m) for m in p.extra["refused_args_operands"]()), 1.0)),
    "refused_args_operands": lambda: (eref.gram_exact_case(63).astype(np.float32),) * 2,  # (item_users, user_items)
    "refused_args_reason": "the same orientation twice: not the two orientations of one matrix",
}


@functools.lru_cache(maxsize=None)
def _weights_input(n=EASE_ITEMS):
    return eref.lapack32_inverse(eref.spd_case(n)[0]).astype(np.float32)


def _ease_weights(gpu, P):
    return {"B": gpu.ease_weights(gpu.Matrix(P.copy())).to_numpy()}


def _bad_diagonal():
    P = _weights_input(65).copy()
    P[17, 17] = 0.0
    return P


add("ease-weights", "ease", "the diagonal copy and the flag (pool blocks)", lambda gpu: _ease_weights(gpu, _weights_input()),
    lambda gpu, oracle, out: np.testing.assert_array_equal(out["B"].view(np.uint32), eref.weights32(_weights_input()).view(np.uint32)),
    lambda oracle: [eref.weights32(_weights_input())], ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "ease.hip: one division and a sign flip per entry", lambda: (EASE_ITEMS, EASE_ITEMS ** 2), lambda: (1200, 1200 ** 2))
PROBES["ease-weights"].extra = {
    "bigger": lambda gpu, p: _ease_weights(gpu, np.asarray(eref.spd_case(1200)[1], dtype=np.float32) * np.float32(SCALE)),
    "other_width": lambda gpu, p: _ease_weights(gpu, _weights_input(65)),
    "refused_args": lambda gpu, p: (lambda: _ease_weights(gpu, p.extra["refused_args_operands"]())),
    "refused_args_operands": _bad_diagonal,
    "refused_args_reason": "a zero on the diagonal",
}

SPMM_L = 130


@functools.lru_cache(maxsize=None)
def _spmm_inputs():
    A = sref.spmm_case()
    D = sref.dense_case(A.shape[1], SPMM_L)
    return A, D


def _spmm(gpu, A, D):
    Dd = gpu.Matrix(D)
    out = gpu.Matrix(np.full((A.shape[0], D.shape[1]), 7.0, dtype=np.float32))  # a buffer that held something else
    gpu.spmm(gpu.CSRMatrix(A), Dd, out=out)
    return {"out": out.to_numpy(), "D": Dd.to_numpy()}


def _spmm_gate(gpu, oracle, out):
    A, D = _spmm_inputs()
    np.testing.assert_array_equal(out["out"].view(np.uint32), np.ascontiguousarray(sref.spmm32(A, D)[0], dtype=np.float32).view(np.uint32))
    assert bits(out["D"]) == bits(D)


@functools.lru_cache(maxsize=None)
def _spmm_bigger_inputs():
    A, _ = _spmm_inputs()
    return sp.vstack([A] * 4).tocsr() * SCALE, sref.dense_case(A.shape[1], 264, seed=8)


add("spmm", "svd", "the long rows' partials (a pool block)", lambda gpu: _spmm(gpu, *_spmm_inputs()), _spmm_gate,
    lambda oracle: [sref.spmm32(*_spmm_inputs())[0]], ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "svd.hip: a row's products in stored order, runs of 1024 added in order", lambda: _sizes(_spmm_inputs()[0]),
    lambda: _sizes(_spmm_bigger_inputs()[0]), matrix=lambda: _spmm_inputs()[0], classes=("sub_long", "long", "empty"))
PROBES["spmm"].extra = {
    "bigger": lambda gpu, p: _spmm(gpu, *_spmm_bigger_inputs()),
    "other_width": lambda gpu, p: _spmm(gpu, _spmm_inputs()[0], sref.dense_case(_spmm_inputs()[0].shape[1], 24)),
    "refused_args": lambda gpu, p: (lambda: _spmm(gpu, *p.extra["refused_args_operands"]())),
    "refused_args_operands": lambda: (_spmm_inputs()[0], sref.dense_case(_spmm_inputs()[0].shape[1] + 1, SPMM_L)),
    "refused_args_reason": "D has one row more than A has columns",
}

MULT = (1000, 130, 128)


def _multiply(gpu, Y, W):
    Yd, Wd = gpu.Matrix(Y), gpu.Matrix(W)
    out = gpu.Matrix(np.full((Y.shape[0], W.shape[1]), 7.0, dtype=np.float32))
    gpu.multiply_small(Yd, Wd, out=out)
    return {"out": out.to_numpy(), "Y": Yd.to_numpy(), "W": Wd.to_numpy()}


def _mult_inputs():
    return sref.dense_case(MULT[0], MULT[1]), sref.dense_case(MULT[1], MULT[2], seed=6)


def _multiply_gate(gpu, oracle, out):
    Y, W = _mult_inputs()
    exact, bound = sref.multiply_bound(Y, W)
    assert (np.abs(out["out"].astype(np.float64) - exact) <= bound).all()
    assert bits(out["Y"]) == bits(Y) and bits(out["W"]) == bits(W)


add("multiply-small", "svd", "none kept", lambda gpu: _multiply(gpu, *_mult_inputs()), _multiply_gate,
    lambda oracle: [sref.multiply_bound(*_mult_inputs())[0]], ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "svd.hip: exact fp32 products on the matrix cores in a fixed order", lambda: (MULT[0], MULT[0] * MULT[1]),
    lambda: (4 * MULT[0], 4 * MULT[0] * 264))
PROBES["multiply-small"].extra = {
    "bigger": lambda gpu, p: _multiply(gpu, sref.dense_case(4 * MULT[0], 264, seed=2) * np.float32(SCALE), sref.dense_case(264, 256, seed=3)),
    "other_width": lambda gpu, p: _multiply(gpu, sref.dense_case(MULT[0], 24), sref.dense_case(24, 16, seed=6)),
    "refused_args": lambda gpu, p: (lambda: _multiply(gpu, *p.extra["refused_args_operands"]())),
    "refused_args_operands": lambda: (sref.dense_case(65, 24), sref.dense_case(25, 16)),
    "refused_args_reason": "W has one row more than Y has columns",
}


# =================================================================================================================================
# 4. shared handles: KnnQuery (topk, rank, ease_topk), IVFIndex, RankingMetrics
# =================================================================================================================================
_HANDLES = {}


def handle(gpu, kind):
    """The process's one KnnQuery / IVFIndex / RankingMetrics: every probe and every predecessor of the family goes through it."""
    if kind not in _HANDLES:
        if kind == "knn":
            _HANDLES[kind] = gpu.KnnQuery()
        elif kind == "ivf":
            _HANDLES[kind] = _ivf_build(gpu)
        else:
            _HANDLES[kind] = gpu.RankingMetrics(eval_pattern(), EVAL_K)
    return _HANDLES[kind]


def _topk_routes():
    import test_gpu_topk_routes as troutes

    return troutes


@functools.lru_cache(maxsize=None)
def _topk_inputs(name):
    troutes = _topk_routes()
    return troutes._inputs(troutes.BY_NAME[name])


def _topk(gpu, items, q, k, norms=None, liked=None, filt=None):
    kw = {}
    if norms is not None:
        kw["item_norms"] = gpu.Matrix(norms.reshape(1, -1))
    if liked is not None:  # through the page-locked stage and its event (pin_stage), as recommend() builds its filter
        kw["query_filter"] = gpu.COOMatrix.from_csr_pattern(liked)
    if filt is not None:
        kw["item_filter"] = gpu.IntVector(filt)
    I, Q = gpu.Matrix(items), gpu.Matrix(q)
    ids, d = handle(gpu, "knn").topk(I, Q, k, **kw)
    return {"ids": ids, "dist": d, "items": I.to_numpy(), "queries": Q.to_numpy()}


def _topk_run(gpu, name):
    items, q, S, norms, liked, filt = _topk_inputs(name)
    return _topk(gpu, items, q, _topk_routes().BY_NAME[name].k, norms, liked, filt)


def _topk_gate(gpu, oracle, name, out):
    troutes = _topk_routes()
    case = troutes.BY_NAME[name]
    items, q, S, norms, liked, filt = _topk_inputs(name)
    assert out["ids"].shape == out["dist"].shape == (case.nq, case.k) and out["ids"].dtype == np.int32
    troutes.judge(case, items, q, S, norms, out["ids"], out["dist"])
    assert bits(out["items"]) == bits(items) and bits(out["queries"]) == bits(q)


def _topk_bigger(gpu, f, dt):
    """Four times the items and queries, k = 64, the per-query filter alone, factors of another seed times 64."""
    rng = np.random.default_rng(500 + f)
    items = (rng.standard_normal((4 * 8192, f)) * 0.1 * SCALE).astype(dt)
    q = (rng.standard_normal((4 * 130, f)) * 0.1 * SCALE).astype(dt)
    liked = sp.random(q.shape[0], items.shape[0], density=20.0 / items.shape[0], format="csr", dtype=np.float32, random_state=5)
    _topk(gpu, items, q, 64, liked=liked)


def _topk_other_width(gpu, f):
    other = {64: 100, 100: 16}[f]  # 16 to 100: the padded copies are laid out anew; 100 to 64: left behind, unused
    rng = np.random.default_rng(600 + other)
    _topk(gpu, (rng.standard_normal((8192, other)) * 0.1).astype(np.float32), (rng.standard_normal((130, other)) * 0.1).astype(np.float32), 10)


TOPK_PROBES = {"topk-f64-filters": "emit-filters", "topk-f100": "emit-padded", "topk-f64-fp16": "emit-fp16", "topk-f64-cosine": "emit-cosine"}
DETERMINISTIC_TOPK = ("topk.hip, topk_select.h, topk_resident.h: candidate lists are filled through integer atomics (slots) and float bit "
                      "patterns through atomicMax, both order-independent; the select orders by the total order (score, id)")
for _name, _case in TOPK_PROBES.items():
    _c = _topk_routes().BY_NAME[_case]
    add(_name, "knn", "imp_knn: scores, candidates, thresholds, fallback lists, bitmaps, padded copies, planes",
        lambda gpu, _case=_case: _topk_run(gpu, _case), lambda gpu, oracle, out, _case=_case: _topk_gate(gpu, oracle, _case, out),
        lambda oracle, _case=_case: [np.where(np.isfinite(_topk_inputs(_case)[2]), _topk_inputs(_case)[2], 0.0)],
        ["quiet", "bigger", "other_width"] + [f"cross:{n}" for n in TOPK_PROBES if n != _name] + ["cross:knn-rank", "cross:ease-topk",
                                                                                                    "refused_args", *ALWAYS],
        DETERMINISTIC_TOPK, lambda _c=_c: (_c.nq, _c.ni), lambda: (4 * 130, 4 * 8192))
    PROBES[_name].extra = {
        "bigger": lambda gpu, p, _c=_c: _topk_bigger(gpu, _c.f, _c.dt),
        "other_width": lambda gpu, p, _c=_c: _topk_other_width(gpu, _c.f),
        "refused_args": lambda gpu, p: (lambda: _topk(gpu, *p.extra["refused_args_operands"](), 5)),
        "refused_args_operands": lambda _c=_c: (np.zeros((50, _c.f), np.float32), np.zeros((3, _c.f + 1), np.float32)),
        "refused_args_reason": "the queries have one column more than the items",
    }

RANK_MODEL, RANK_N = "als32", 10


@functools.lru_cache(maxsize=None)
def _rank_inputs(model=RANK_MODEL, copies=1):
    """(X, Y, lists, offsets, candidates): every user of rank_cases against its own list, the batch `copies` times over."""
    from implicit_amd.utils import candidate_lists

    X, Y = rc.factors(model)
    users = np.tile(rc.ALL, copies)
    lists = rc.lists_of(users)
    offsets, cand = candidate_lists(lists, len(users))
    return X[users], Y, lists, offsets, cand


def _rank(gpu, X, Y, offsets, cand, n, liked=None):
    knn = handle(gpu, "knn")
    Yd, Xd = gpu.Matrix(np.array(Y)), gpu.Matrix(np.array(X))
    scores = knn.rank(Yd, Xd, offsets, cand, 0, liked)
    ids, best = knn.rank(Yd, Xd, offsets, cand, n, liked)
    return {"scores": scores, "ids": ids, "best": best, "items": Yd.to_numpy(), "queries": Xd.to_numpy()}


def _rank_gate(gpu, oracle, out):
    import test_gpu_rank as trank

    X, Y, lists, offsets, cand = _rank_inputs()
    s64, mags = rref.scores(X, Y, rc.ALL, lists)
    got = np.split(out["scores"], offsets[1:-1])
    width = rc.MODELS[RANK_MODEL][1]
    for s, want, m in zip(got, s64, mags):  # test_gpu_rank.test_scores_against_float64
        assert (np.abs(s.astype(np.float64) - want) <= width * 2.0 ** -23 * m).all()
    trank.assert_ranked((out["ids"], out["best"]), trank.expected_rank(got, lists, RANK_N))
    assert bits(out["items"]) == bits(Y) and bits(out["queries"]) == bits(X)


def _rank_bigger(gpu, p):
    X, Y, lists, offsets, cand = _rank_inputs("als256", 4)
    liked = sp.vstack([rc.liked().sorted_indices()] * 4).tocsr()
    _rank(gpu, X * np.float32(SCALE), Y * np.float32(SCALE), offsets, cand, 1024, liked)


add("knn-rank", "knn", "the chunk's pool blocks; the handle's budget", lambda gpu: _rank(gpu, *_rank_inputs()[:2], *_rank_inputs()[3:], RANK_N),
    _rank_gate, lambda oracle: [np.concatenate(rref.scores(*_rank_inputs()[:2], rc.ALL, _rank_inputs()[2])[0])],
    ["quiet", "bigger", "other_width", "cross:topk-f100", "cross:ease-topk", "refused_args", *ALWAYS],
    "rank.hip: one workgroup per list, integer atomics on LDS slots, total order", lambda: (rc.USERS, len(_rank_inputs()[4])),
    lambda: (4 * rc.USERS, len(_rank_inputs("als256", 4)[4])))
PROBES["knn-rank"].extra = {
    "bigger": _rank_bigger,  # the batch four times over against 256 columns, N = 1024, the liked filter
    "other_width": lambda gpu, p: _rank(gpu, *_rank_inputs("als100")[:2], *_rank_inputs("als100")[3:], 2),
    "refused_args": lambda gpu, p: (lambda: _rank(gpu, *p.extra["refused_args_operands"](), *_rank_inputs()[3:], 5)),
    "refused_args_operands": lambda: (np.zeros((rc.USERS, rc.MODELS[RANK_MODEL][1] + 1), np.float32), _rank_inputs()[1]),
    "refused_args_reason": "the queries have one column more than the items",
}

EASE_TOPK = (257, 10)


@functools.lru_cache(maxsize=None)
def _ease_topk_inputs(items=EASE_TOPK[0]):
    B, rows = eref.topk_case(items)
    return B, rows, np.unique(np.array([0, items // 3, items - 1], dtype=np.int32))


def _ease_topk(gpu, B, rows, k, liked, filt):
    Bd = gpu.Matrix(B)
    ids, scores = gpu.ease_topk(handle(gpu, "knn"), Bd, rows, k, liked, filt)
    return {"ids": ids, "scores": scores, "B": Bd.to_numpy()}


def _ease_topk_gate(gpu, oracle, out):
    B, rows, filt = _ease_topk_inputs()
    want_ids, want_scores = eref.recommend32(B, rows, EASE_TOPK[1], True, filt)
    np.testing.assert_array_equal(out["ids"], want_ids)
    np.testing.assert_array_equal(out["scores"].view(np.uint32), want_scores.view(np.uint32))
    assert bits(out["B"]) == bits(B)


def _ease_topk_bigger(gpu, p):
    B, rows, _ = _ease_topk_inputs(5000)
    _ease_topk(gpu, B * np.float32(SCALE), sp.vstack([rows] * 4).tocsr(), 1024, False, None)


add("ease-topk", "knn", "the chunk's pool blocks, the filter bitmap; the handle's budget",
    lambda gpu: _ease_topk(gpu, *_ease_topk_inputs()[:2], EASE_TOPK[1], True, _ease_topk_inputs()[2]), _ease_topk_gate,
    lambda oracle: [eref.recommend32(*_ease_topk_inputs()[:2], EASE_TOPK[1], True, _ease_topk_inputs()[2])[1]],
    ["quiet", "bigger", "other_width", "cross:topk-f64-filters", "cross:knn-rank", "refused_args", *ALWAYS],
    "ease.hip: a score is one thread's sum in stored order; slabs sorted, merged under the total order",
    lambda: _sizes(_ease_topk_inputs()[1]), lambda: (4 * _ease_topk_inputs(5000)[1].shape[0], 4 * _ease_topk_inputs(5000)[1].nnz))
PROBES["ease-topk"].extra = {
    "bigger": _ease_topk_bigger,
    "other_width": lambda gpu, p: _ease_topk(gpu, *_ease_topk_inputs(70)[:2], 10, False, None),
    "refused_args": lambda gpu, p: (lambda: _ease_topk(gpu, *_ease_topk_inputs()[:2], p.extra["refused_args_operands"](), False, None)),
    "refused_args_operands": lambda: 1025,
    "refused_args_reason": "k = 1025: ease_topk takes 1 .. 1024",
}

IVF_CASE, IVF_SEARCH = "tiles", 1


def _ivf_build(gpu, vectors=None):
    c = ic.get(IVF_CASE)
    return gpu.IVFIndex.build(ic.cast(c.vectors, c.vdtype) if vectors is None else vectors, c.nlist, 0, init_rows=c.init_rows)


def _ivf_search(gpu, queries, k, nprobe, build=False):
    """The search on the process's one handle; build: an index built anew by this call as well -- its centroids and lists, and
    the same search on it (a workspace that has held nothing)."""
    ids, dist, probes = handle(gpu, "ivf").search(queries, k, nprobe, return_probes=True)
    out = {"ids": ids, "dist": dist, "probes": probes}
    if build:
        ix = _ivf_build(gpu)
        ids, dist, probes = ix.search(queries, k, nprobe, return_probes=True)
        out.update(centroids=ix.centroids, list_offsets=ix.list_offsets, list_ids=ix.list_ids, new_ids=ids, new_dist=dist, new_probes=probes)
    return out


def _ivf_queries(s):
    q = ic.cast(s.queries, s.qdtype)
    return q if s.repeat is None else q[np.arange(s.repeat) % len(q)]


def _ivf_size(s):
    return len(_ivf_queries(s)), len(_ivf_queries(s)) * s.k  # queries, result slots


def _ivf_run(gpu):
    s = ic.get(IVF_CASE).searches[IVF_SEARCH]
    return _ivf_search(gpu, _ivf_queries(s), s.k, s.nprobe, build=True)


def _ivf_want():
    import ivf_reference as iref

    c = ic.get(IVF_CASE)
    s = c.searches[IVF_SEARCH]
    coord, sign, assign, offsets, ids = iref.exact_build(c.vectors, c.init_rows)
    probes, want_ids, scores = iref.exact_search(coord, sign, assign, c.vectors, s.queries, s.k, s.nprobe)
    if s.repeat is not None:
        rows = np.arange(s.repeat) % len(s.queries)
        probes, want_ids, scores = probes[rows], want_ids[rows], scores[rows]
    return (probes, want_ids, scores.astype(np.float32), iref.exact_centroid_matrix(coord, sign, c.vectors.shape[1]), offsets, ids)


def _ivf_gate(gpu, oracle, out):
    probes, ids, scores, centroids, offsets, list_ids = _ivf_want()
    for key, want in (("probes", probes), ("ids", ids), ("dist", scores), ("centroids", centroids), ("list_offsets", offsets),
                      ("list_ids", list_ids), ("new_probes", probes), ("new_ids", ids), ("new_dist", scores)):
        np.testing.assert_array_equal(out[key], want, err_msg=key)  # test_gpu_ivf_edges: zero tolerance


def _ivf_bigger(gpu, p):
    c = ic.get(IVF_CASE)
    q = _ivf_queries(c.searches[0])
    _ivf_search(gpu, np.tile(q, (4, 1)) * np.float32(SCALE), 300, 7)
    _ivf_build(gpu, np.tile(ic.cast(c.vectors, c.vdtype), (4, 1)) * np.float32(SCALE))  # four times the rows through the build kernels


add("ivf", "ivf", "imp_ivf::Workspace: Q, S, probes, the grouping counters, out_ids / out_dist; the build's temporaries (pool blocks)",
    _ivf_run, _ivf_gate,
    lambda oracle: [_ivf_want()[2]], ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "ivf.hip: integer atomics on counters and slots; scores are one lane's MFMA accumulation in a fixed order; the select uses the "
    "total order", lambda: _ivf_size(ic.get(IVF_CASE).searches[IVF_SEARCH]),
    lambda: (4 * len(_ivf_queries(ic.get(IVF_CASE).searches[0])), 4 * len(_ivf_queries(ic.get(IVF_CASE).searches[0])) * 300))
PROBES["ivf"].extra = {
    "bigger": _ivf_bigger,
    "other_width": lambda gpu, p: _ivf_search(gpu, _ivf_queries(ic.get(IVF_CASE).searches[0])[:2], 7, 2),  # another k and probe count
    "refused_args": lambda gpu, p: (lambda: _ivf_search(gpu, p.extra["refused_args_operands"](), 3, 1)),
    "refused_args_operands": lambda: np.zeros((2, ic.get(IVF_CASE).vectors.shape[1] + 1), np.float32),
    "refused_args_reason": "the queries have one column more than the index",
}

EVAL_K, EVAL_USERS, EVAL_ITEMS, EVAL_ROWS = 10, 400, 300, 65


@functools.lru_cache(maxsize=None)
def eval_pattern():
    """The held-out pattern of tests/test_gpu_eval.py's fixture: a quarter of the users holds nothing out, the others 1 .. 150."""
    rng = np.random.default_rng(9)
    lengths = np.where(np.arange(EVAL_USERS) % 4 == 1, 0, rng.integers(1, 151, EVAL_USERS))
    lengths[:4] = (1, 0, 150, 64)
    indices = np.concatenate([np.sort(rng.choice(EVAL_ITEMS, size=n, replace=False)) for n in lengths]).astype(np.int32)
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(EVAL_USERS, EVAL_ITEMS))


def _eval_rows(n, seed):
    import test_gpu_eval as teval

    return teval.rows_for(EVAL_K, n, seed, EVAL_ITEMS)


def _eval(gpu, ids, userids, reset=True):
    acc = handle(gpu, "eval")
    if reset:
        acc.reset()
    rows = acc.add(ids, userids, per_row=True)
    return {"rows": rows, "sums": np.array([acc.sums()[k] for k in evref.SUMS])}


def _eval_gate(gpu, oracle, out):
    import test_gpu_eval as teval

    ids, userids = _eval_rows(EVAL_ROWS, 7)
    want, want_rows = evref.metrics(eval_pattern(), ids, userids, EVAL_K)
    assert np.array_equal(out["rows"][:, 0], want_rows[:, 0])
    np.testing.assert_allclose(out["rows"], want_rows, rtol=EVAL_K * 2.0 ** -52, atol=0)  # test_kernel_equals_numpy
    teval.check_sums(dict(zip(evref.SUMS, out["sums"].tolist())), want)


add("ranking-metrics", "eval", "imp_eval: sums, slots", lambda gpu: _eval(gpu, *_eval_rows(EVAL_ROWS, 7)), _eval_gate,
    lambda oracle: [evref.metrics(eval_pattern(), *_eval_rows(EVAL_ROWS, 7), EVAL_K)[1]],
    ["quiet", "bigger", "refused_args", *ALWAYS],
    "evaluation.hip: per-workgroup slots in row order, folded by one workgroup in a fixed tree", lambda: (EVAL_ROWS, EVAL_ROWS * EVAL_K),
    lambda: (3000, 3000 * EVAL_K))
PROBES["ranking-metrics"].extra = {
    "bigger": lambda gpu, p: _eval(gpu, *_eval_rows(3000, 8), reset=False),  # more workgroups' slots, and sums the probe has to reset
    "refused_args": lambda gpu, p: (lambda: _eval(gpu, *p.extra["refused_args_operands"]())),
    "refused_args_operands": lambda: (np.zeros((4, EVAL_K + 1), np.int32), np.zeros(4, np.int32)),
    "refused_args_reason": "ids has K + 1 columns",
}


# =================================================================================================================================
# 5. sparse_topk_product, lmf_update, warp_epoch
# =================================================================================================================================
KNN_CASE = "table_cut_k100"  # rows of 1535 / 1536 touched columns stay in the hash pass, 1537 / 1600 go to the dense pass


def _product(gpu, c):
    ids, scores, counts = gpu.sparse_topk_product(gpu.SpMat(c.A), gpu.SpMat(c.B), c.k, c.zero_own)
    return {"ids": ids, "scores": scores, "counts": counts}


def _product_gate(gpu, oracle, out):
    c = kc.get(KNN_CASE)
    wi, ws, wc = kr.product_topk(c.A, c.B, c.k, c.zero_own)
    np.testing.assert_array_equal(out["counts"], wc)
    np.testing.assert_array_equal(out["ids"], wi)
    np.testing.assert_array_equal(out["scores"].view(np.int64), ws.view(np.int64))


def _product_refused_operands():
    rep = kc.csr_from_rows([([1, 2, 1], [1.0, 2.0, 3.0]), ([0], [1.0]), ([], [])], 3)  # test_failure_paths_leave_the_device_usable
    return sp.csr_matrix(np.eye(3)), rep


def _product_refused(gpu):
    A, B = _product_refused_operands()
    return lambda: gpu.sparse_topk_product(gpu.SpMat(A), gpu.SpMat(B), 2)


add("sparse-topk-product", "knn-product", "knn_acc, knn_touched, knn_cols", lambda gpu: _product(gpu, kc.get(KNN_CASE)), _product_gate,
    lambda oracle: [np.where(np.isfinite(kr.product_topk(kc.get(KNN_CASE).A, kc.get(KNN_CASE).B, 100, False)[1]),
                             kr.product_topk(kc.get(KNN_CASE).A, kc.get(KNN_CASE).B, 100, False)[1], 0.0)],
    ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "knn.hip: a row's sums in A's stored order; the atomicCAS claims hash slots, the atomicAdd of line 247 orders the dense pass's "
    "work list, neither enters a sum; total order", lambda: (kc.get(KNN_CASE).A.shape[0], kc.pair_count(kc.get(KNN_CASE).A, kc.get(KNN_CASE).B)),
    lambda: (kc.get("dense_reuse_k20").A.shape[0], kc.pair_count(kc.get("dense_reuse_k20").A, kc.get("dense_reuse_k20").B)))
PROBES["sparse-topk-product"].extra = {
    "bigger": lambda gpu, p: _product(gpu, kc.get("dense_reuse_k20")),  # 2500 rows, all in the dense pass
    "other_width": lambda gpu, p: _product(gpu, kc.get("table_cut_c5000_k100")),  # another C: the accumulators are laid out anew
    "refused_args": lambda gpu, p: _product_refused(gpu),
    "refused_args_operands": _product_refused_operands,
    "refused_args_reason": "B repeats a column within a row",
}

LMF_C = 34


@functools.lru_cache(maxsize=None)
def _lmf_inputs(C=LMF_C, copies=1, scale=1.0):
    """(matrix, X0, Y0, G0) of the item side of sgd_cases.lmf_reduced_matrix -- its first row (600 entries) is cut into segments --,
    `copies` such matrices of consecutive seeds stacked."""
    sides = []
    for i in range(copies):
        mt = sgd.lmf_reduced_matrix(C, seed=C + i).T.tocsr()
        mt.sort_indices()
        sides.append(mt)
    mt = sp.vstack(sides).tocsr() if copies > 1 else sides[0]
    rng = np.random.default_rng(C)
    U = (rng.standard_normal((mt.shape[1], C)) * 0.3 * scale).astype(np.float32)
    V = (rng.standard_normal((mt.shape[0], C)) * 0.3 * scale).astype(np.float32)
    G0 = rng.uniform(0.0, 2.0, V.shape).astype(np.float32)
    return mt, V, U, G0


LMF_ARGS = (0.7, 0.2, 30, 5)  # lr, reg, neg_prop, seed: test_gpu_lmf.test_half_sweeps_match_float64


def _lmf(gpu, m, X0, Y0, G0):
    X, Y, G = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix(G0)
    gpu.lmf_update(gpu.CSRMatrix(m), X, Y, G, *LMF_ARGS)
    return {"X": X.to_numpy(), "G": G.to_numpy(), "Y": Y.to_numpy()}


def _lmf_gate(gpu, oracle, out):
    m, X0, Y0, G0 = _lmf_inputs()
    X64, G64, bX, bG = lref.half_sweep64(m, X0, Y0, G0, *LMF_ARGS)
    assert lref.within(out["X"], X64, bX)[0] and lref.within(out["G"], G64, bG)[0]
    assert bits(out["Y"]) == bits(Y0)


add("lmf-update", "lmf", "lmf_ws", lambda gpu: _lmf(gpu, *_lmf_inputs()), _lmf_gate,
    lambda oracle: list(lref.half_sweep64(*_lmf_inputs(), *LMF_ARGS)[:2]),
    ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "lmf.hip: a row's terms in a fixed order per lane group, long rows' segment partials added in order "
    "(test_bitwise_reproducible_and_seed_dependent)", lambda: _sizes(_lmf_inputs()[0]), lambda: _sizes(_lmf_inputs(LMF_C, 4, SCALE)[0]),
    matrix=lambda: _lmf_inputs()[0], classes=("long", "team16", "short16", "empty"))
PROBES["lmf-update"].extra = {
    "bigger": lambda gpu, p: _lmf(gpu, *_lmf_inputs(LMF_C, 4, SCALE)),  # four such item sides: four segmented rows
    "other_width": lambda gpu, p: _lmf(gpu, *_lmf_inputs(130)),
    "refused_args": lambda gpu, p: (lambda: _lmf(gpu, *p.extra["refused_args_operands"]())),
    "refused_args_operands": lambda: _lmf_inputs()[:3] + (_lmf_inputs()[3][:, :-1].copy(),),  # (matrix, X, Y, deriv_sum_sq)
    "refused_args_reason": "deriv_sum_sq has one column less than X",
}

WARP_C = sgd.SEARCH_C[0]


@functools.lru_cache(maxsize=None)
def _warp_inputs():
    m = sgd.search_matrix()
    X0, Y0 = sgd.warp_frozen_factors(m, WARP_C)
    return m, X0, Y0


def _warp(gpu, m, X0, Y0, lr=0.0, reg=0.0):
    import bpr_reference as bref

    userids, itemids = bref.coo_ids(m)
    uid, iid, ptr = gpu.IntVector(userids), gpu.IntVector(itemids), gpu.IntVector(np.asarray(m.indptr, dtype=np.int32))
    X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
    got = gpu.warp_epoch(uid, iid, ptr, X, Y, lr, reg, sgd.SEARCH_EPOCH_SEED, sgd.SEARCH_MAX_SAMPLED)
    return {"counts": np.array(got, dtype=np.int64), "X": X.to_numpy(), "Y": Y.to_numpy()}


@functools.lru_cache(maxsize=None)
def _warp_bigger():
    m = sp.vstack([sgd.search_matrix()] * 4).tocsr()
    m.sort_indices()
    X0, Y0 = sgd.warp_frozen_factors(m, WARP_C)
    return m, X0 * np.float32(4.0), Y0


def _warp_want():
    m, X0, Y0 = _warp_inputs()
    return wref.serial_epochs(m, X0, Y0, [sgd.SEARCH_EPOCH_SEED], 0.0, 0.0, sgd.SEARCH_MAX_SAMPLED, with_margin=True)[2][0]


def _warp_gate(gpu, oracle, out):
    m, X0, Y0 = _warp_inputs()
    assert tuple(out["counts"].tolist()) == tuple(_warp_want())  # test_gpu_warp.test_zero_learning_rate_epoch_is_exact
    assert bits(out["X"]) == bits(X0) and bits(out["Y"]) == bits(Y0)


add("warp-epoch-frozen", "pair-sgd", "pair_stats", lambda gpu: _warp(gpu, *_warp_inputs()), _warp_gate,
    lambda oracle: [np.array(_warp_want(), dtype=np.float64)], ["quiet", "bigger", "other_width", "refused_args", *ALWAYS],
    "lr = reg = 0: every store writes back what its lane loaded, so the Hogwild order cannot show; the counts are integer atomics "
    "(sgd_group.h:97-103); the only sgd_cases case its own file compares bit for bit -- bpr_epoch's frozen epoch is held to a range "
    "and the learning epochs of both are Hogwild, so they are left out", lambda: _sizes(_warp_inputs()[0]), lambda: _sizes(_warp_bigger()[0]))
PROBES["warp-epoch-frozen"].extra = {
    # four times the users, with a learning rate: factors move, the counts differ, pair_stats holds other values
    "bigger": lambda gpu, p: _warp(gpu, *_warp_bigger(), 0.05, 0.01),
    "other_width": lambda gpu, p: _warp(gpu, sgd.search_matrix(), *sgd.warp_frozen_factors(sgd.search_matrix(), sgd.SEARCH_C[1])),
    "refused_args": lambda gpu, p: (lambda: _warp(gpu, *p.extra["refused_args_operands"]())),
    "refused_args_operands": lambda: (_warp_inputs()[0], _warp_inputs()[1][:, :-1].copy(), _warp_inputs()[2]),  # (matrix, X, Y)
    "refused_args_reason": "X has one column less than Y",
}


# =================================================================================================================================
# 6. predecessors
# =================================================================================================================================
POOL_CLASSES = range(8, 23)  # 256 B .. 4 MB: Storage::kSmallMax (csrc/common.h)
POOL_BLOCKS = 8
# NaN in fp32 and fp16, -1 in int32, all ones in 64-bit keys; a large finite float.  Each is a predecessor of its own: the free
# lists are last in, first out, so a second fill takes the first one's blocks back and overwrites them
POOL_PATTERNS = {"pool_nan": 0xFFFFFFFF, "pool_finite": 0x7F7F7F7F}


def pool_arrays(pattern, size_class):
    return np.full((1, (1 << size_class) // 4), pattern, dtype=np.uint32).view(np.float32)


def fill_pool(gpu, pattern):
    """The recycled-block pool topped with loud bytes: per size class POOL_BLOCKS live matrices uploaded from the host, then
    dropped together, so that the next POOL_BLOCKS temporaries of every class start from `pattern`.  Only uploads and frees touch
    the blocks, no kernel computes on them."""
    held = [gpu.Matrix(pool_arrays(pattern, c)) for c in POOL_CLASSES for _ in range(POOL_BLOCKS)]
    del held
    gpu.synchronize()


# what the library says when it refuses an argument-kind predecessor, by the reason the probe states
REFUSAL_TEXT = {
    "YtY has one column more than Y": "YtY and Y should have the same number of columns",
    "1025 factors: calculate_loss takes at most 1024": "factors must be <= 1024",
    "X has one column more than Y": "X and Y should have the same number of columns",
    "block_size 33: the subspace sweep takes 1 .. 32": "block_size must be 1 .. 32",
    "weights is 16 x 16 for three users of 16 factors: it must have 48 rows": "weights must have Cui.rows * factors rows",
    "a 4 x 5 matrix is not square": "must be square",
    "the same orientation twice: not the two orientations of one matrix": "two orientations of one matrix",
    "a zero on the diagonal": "diagonal entry is zero or not finite",
    "D has one row more than A has columns": "do not agree",
    "W has one row more than Y has columns": "do not agree",
    "the queries have one column more than the items": "same number of columns",
    "k = 1025: ease_topk takes 1 .. 1024": "topk must lie in 1 .. 1024",
    "the queries have one column more than the index": "column count differs from the index",
    "ids has K + 1 columns": "ids must have k columns",
    "B repeats a column within a row": "repeats a column within a row",
    "deriv_sum_sq has one column less than X": "deriv_sum_sq must have the shape of X",
    "X has one column less than Y": "X and Y should have the same number of columns",
}


def _refused(kind):
    def run(gpu, p):
        call = p.extra[kind](gpu, p)
        try:
            call()
        except ValueError as e:
            if kind == "refused_args":  # refused for the stated reason, not for another
                assert REFUSAL_TEXT[p.extra["refused_args_reason"]] in str(e), (p.name, str(e))
            return
        raise AssertionError(f"{p.name}: the {kind} predecessor was not refused")

    return run


def _sequence(gpu, p):
    from test_gpu_knn_edges import _num_cus

    run_sequence(gpu, p.extra["kind"], _num_cus())


PREDECESSORS = {
    "quiet": lambda gpu, p: p.run(gpu),
    "bigger": lambda gpu, p: p.extra["bigger"](gpu, p),
    "other_width": lambda gpu, p: p.extra["other_width"](gpu, p),
    "refused_args": _refused("refused_args"),
    "refused_pivot": _refused("refused_pivot"),
    "released": lambda gpu, p: gpu.release_workspaces(),
    "pool_nan": lambda gpu, p: fill_pool(gpu, POOL_PATTERNS["pool_nan"]),
    "pool_finite": lambda gpu, p: fill_pool(gpu, POOL_PATTERNS["pool_finite"]),
    # the context's grow-only workspaces dropped first, so that their next blocks come from the NaN-filled lists too
    "released_pool_nan": lambda gpu, p: (gpu.release_workspaces(), fill_pool(gpu, POOL_PATTERNS["pool_nan"])),
    "sequence": _sequence,
}


def run_predecessor(gpu, probe, name):
    if name.startswith("cross:"):
        PROBES[name[6:]].run(gpu)
    else:
        PREDECESSORS[name](gpu, probe)


def cells():
    return [(p.name, pred) for p in PROBES.values() for pred in p.before]


# ---- sequences --------------------------------------------------------------------------------------------------------------------
CHAIN_WORKGROUPS_PER_CU, WIDE_WORKGROUPS_PER_CU = 2, 1  # launch_team_chain / launch_wide_chain on the MI355X (tests/test_gpu_cg_*_chain.py)
CHAIN_TEAMS = (1, 2, 4)  # teams of width 8 / 4 / 2 in a workgroup of 8 wavefronts
SEQUENCE_SOLVER_ROWS = (1000, 500, 240, 60, 300)  # the other two families: the size of `fifth`


def static_cut(num_cus):
    """Rows up to which a class is served by static tickets alone, four per team: (team2, team4, team8, team16, short rows)."""
    chain, wide = num_cus * CHAIN_WORKGROUPS_PER_CU, num_cus * WIDE_WORKGROUPS_PER_CU
    return (4 * chain * 4, 4 * chain * 2, 4 * chain * 1, 4 * wide, 4 * wide * 16)


def sequence_counts(num_cus=256):
    """A dozen class-count vectors (team2, team4, team8, team16, short rows) for the f = 128 CG half sweep on a device of num_cus
    CUs: every class empty, below three rows per team (no draw), between three and four (draws past the end only), at the cut, one
    past it and well past it, in changing company.  At 256 CUs the largest holds the rows of `drawn`."""
    c2, c4, c8, c16, cs = static_cut(num_cus)
    return [
        (0, 0, 0, 0, 40),
        (c2 + c2 // 8, 0, c8 - 1, 0, 0),
        (0, c4 + 1, 0, c16 // 2, cs // 4),
        (c2 * 3 // 4 + 9, c4 * 3 // 4 - 5, c8 + c8 // 8, 0, 0),
        (5, 3, 1, 1, 17),
        (c2, c4, c8, c16, 0),
        (0, 0, c8 + 1, c16 + 1, cs + 16),
        (c2 - 1, c4 - 1, 0, c16 * 3 // 4 + 9, 0),
        (c2 + 1, 0, c8 * 3 // 4 + 9, c16 + c16 // 4, cs * 3 // 4 + 160),
        (0, c4 + c4 // 8, c8 * 3 // 4 - 5, c16 - 1, cs),
        (c2 * 3 // 4 - 5, c4 * 3 // 4 + 9, c8, 0, cs + cs // 8),
        (0, 0, 0, 0, 0),
    ]


def run_sequence(gpu, kind, num_cus):
    """About a dozen half sweeps in a row on one solver object, every one on another matrix; nothing is checked here -- a wrong
    draw prediction shifts the base of the NEXT launch, which is the probe's."""
    solver = gpu.LeastSquaresSolver()
    for i, counts in enumerate(sequence_counts(num_cus)):
        if kind != "cg":  # the other families draw no tickets from kept counters: same class mix, at the size of `fifth`
            counts = tuple(min(c, s) for c, s in zip(counts, SEQUENCE_SOLVER_ROWS))
        f = {"cg": 128, "cholesky": 128, "subspace": SUB_F}[kind]
        C, X0, Y0 = _class_inputs(counts, 100 + i, f)
        Xd, Yd, G = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix.zeros(f, f)
        if kind == "cg":
            solver.calculate_yty(Yd, G, 0.05)
            solver.least_squares(gpu.CSRMatrix(C), Xd, G, Yd, 3)
        elif kind == "cholesky":
            solver.calculate_yty(Yd, G, 0.0)
            solver.least_squares_cholesky(gpu.CSRMatrix(C), Xd, G, Yd, 0.05)
        else:
            solver.calculate_yty(Yd, G, 0.0)
            solver.least_squares_subspace(gpu.CSRMatrix(C), Xd, G, Yd, 0.05, SUB_K, 1)


# ---- the fresh child process ------------------------------------------------------------------------------------------------------
def run_fresh():
    """Body of the child process of test_fresh_process: every probe once, in table order, nothing else; prints one JSON line of
    digests.  The first probe of every family is the first call of that family in the process."""
    import warnings

    warnings.simplefilter("ignore")
    import implicit_amd.gpu as gpu

    print("history digests " + json.dumps({name: digest(p.run(gpu)) for name, p in PROBES.items()}))
