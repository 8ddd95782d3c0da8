"""Every in-place writer of a factor matrix against every piece of state the library derives from one and keeps between calls.

Derived state (csrc/common.h): the fragment-ordered fp16 item planes of a KnnQuery handle (topk.hip, split_planes), the
zero-padded copy of Y of the padded CG half sweep (als_pad.hip, pad_in), and on the Python side the top-k handle, norms and
gramians a model keeps.  Each is right only while every write to the matrix is reported, or while the library refuses to keep
anything of memory it cannot watch.  Inside the library that is no longer a line per writer: the only way to a mutable device
pointer of a matrix is its write accessor (imp_matrix::mut_rows, common.h), which reports exactly the bytes it hands out.  A
miss gives no crash and no NaN: it gives the previous contents' answer.

A cell = one writer x one consumer, always the same four beats:
  1. the matrix holds A; the consumer's answer is the reference's for A;
  2. the cache is shown to be LIVE: the same call again answers bit for bit the same and the profiling scope that counts
     rebuilds ("item_planes_split": one per split of the item matrix; "padded_y_check": one per call that found a kept copy of
     Y to vouch for) says nothing was rebuilt.  A cell on memory the library must never cache from asserts the opposite count;
  3. the writer leaves contents B behind the same handle;
  4. the same consumer state answers for B: the reference's answer for B, and what fresh state on a fresh copy of B gives,
     bit for bit.
Top-k reference: the float64 score matrix under a stable descending sort; agreement = share of equal id positions, at least
0.99 (the bar of test_item_plane_cache_follows_writes), with the fp32 CPU oracle as a second opinion held to the same bar.
reference(A) and reference(B) agree on less than 0.2 of the positions in every cell, so stale state cannot pass; partial writers
scale what they write until it takes at least half of the places of reference(A)'s top-k.  At 4096 items, 64 queries and
k = 10 every factor count here runs the materialising route on the resident planes (emit_stride < 8), which is the caching
route: beat 2 fails otherwise.  Padded-copy reference: the CPU oracle under the gramian the solver was handed, row by row within
the parity gate of test_gpu_solver_routes.py; the staleness check hands the solver the OLD gramian after the write, as
test_padded_copy_of_y_is_reused_only_while_it_is_valid does, so that only the write notification can save the answer.

Writers: 1 copy_from_numpy, 2 assign_rows (every third row), 3 copy_rows_from (a row range), 4 resize + copy_from_numpy and
destroy + create (the pool hands the freed block out again), 5 CG sweep and 6 Cholesky sweep into the matrix (all rows, and a
row-slice view), 8 a write through an address obtained with device_ptr AFTER the cache was live, 9 foreign memory wrapped
through __cuda_array_interface__ and rewritten behind the library's back, 10 calculate_yty with the matrix as its OUTPUT (a
square Y, 100 items x 100 factors: the one writer that had no notification line of its own).

Cells left out, and why:
  * 7 bpr_epoch / lmf_update x planes: test_gpu_bpr.py::test_plane_cache_invalidated_by_bpr_epoch and
    test_gpu_lmf.py::test_plane_cache_invalidated_by_lmf_update are those cells;
  * 5 / 6 x padded copy ("the matrix a sweep wrote is the Y of the next one") for every sweep that pads: its own pad_in
    replaces (CG) or forgets (Cholesky, 64 < f < 128) the kept copy whatever it reports, the cell could not fail.  The
    Cholesky sweep at f = 32 pads nothing and is the one such cell here; the model cells run the whole two-half-sweep sequence;
  * padded copy x fp16: fp16 factors at a padded factor count are solved on fp32 temporaries that die with the call, nothing
    of them survives to go stale;
  * cosine form x sweeps: a sweep leaves empty rows zero, and a zero row's cosine is a 0 / 1e-10 tie by construction;
  * 9 with a torch tensor as the foreign memory: the PyTorch ROCm wheel loads the HIP runtime it bundles, this library the
    system's, and in a process where the library's runtime holds the device torch.cuda.is_available() is False -- there is
    no tensor to wrap.  The foreign memory here is a hipMalloc block of the runtime the library itself runs on, published
    through the same __cuda_array_interface__ a tensor has and rewritten with hipMemcpy: to the library it is as foreign
    as a tensor (Storage::owned == false);
  * the comm.hip writers (no peer to exercise them) and anything across devices.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_equal

from implicit_amd.synthetic import synthetic_csr

pytestmark = pytest.mark.gpu

NI, NQ, K = 4096, 64, 10
AGREE, APART = 0.99, 0.2
TOL = {"float32": 1e-4, "float16": 1e-3}  # tests/test_gpu_solver_routes.py
REG = 0.05
PARTIAL_SCALE = 4.0  # rows a partial writer writes, against the rows they replace


# ---- references and measures ------------------------------------------------------------------------------------------------
def rank64(items, queries, k=K, cosine=False):
    """ids of the k best items per query row: float64 scores, stable descending sort; cosine: scores / ||item|| (0 -> 1e-10)."""
    items, queries = np.asarray(items, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    scores = queries @ items.T
    if cosine:
        norms = np.linalg.norm(items, axis=1)
        norms[norms == 0] = 1e-10
        scores /= norms[None, :]
    return np.argsort(-scores, axis=1, kind="stable")[:, :k].astype(np.int32)


def agreement(got, want):
    assert got.shape == want.shape
    return float((np.asarray(got) == np.asarray(want)).mean())


def displaced(ref_a, ref_b):
    """Share of reference(A)'s top-k members that are no longer among reference(B)'s of the same query."""
    gone = [len(set(ra.tolist()) - set(rb.tolist())) for ra, rb in zip(ref_a, ref_b)]
    return float(np.sum(gone)) / ref_a.size


class Scope:
    """Launch count of ONE profiling scope while the block runs, under a name filter: the two scopes read here are nested in
    others and only recorded when asked for by name, and unfiltered profiling changes kernel routes."""

    def __init__(self, gpu, name):
        self.gpu, self.name = gpu, name

    def __enter__(self):
        self.gpu.Profiler.reset()
        self.gpu.Profiler.enable(True, only=self.name)
        return self

    def __call__(self):
        return self.gpu.Profiler.get(self.name)[1]

    def __exit__(self, *exc):
        self.gpu.Profiler.enable(False)
        self.gpu.Profiler.reset()


# ---- memory the library does not own, and writes it does not see -------------------------------------------------------------
def _runtime(gpu):
    """The HIP runtime the library is linked against, through the library's own handle (dlsym searches its dependencies)."""
    from implicit_amd.gpu._hip import lib

    rt = lib()
    rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    rt.hipFree.argtypes = [ctypes.c_void_p]
    rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    rt.hipDeviceSynchronize.argtypes = []
    return rt


def raw_write(gpu, device_ptr, host):
    """host -> device_ptr with a plain blocking hipMemcpy: a write the library is not told about."""
    host = np.ascontiguousarray(host)
    rt = _runtime(gpu)
    gpu.synchronize()
    assert rt.hipMemcpy(ctypes.c_void_p(device_ptr), ctypes.c_void_p(host.ctypes.data), host.nbytes, 1) == 0  # hipMemcpyHostToDevice
    assert rt.hipDeviceSynchronize() == 0
    gpu.synchronize()


class ForeignBuffer:
    """A device block that is not the library's, with the __cuda_array_interface__ of a 2-d C-contiguous array."""

    def __init__(self, gpu, host):
        host = np.ascontiguousarray(host)
        self.gpu, self.shape, self.typestr = gpu, host.shape, host.dtype.str
        p = ctypes.c_void_p()
        assert _runtime(gpu).hipMalloc(ctypes.byref(p), host.nbytes) == 0
        self.ptr = p.value
        self.write(host)

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.typestr, "data": (self.ptr, False), "version": 2}

    def write(self, host):
        assert host.shape == self.shape and host.dtype.str == self.typestr
        raw_write(self.gpu, self.ptr, host)

    def close(self):
        if self.ptr:
            self.gpu.synchronize()
            assert _runtime(self.gpu).hipFree(ctypes.c_void_p(self.ptr)) == 0
            self.ptr = None


class Cell:
    """What a writer works on: hold[0] is THE handle (writers may replace it, nothing else keeps a reference to it)."""

    def __init__(self, gpu, contents, foreign=False):
        self.gpu, self.foreign = gpu, ForeignBuffer(gpu, contents) if foreign else None
        self.hold = [gpu.Matrix(self.foreign if foreign else contents)]
        self.written = None  # row ids of a partial write

    @property
    def m(self):
        return self.hold[0]

    def close(self):
        self.hold[0] = None
        if self.foreign:
            self.foreign.close()


# ---- writers 1-4, 8, 9: (cell, A, B, big) -> contents afterwards; `big`: rows PARTIAL_SCALE times as large as A's ------------
def w_copy_from_numpy(cell, a, b, big):
    cell.m.copy_from_numpy(b)
    return b


def w_assign_rows(cell, a, b, big):
    rows = np.arange(0, len(a), 3, dtype=np.int32)
    cell.m.assign_rows(rows, cell.gpu.Matrix(big[rows]))
    out = a.copy()
    out[rows] = big[rows]
    cell.written = rows
    return out


def w_copy_rows_from(cell, a, b, big):
    lo, hi = len(a) // 4, len(a) // 4 + (3 * len(a)) // 8
    cell.m.copy_rows_from(lo, cell.gpu.Matrix(big), lo, hi - lo)
    out = a.copy()
    out[lo:hi] = big[lo:hi]
    cell.written = np.arange(lo, hi)
    return out


def w_resize_then_copy(cell, a, b, big):
    extra = max(1, len(a) // 32)
    out = np.concatenate([b, a[:extra]])
    cell.m.resize(len(out), a.shape[1])
    cell.m.copy_from_numpy(out)
    return out


def w_destroy_and_create(cell, a, b, big):
    """The block goes back to the pool and the new matrix of the same size most likely gets it: whichever address it got, the
    answer is for the new contents."""
    cell.hold[0] = None  # the only reference: imp_matrix_destroy runs here
    cell.hold[0] = cell.gpu.Matrix(b)
    return b


def w_device_ptr_write(cell, a, b, big):
    raw_write(cell.gpu, cell.m.device_ptr, b)
    return b


def w_foreign_rewrite(cell, a, b, big):
    cell.foreign.write(b)
    return b


CONTAINER_WRITERS = [w_copy_from_numpy, w_assign_rows, w_copy_rows_from, w_resize_then_copy, w_destroy_and_create]
UNTRACKED_WRITERS = [w_device_ptr_write, w_foreign_rewrite]


def writer_id(w):
    return w.__name__[2:]


# ---- consumer 1: the item planes of a KnnQuery handle ------------------------------------------------------------------------
TOPK_CONFIGS = [(64, "float32"), (64, "float16"), (32, "float16"), (40, "float32")]  # f = 40 reaches the planes through pad_items


@functools.lru_cache(maxsize=None)
def topk_inputs(f, dtype, cosine=False, a_scale=0.1):
    """(A, B, queries, big) in their storage type, read-only.  Cosine cells give every row its own length (0.5 .. 2), so that
    the norms matter -- and since no length moves a cosine, their `big` rows lean towards one query row each instead."""
    rng = np.random.default_rng(100 * f + (1 if dtype == "float16" else 0))
    a, b, big, q = (rng.standard_normal((n, f)) for n in (NI, NI, NI, NQ))
    if cosine:
        big += 3.0 * q[rng.integers(NQ, size=NI)]
        a, b, big = (m * rng.uniform(0.5, 2.0, (NI, 1)) for m in (a, b, big))
    out = [(a * a_scale).astype(dtype), (b * 0.1).astype(dtype), (q * 0.1).astype(dtype), (big * 0.1 * PARTIAL_SCALE).astype(dtype)]
    for m in out:
        m.setflags(write=False)
    return tuple(out)


def run_topk_cell(gpu, oracle, a, q, write, foreign=False, exposes=False, cosine=False):
    """The four beats on the item planes.  `write(cell)` applies the writer and returns the contents it left; `foreign`: the
    items live in memory the library does not own; `exposes`: the writer hands the address out (nothing is kept afterwards)."""
    knn, Q = gpu.KnnQuery(), gpu.Matrix(q)
    cell = Cell(gpu, a, foreign)
    trusted = not foreign

    def query(handle, items):
        norms = gpu.calculate_norms(items) if cosine else None  # recomputed from the current contents
        return handle.topk(items, Q, K, item_norms=norms)

    try:
        with Scope(gpu, "item_planes_split") as splits:
            ref_a = rank64(a, q, cosine=cosine)
            ids, dist = query(knn, cell.m)                                    # 1
            assert agreement(ids, ref_a) >= AGREE
            assert splits() == 1
            again = query(knn, cell.m)                                        # 2
            assert_array_equal(again[0], ids)
            assert_array_equal(again[1], dist)
            assert splits() == (1 if trusted else 2), "the route does not cache" if trusted else "foreign memory was cached from"
            b = write(cell)                                                   # 3
            ref_b = rank64(b, q, cosine=cosine)
            print(f"reference(A) vs reference(B): {agreement(ref_a, ref_b[:, :K]):.3f} equal, {displaced(ref_a, ref_b):.3f} displaced")
            assert b.shape[1:] == a.shape[1:] and agreement(ref_a, ref_b) < APART
            if cell.written is not None:
                assert displaced(ref_a, ref_b) >= 0.5 and np.isin(ref_b, cell.written).mean() >= 0.5
            norms_b = np.linalg.norm(b.astype(np.float64), axis=1) if cosine else None
            assert agreement(oracle.topk(b, q, K, item_norms=norms_b)[0], ref_b) >= AGREE  # the second opinion
            before = splits()
            ids_b, dist_b = query(knn, cell.m)                                # 4
            print(f"same handle vs reference(B): {agreement(ids_b, ref_b):.4f}; vs reference(A): {agreement(ids_b, ref_a):.4f}")
            assert agreement(ids_b, ref_b) >= AGREE
            assert splits() == before + 1
            fresh = query(gpu.KnnQuery(), gpu.Matrix(b))
            assert_array_equal(ids_b, fresh[0])
            assert_array_equal(dist_b, fresh[1])
            if trusted and not exposes:                                       # and the new planes are kept in their turn
                assert_array_equal(query(knn, cell.m)[0], ids_b)
                assert splits() == before + 2  # (+ 1: the fresh handle's)
    finally:
        cell.close()


@pytest.mark.parametrize("f,dtype", TOPK_CONFIGS, ids=lambda v: str(v))
@pytest.mark.parametrize("writer", CONTAINER_WRITERS + UNTRACKED_WRITERS, ids=writer_id)
def test_planes_follow_container_writes(gpu, oracle, writer, f, dtype):
    a, b, q, big = topk_inputs(f, dtype)
    run_topk_cell(gpu, oracle, a, q, lambda cell: writer(cell, a, b, big), foreign=writer is w_foreign_rewrite,
                  exposes=writer is w_device_ptr_write)


@pytest.mark.parametrize("writer", CONTAINER_WRITERS + UNTRACKED_WRITERS, ids=writer_id)
def test_planes_follow_container_writes_cosine(gpu, oracle, writer):
    """The cosine form scores on the same planes: item_norms= recomputed after the write."""
    a, b, q, big = topk_inputs(64, "float32", cosine=True)
    run_topk_cell(gpu, oracle, a, q, lambda cell: writer(cell, a, b, big), foreign=writer is w_foreign_rewrite,
                  exposes=writer is w_device_ptr_write, cosine=True)


# writers 5 and 6: a half sweep into the item matrix, the queries as the other side's factors (what fit() does between
# recommend() calls).  fp16 at f = 32 / 96 is solved on an fp32 temporary and copied back (solver.hip, run_with_f32)
SWEEPS = ([("cg", f, dtype) for f, dtype in [(64, "float32"), (100, "float32"), (32, "float32"), (64, "float16"), (32, "float16"), (96, "float16")]]
          + [("cholesky", 64, "float32"), ("cholesky", 32, "float16")])
SLICE = (NI // 4, NI // 4 + NI // 2)


@functools.lru_cache(maxsize=None)
def sweep_matrix():
    """items x queries: every item row has entries, so a sweep rewrites every row it covers."""
    C = synthetic_csr(NI, NQ, 12_000, seed=4)
    assert (np.diff(C.indptr) > 0).all()
    return C


@pytest.mark.parametrize("rows", ["all", "slice"])
@pytest.mark.parametrize("solver_kind,f,dtype", SWEEPS, ids=lambda v: str(v))
def test_planes_follow_solver_sweeps(gpu, oracle, solver_kind, f, dtype, rows):
    """A holds rows a tenth as long as the other cells': the rows a sweep solves (scores near 1 on what the row likes) take the
    top of every ranking, also where only the slice is solved."""
    a, _, q, _ = topk_inputs(f, dtype, a_scale=0.01)
    C = sweep_matrix()

    def write(cell):
        solver, Q, gram = gpu.LeastSquaresSolver(), gpu.Matrix(q), gpu.Matrix.zeros(f, f)
        lo, hi = (0, NI) if rows == "all" else SLICE
        X = cell.m if rows == "all" else cell.m[lo:hi]
        Cd = gpu.CSRMatrix(C[lo:hi])
        if solver_kind == "cg":
            solver.calculate_yty(Q, gram, REG)
            solver.least_squares(Cd, X, gram, Q, 3)
        else:
            solver.calculate_yty(Q, gram, 0.0)
            solver.least_squares_cholesky(Cd, X, gram, Q, REG)
        now = cell.m.to_numpy()
        assert_array_equal(now[:lo], a[:lo])
        assert_array_equal(now[hi:], a[hi:])
        assert np.isfinite(now.astype(np.float32)).all()
        if rows == "slice":
            cell.written = np.arange(lo, hi)
        return now

    run_topk_cell(gpu, oracle, a, q, write)


# ---- consumer 2: the zero-padded copy of Y of the padded CG half sweep --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pad_inputs(f, square=False):
    """square: Y has as many rows (items) as columns, so that it can stand where a gramian is written."""
    users, items = (48, f) if square else (600, 300)
    C = synthetic_csr(users, items, 15 * users, seed=11, empty_frac=0.1 if square else 0.03)
    assert (np.diff(C.indptr) == 0).any()
    rng = np.random.default_rng(f)
    X0, YA, YB, big = (rng.random((n, f), dtype=np.float32) * 0.2 - 0.1 for n in (users, items, items, items))
    big = big * np.float32(PARTIAL_SCALE)
    for m in (X0, YA, YB, big):
        m.setflags(write=False)
    return C, X0, YA, YB, big


def w_cholesky_sweep_into_y(cell, a, b, big):
    """Writer 6 for this consumer: the matrix that is Y here is the X of the other half sweep (f = 32: no padding there, the
    kept copy is only dropped if the sweep reports its write)."""
    gpu, f = cell.gpu, a.shape[1]
    C, X0 = pad_inputs(f)[:2]
    solver, other, gram = gpu.LeastSquaresSolver(), gpu.Matrix(X0), gpu.Matrix.zeros(f, f)
    solver.calculate_yty(other, gram, 0.0)
    solver.least_squares_cholesky(gpu.CSRMatrix(C.T.tocsr()), cell.m, gram, other, REG)
    return cell.m.to_numpy()


def w_gramian_into_y(cell, a, b, big):
    """Writer 10: the matrix that is Y here is the output of calculate_yty (Z^T Z of a small random Z of as many columns)."""
    gpu, f = cell.gpu, a.shape[1]
    assert a.shape == (f, f)
    Z = (np.random.default_rng(f + 1).random((16, f), dtype=np.float32) * 0.4 - 0.2).astype(np.float32)
    gpu.LeastSquaresSolver().calculate_yty(gpu.Matrix(Z), cell.m, 0.0)
    return cell.m.to_numpy()


def rows_rel(got, want, lens):
    """Worst relative distance of a non-empty row; empty rows must be zero."""
    assert not got[lens == 0].any()
    diff = np.linalg.norm(got.astype(np.float64) - want, axis=1)[lens > 0]
    return float((diff / np.maximum(np.linalg.norm(want.astype(np.float64), axis=1)[lens > 0], 1e-30)).max())


PAD_CELLS = ([(f, w) for f in (100, 32) for w in CONTAINER_WRITERS + UNTRACKED_WRITERS] + [(32, w_cholesky_sweep_into_y)]
             + [(100, w_gramian_into_y)])


@pytest.mark.parametrize("f,writer", PAD_CELLS, ids=lambda v: writer_id(v) if callable(v) else str(v))
def test_padded_copy_of_y_follows_writes(gpu, oracle, f, writer):
    C, X0, YA, YB, big = pad_inputs(f, square=writer is w_gramian_into_y)
    lens = np.diff(C.indptr)
    foreign = writer is w_foreign_rewrite
    trusted = not foreign
    solver, Cd = gpu.LeastSquaresSolver(), gpu.CSRMatrix(C)
    gpu.release_workspaces()  # no kept copy of an earlier test
    cell = Cell(gpu, YA, foreign)

    def sweep(Y, gram, state=solver):
        X = gpu.Matrix(X0)
        state.least_squares(Cd, X, gram, Y, 3)
        return X.to_numpy()

    def oracle_sweep(Y, gram):
        want = X0.copy()
        oracle.least_squares_cg(C, want, Y, REG, cg_steps=3, YtY=gram.to_numpy())
        return want

    try:
        gram = gpu.Matrix.zeros(f, f)
        solver.calculate_yty(cell.m, gram, REG)
        with Scope(gpu, "padded_y_check") as checks:
            first = sweep(cell.m, gram)                                       # 1
            err = rows_rel(first, oracle_sweep(YA, gram), lens)
            print(f"A: worst row {err:.2e}")
            assert err < TOL["float32"]
            assert checks() == 0
            assert_array_equal(sweep(cell.m, gram), first)                    # 2
            kept = checks()
            if trusted:
                assert kept == 1, "the route keeps no copy"
            b = writer(cell, YA, YB, big)                                     # 3
            stale_gram = sweep(cell.m, gram)                                  # 4: the caller's gramian is still A's
            after = checks()
            gpu.release_workspaces()
            fresh = sweep(gpu.Matrix(b), gpu.Matrix(gram.to_numpy()), gpu.LeastSquaresSolver())
            assert_array_equal(stale_gram, fresh)
            assert not np.array_equal(stale_gram, first)                      # (B is not A: a stale copy would have shown)
            assert after == kept, "the kept copy survived the write"
            assert trusted or kept == 0, "a copy of foreign memory was kept"
            solver.calculate_yty(cell.m, gram, REG)                           # and with the gramian that goes with B
            err = rows_rel(sweep(cell.m, gram), oracle_sweep(b, gram), lens)
            print(f"B: worst row {err:.2e}")
            assert err < TOL["float32"]
    finally:
        cell.close()


# ---- consumer 3: what a model keeps across fit / partial_fit ---------------------------------------------------------------
USERS, ITEMS, MODEL_NNZ = 400, 300, 6000
QUERY_USERS = np.arange(NQ)
REFIT_ITEMS = np.arange(0, ITEMS, 3)  # every third item: what partial_fit_items rewrites, and the similar_items queries
MODELS = [(32, "float16"), (64, "float32"), (100, "float32")]


@functools.lru_cache(maxsize=None)
def model_data():
    """Two unrelated interaction matrices of one shape (the second with its popular items elsewhere), and the rows of the
    partial fits: every refitted item liked by a random third of all users, every second queried user by a random tenth of the
    items, both with high confidence -- their predictions move to the top of the rankings."""
    first = synthetic_csr(USERS, ITEMS, MODEL_NNZ, seed=21)
    rng = np.random.default_rng(22)
    second = synthetic_csr(USERS, ITEMS, MODEL_NNZ, seed=23)[:, rng.permutation(ITEMS)].tocsr()
    second.sort_indices()
    item_users = sp.random(len(REFIT_ITEMS), USERS, density=0.33, format="csr", dtype=np.float32, random_state=24)
    item_users.data = 20 + 20 * item_users.data
    user_items = sp.random(len(QUERY_USERS[::2]), ITEMS, density=0.1, format="csr", dtype=np.float32, random_state=25)
    user_items.data = 20 + 20 * user_items.data
    return first, second, item_users, user_items


def model_answers(model):
    rec = model.recommend(QUERY_USERS, None, N=K, filter_already_liked_items=False)[0]
    sim = model.similar_items(REFIT_ITEMS[:NQ], N=K)[0]
    return rec, sim


def model_references(model):
    X, Y = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    return rank64(Y, X[QUERY_USERS]), rank64(Y, Y[REFIT_ITEMS[:NQ]], cosine=True)


def run_model_cell(gpu, model, fit, rewrite, answers=model_answers, state=None):
    """`state()`: what tells a rebuild of the derived state from a re-use (default: the count of item-plane splits)."""
    with Scope(gpu, "item_planes_split") as splits:
        state = state or splits
        fit(model)
        got_a, ref_a = answers(model), model_references(model)               # 1
        for got, ref in zip(got_a, ref_a):
            assert agreement(got, ref) >= AGREE
        built = state()
        assert built
        for again, got in zip(answers(model), got_a):                        # 2
            assert_array_equal(again, got)
        assert state() == built
        rewrite(model)                                                        # 3
        got_b, ref_b = answers(model), model_references(model)               # 4
        for name, got, ra, rb in zip(("recommend", "similar_items"), got_b, ref_a, ref_b):
            print(f"{name}: reference(A) vs reference(B) {agreement(ra, rb):.3f}, got vs reference(B) {agreement(got, rb):.4f}")
            assert agreement(ra, rb) < APART
            assert agreement(got, rb) >= AGREE
        assert state() != built
    return got_b


def fresh_model_answers(gpu, model):
    """The same queries on a fresh model object holding fresh copies of the factors."""
    import implicit_amd.gpu.als as gals

    fresh = gals.AlternatingLeastSquares(factors=model.factors, dtype=model.dtype)
    fresh.user_factors, fresh.item_factors = gpu.Matrix(model.user_factors.to_numpy()), gpu.Matrix(model.item_factors.to_numpy())
    return model_answers(fresh)


@pytest.mark.parametrize("sequence", ["refit", "partial_fit"])
@pytest.mark.parametrize("factors,dtype", MODELS, ids=lambda v: str(v))
def test_model_answers_follow_its_factors(gpu, factors, dtype, sequence):
    """fit -> recommend + similar_items -> fit on other data / partial_fit_items + partial_fit_users, same model object -> the
    same queries: the model keeps its KnnQuery handle (and the item planes in it) across all of it."""
    import implicit_amd.gpu.als as gals

    first, second, item_users, user_items = model_data()
    model = gals.AlternatingLeastSquares(factors=factors, dtype=np.dtype(dtype), iterations=3, regularization=REG, random_state=3)

    def partial_fit(m):
        m.partial_fit_items(REFIT_ITEMS, item_users)
        m.partial_fit_users(QUERY_USERS[::2], user_items)

    rewrite = (lambda m: m.fit(second, show_progress=False)) if sequence == "refit" else partial_fit
    got = run_model_cell(gpu, model, lambda m: m.fit(first, show_progress=False), rewrite)
    for mine, fresh in zip(got, fresh_model_answers(gpu, model)):
        assert_array_equal(mine, fresh)


def test_ivf_model_answers_follow_a_refit(gpu):
    """IVFAlternatingLeastSquares keeps two IVF indexes built from the item factors; fit() rebuilds them.  Every list probed,
    as in test_gpu_ann_model.py: the approximate answers are the exact ranking's."""
    from implicit_amd.approximate_als import IVFAlternatingLeastSquares

    first, second = model_data()[:2]
    wrapped = IVFAlternatingLeastSquares(factors=32, iterations=3, regularization=REG, random_state=7, nlist=12, nprobe=12, use_gpu=True)

    def answers(model):
        assert model is wrapped.model
        return (wrapped.recommend(QUERY_USERS, None, N=K, filter_already_liked_items=False)[0],
                wrapped.similar_items(REFIT_ITEMS[:NQ], N=K)[0])

    run_model_cell(gpu, wrapped.model, lambda m: wrapped.fit(first, show_progress=False),
                   lambda m: wrapped.fit(second, show_progress=False), answers,
                   state=lambda: (wrapped.recommend_index, wrapped.similar_items_index))  # the index objects themselves
