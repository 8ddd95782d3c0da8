"""Python surface of the `implicit.gpu` plug-in, re-hosted on libimplicit_hip.so.

Mirrors, name for name and argument for argument, the classes the reference exposes from its
Cython module implicit/gpu/_cuda.pyx (file:line cited per class): RandomState, KnnQuery, Matrix,
IntVector, CSRMatrix, COOMatrix, LeastSquaresSolver, calculate_norms, get_device_count,
bpr_update.  Host code stays Python; every heavy call goes through the C-ABI with the GIL
released (ctypes.CDLL does that), as the reference does with `with nogil` (_cuda.pyx:79,257,264,271).

NEW relative to the reference: LeastSquaresSolver.least_squares_cholesky (the reference GPU path
has no Cholesky solver), the Comm class (RCCL exchange for the multi-GPU fit), lmf_update (the
reference has no GPU LMF), SpMat / sparse_topk_product (the reference's nearest-neighbour models are CPU only), IVFIndex
(a native IVF-Flat index in place of the faiss one the reference's ann wrappers build) and ease_gram / spd_inverse /
ease_weights / ease_topk (the EASE model, which the reference does not have), slim_solve (the SLIM model, likewise), and
spmm / multiply_small (the products of the randomized SVD behind PureSVD, which the reference does not have either).
"""
import ctypes

import numpy as np

from ..utils import check_csr
from ._hip import check, lib


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _check_failing(fn, *args, attr="failed_row"):
    """check(fn(*args, &failed)) for the entry points that report where a factorisation failed: a ValueError leaves with
    `attr` set to the smallest failing index, -1 unless the factorisation itself failed (an argument error)."""
    failed = ctypes.c_int64(-1)
    try:
        check(fn(*args, ctypes.byref(failed)))
    except ValueError as e:
        setattr(e, attr, failed.value)
        raise


class RandomState:
    """_cuda.pyx:25-42"""

    def __init__(self, seed=42):
        self._h = ctypes.c_void_p()
        check(lib().imp_random_create(int(seed), ctypes.byref(self._h)))

    def uniform(self, rows, cols, low=0.0, high=1.0):
        ret = Matrix(None)
        check(lib().imp_random_uniform(self._h, rows, cols, float(low), float(high), ctypes.byref(ret._h)))
        return ret

    def randn(self, rows, cols, mean=0.0, stddev=1.0):
        ret = Matrix(None)
        check(lib().imp_random_randn(self._h, rows, cols, float(mean), float(stddev), ctypes.byref(ret._h)))
        return ret

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_random_destroy(self._h)
            self._h = None


class KnnQuery:
    """_cuda.pyx:45-83"""

    def __init__(self, max_temp_memory=0):
        self._h = ctypes.c_void_p()
        check(lib().imp_knn_create(int(max_temp_memory), ctypes.byref(self._h)))

    def topk(self, items, m, k, item_norms=None, query_filter=None, item_filter=None):
        if not isinstance(items, Matrix) or not isinstance(m, Matrix):
            raise TypeError("KnnQuery.topk expects implicit.gpu.Matrix arguments")
        k = int(k)
        rows = m.shape[0]
        indices = np.zeros((rows, k), dtype="int32")
        distances = np.zeros((rows, k), dtype="float32")
        check(lib().imp_knn_topk(
            self._h, items._h, m._h, k, _vp(indices), _vp(distances),
            item_norms._h if item_norms is not None else None,
            query_filter._h if query_filter is not None else None,
            item_filter._h if item_filter is not None else None))
        return indices, distances

    def topk_device(self, items, m, k, item_norms=None, query_filter=None, item_filter=None):
        """NEW: the same call with DEVICE output buffers (knn.cu:40-54,147-164 detects where its output pointers live): returns
        (ids, distances) as two rows x k device Matrix objects; the ids are int32 bit patterns in a 4-byte-per-element
        matrix (`ids.to_numpy().view(np.int32)`).  For callers that keep post-processing on the device."""
        if not isinstance(items, Matrix) or not isinstance(m, Matrix):
            raise TypeError("KnnQuery.topk expects implicit.gpu.Matrix arguments")
        k = int(k)
        rows = m.shape[0]
        ids, dist = Matrix.zeros(rows, k), Matrix.zeros(rows, k)
        check(lib().imp_knn_topk(
            self._h, items._h, m._h, k, ctypes.c_void_p(ids.device_ptr), ctypes.c_void_p(dist.device_ptr),
            item_norms._h if item_norms is not None else None,
            query_filter._h if query_filter is not None else None,
            item_filter._h if item_filter is not None else None))
        return ids, dist

    def rank(self, items, query, offsets, candidates, n=0, liked=None):
        """NEW: scores the candidate list of every query row -- row r against items[candidates[offsets[r]:offsets[r + 1]]] --
        and, for n >= 1, ranks it (csrc/rank.hip).  offsets / candidates: host arrays (int64 / int32).  liked: a scipy CSR
        pattern with one row per query and sorted indices, or None; a candidate stored in its row scores -FLT_MAX.  n == 0:
        returns the scores, aligned with `candidates`; n >= 1: (ids, scores), rows x n, best first, padded with (-1, -FLT_MAX)."""
        if not isinstance(items, Matrix) or not isinstance(query, Matrix):
            raise TypeError("KnnQuery.rank expects implicit.gpu.Matrix arguments")
        n, rows = int(n), query.shape[0]
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        candidates = np.ascontiguousarray(candidates, dtype=np.int32)
        if offsets.shape != (rows + 1,) or candidates.ndim != 1 or len(candidates) != (offsets[-1] if rows else 0):
            raise ValueError("rank: offsets must hold one entry per query row plus one and end at len(candidates)")
        indptr = indices = None
        if liked is not None:
            if liked.shape[0] != rows:
                raise ValueError("rank: liked must contain 1 row for every query row")
            indptr = np.ascontiguousarray(liked.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(liked.indices, dtype=np.int32)
        ids = np.zeros((rows, n), dtype=np.int32) if n > 0 else None
        scores = np.zeros((rows, n) if n > 0 else len(candidates), dtype=np.float32)
        check(lib().imp_knn_rank(self._h, items._h, query._h, _vp(offsets), _vp(candidates), n,
                                 _vp(indptr) if liked is not None else None, _vp(indices) if liked is not None else None,
                                 _vp(ids) if n > 0 else None, _vp(scores)))
        return (ids, scores) if n > 0 else scores

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_knn_destroy(self._h)
            self._h = None


class Matrix:
    """_cuda.pyx:85-207.  Always truthy when constructed (the reference's cdef class defines no
    __len__/__bool__, and the model layer relies on `if self.item_factors`)."""

    def __init__(self, X):
        self._h = ctypes.c_void_p()
        self._keepalive = None
        if X is None:
            return
        cai = getattr(X, "__cuda_array_interface__", None)
        if cai:
            shape = cai["shape"]
            data = cai["data"][0]
            typestr = cai["typestr"]
            if typestr not in ("<f4", "<f2", "=f4", "=f2", "|f4", "|f2"):
                raise ValueError(f"unhandled dtype for GPU Matrix {typestr} (float32 / float16 only)")
            if len(shape) != 2:
                raise ValueError("Matrix expects a 2 dimensional array")
            itemsize = int(typestr[2])
            strides = cai.get("strides")
            if strides is not None and tuple(strides) != (shape[1] * itemsize, itemsize):
                raise ValueError("Matrix can only wrap C-contiguous device arrays")
            # the library works on its own non-blocking stream: order it after whatever the producer still has in
            # flight (the reference runs on the legacy default stream, which is implicitly ordered)
            synchronize()
            check(lib().imp_matrix_wrap_device(shape[0], shape[1], ctypes.c_void_p(data), itemsize,
                                               ctypes.byref(self._h)))
            self._keepalive = X  # no ownership of the memory: keep the exporter alive
            return
        if not hasattr(X, "dtype") or X.dtype.char not in ("f", "e"):
            raise ValueError(f"unhandled dtype for GPU Matrix {getattr(X, 'dtype', type(X))}")
        if X.ndim != 2:
            raise ValueError("Matrix expects a 2 dimensional array")
        X = np.ascontiguousarray(X)
        check(lib().imp_matrix_create(X.shape[0], X.shape[1], _vp(X), X.dtype.itemsize, ctypes.byref(self._h)))

    @classmethod
    def zeros(cls, rows, cols):
        ret = cls(None)
        check(lib().imp_matrix_create(rows, cols, None, 4, ctypes.byref(ret._h)))
        return ret

    def _dims(self):
        r, c, i = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().imp_matrix_shape(self._h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(i)))
        return r.value, c.value, i.value

    @property
    def shape(self):
        r, c, _ = self._dims()
        return r, c

    @property
    def itemsize(self):
        return self._dims()[2]

    @property
    def dtype(self):
        return np.dtype(np.float32) if self.itemsize == 4 else np.dtype(np.float16)

    @property
    def device_ptr(self):
        p = ctypes.c_void_p()
        check(lib().imp_matrix_device_ptr(self._h, ctypes.byref(p)))
        return p.value

    def __getitem__(self, idx):
        ret = Matrix(None)
        ret._keepalive = self._keepalive
        rows = self.shape[0]
        if isinstance(idx, slice):
            if idx.step and idx.step != 1:
                raise ValueError(f"Can't slice matrix with step {idx.step} yet")
            start = idx.start if idx.start is not None else 0
            stop = idx.stop if idx.stop is not None else rows
            if start < 0 or stop < 0:
                start, stop, _ = idx.indices(rows)
            check(lib().imp_matrix_slice(self._h, start, stop, ctypes.byref(ret._h)))
        elif isinstance(idx, int):
            if idx < 0:
                raise ValueError("row index out of bounds for matrix")
            check(lib().imp_matrix_row(self._h, idx, ctypes.byref(ret._h)))
        else:
            try:
                idx = np.array(idx).astype("int32")
            except Exception:
                raise IndexError(f"don't know how to handle __getitem__ on {idx}") from None
            if len(idx.shape) == 0:
                idx = idx.reshape([1])
            if len(idx.shape) != 1:
                raise IndexError(f"don't know how to handle __getitem__ on {idx} - shape={idx.shape}")
            if ((idx < 0) | (idx >= rows)).any():
                raise IndexError("row id out of range for selecting items from matrix")
            ids = IntVector(idx)
            check(lib().imp_matrix_gather(self._h, ids._h, ctypes.byref(ret._h)))
        return ret

    def assign_rows(self, rowids, other):
        rows = IntVector(np.array(rowids).astype("int32"))
        check(lib().imp_matrix_assign_rows(self._h, rows._h, other._h))

    def astype(self, dtype):
        dtype = np.dtype(dtype)
        allowed = (np.float16, np.float32)
        if dtype not in allowed:
            raise ValueError(f"Invalid dtype '{dtype}' for GPU model. Allowed dtypes are: {allowed}")
        ret = Matrix(None)
        check(lib().imp_matrix_astype(self._h, dtype.itemsize, ctypes.byref(ret._h)))
        return ret

    def resize(self, rows, cols):
        check(lib().imp_matrix_resize(self._h, int(rows), int(cols)))

    def to_numpy(self):
        r, c, itemsize = self._dims()
        if itemsize == 4:
            ret = np.zeros((r, c), dtype="float32")
        elif itemsize == 2:
            ret = np.zeros((r, c), dtype="float16")
        else:
            raise ValueError(f"Invalid itemsize {itemsize}")
        check(lib().imp_matrix_to_host(self._h, _vp(ret)))
        return ret

    def copy_from_numpy(self, X):
        """NEW: overwrite in place from a host array of identical shape/dtype (parity harness)."""
        X = np.ascontiguousarray(X)
        if X.shape != self.shape or X.dtype != self.dtype:
            raise ValueError("shape/dtype mismatch in Matrix.copy_from_numpy")
        check(lib().imp_matrix_from_host(self._h, _vp(X)))

    def copy_rows_from(self, dst_row, other, src_row, rows):
        """NEW: device-to-device copy of whole rows other[src_row : src_row + rows] -> self[dst_row : ...] on the library
        stream (the exchange between logical ranks sharing one device, local_comm.py)."""
        check(lib().imp_matrix_copy_rows(self._h, int(dst_row), other._h, int(src_row), int(rows)))

    def __repr__(self):
        return f"Matrix({str(self.to_numpy())})"

    def __str__(self):
        return str(self.to_numpy())

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_matrix_destroy(self._h)
            self._h = None


class IntVector:
    """_cuda.pyx:211-218"""

    def __init__(self, data):
        data = np.ascontiguousarray(data)
        if data.dtype != np.int32 or data.ndim != 1:
            raise ValueError("IntVector expects a 1-d int32 buffer")
        self._h = ctypes.c_void_p()
        self.size = len(data)
        check(lib().imp_intvector_create(_vp(data), len(data), ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_intvector_destroy(self._h)
            self._h = None


def _int32_buffer(a, what):
    a = np.asarray(a)
    if a.dtype != np.int32:
        # the reference binds `cdef int[:] indptr = X.indptr`: a non-int32 buffer is a ValueError
        raise ValueError(f"Buffer dtype mismatch, expected 'int' but got '{a.dtype}' for {what}")
    return np.ascontiguousarray(a)


class CSRMatrix:
    """_cuda.pyx:221-234"""

    def __init__(self, X):
        X = check_csr(X)
        data = np.ascontiguousarray(X.data.astype(np.float32, copy=False))
        self._h = ctypes.c_void_p()
        self.shape = X.shape
        self.nnz = len(data)
        if np.asarray(X.indptr).dtype == np.int64:
            # NEW: the reference binds int32 buffers only (a ValueError for int64); scipy switches both index arrays to
            # int64 once nnz >= 2^31, and the CPU solver accepts that (_als.pyx:76).  Column ids always fit int32.
            indptr = np.ascontiguousarray(X.indptr)
            indices = np.asarray(X.indices)
            if indices.dtype != np.int32:
                if len(indices) and (indices.max() > np.iinfo(np.int32).max or indices.min() < 0):
                    raise ValueError("column index out of range for CSRMatrix")
                indices = indices.astype(np.int32)
            indices = np.ascontiguousarray(indices)
            check(lib().imp_csr_create64(X.shape[0], X.shape[1], len(data), _vp(indptr), _vp(indices), _vp(data),
                                         ctypes.byref(self._h)))
            return
        indptr = _int32_buffer(X.indptr, "indptr")
        indices = _int32_buffer(X.indices, "indices")
        check(lib().imp_csr_create(X.shape[0], X.shape[1], len(data), _vp(indptr), _vp(indices), _vp(data),
                                   ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_csr_destroy(self._h)
            self._h = None


class COOMatrix:
    """_cuda.pyx:236-247"""

    def __init__(self, X):
        row = _int32_buffer(X.row, "row")
        col = _int32_buffer(X.col, "col")
        data = np.ascontiguousarray(X.data.astype(np.float32))
        self._h = ctypes.c_void_p()
        self.shape = X.shape
        check(lib().imp_coo_create(X.shape[0], X.shape[1], len(data), _vp(row), _vp(col), _vp(data),
                                   ctypes.byref(self._h)))

    @classmethod
    def from_csr_pattern(cls, X):
        """NEW: the (row, col) pattern of a scipy CSR matrix as a device COO without its values -- all the top-k filters read
        (knn.cu:197-214 reads row / col only).  Skips scipy's tocoo() and the value upload: recommend() builds one per batch."""
        self = cls.__new__(cls)
        indptr = np.ascontiguousarray(X.indptr)
        if indptr.dtype not in (np.int32, np.int64):
            indptr = indptr.astype(np.int64)
        col = np.ascontiguousarray(X.indices, dtype=np.int32)
        self._h = ctypes.c_void_p()
        self.shape = X.shape
        # indptr + indices go to page-locked staging and a kernel expands the row ids: no np.repeat, no blocking uploads
        check(lib().imp_coo_create_from_csr_pattern(X.shape[0], X.shape[1], _vp(indptr), int(indptr.dtype == np.int64), _vp(col),
                                                    ctypes.byref(self._h)))
        return self

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_coo_destroy(self._h)
            self._h = None


class LeastSquaresSolver:
    """_cuda.pyx:250-275"""

    def __init__(self):
        self._h = ctypes.c_void_p()
        check(lib().imp_solver_create(ctypes.byref(self._h)))

    def least_squares(self, cui, X, YtY, Y, cg_steps):
        check(lib().imp_solver_least_squares(self._h, cui._h, X._h, YtY._h, Y._h, int(cg_steps)))

    def least_squares_cholesky(self, cui, X, YtY, Y, regularization):
        """NEW: mirrors the CPU implicit.cpu._als._least_squares(YtY, ..., regularization): YtY is
        the UNregularised gramian; raises ValueError on a non-positive-definite row."""
        _check_failing(lib().imp_solver_least_squares_cholesky, self._h, cui._h, X._h, YtY._h, Y._h, float(regularization))

    def least_squares_subspace(self, cui, X, YtY, Y, regularization, block_size, sweeps=1):
        """NEW: the block-subspace half sweep of iALS++ for large factor counts: every row of X is improved, from its stored
        value, one block of `block_size` (1 .. 32) coordinates at a time by an exact Newton step in that block, `sweeps`
        times over.  YtY is the UNregularised gramian; float32 X and Y, at most 1024 factors.  block_size >= factors is the
        exact solve of least_squares_cholesky.  Raises ValueError (with .failed_row, -1 for an argument error) when a
        block's matrix is not positive definite; the other rows are solved."""
        _check_failing(lib().imp_solver_least_squares_subspace, self._h, cui._h, X._h, YtY._h, Y._h, float(regularization),
                       int(block_size), int(sweeps))

    def explain_factor(self, cui, YtY, Y, regularization, weights):
        """NEW: the Cholesky factor L of every row's A_u = YtY + regularization I + sum (|c| - 1) y y^T (YtY UNregularised, the
        matrix of least_squares_cholesky) into rows [u f, (u + 1) f) of `weights`, a float32 (cui.rows * f) x f Matrix: lower
        triangular, zeros above the diagonal.  f <= 256, Y float32.  ValueError (with .failed_row) on a non-positive pivot."""
        _check_failing(lib().imp_solver_explain_factor, self._h, cui._h, YtY._h, Y._h, float(regularization), weights._h)

    def explain(self, cui, Y, weights, itemids, items_per_row, n):
        """NEW: for row u of cui and each of its items_per_row ids in the IntVector `itemids` (row-major): the contributions
        c_j (w . y_j), w = A_u^-1 y_i from the row's factor in `weights`, of the liked items (c_j > 0).  Returns host arrays
        (total [pairs] float32, ids [pairs, n] int32, scores [pairs, n] float32): the n largest contributions under (score,
        id) descending, padded with (-1, -FLT_MAX).  Bad ids, n < 1 or a mis-shaped `weights` raise ValueError."""
        items_per_row, n = int(items_per_row), int(n)
        if not (1 <= n < 2**31 and 1 <= items_per_row < 2**31):
            raise ValueError("explain: n and items_per_row must be >= 1")
        pairs = cui.shape[0] * items_per_row
        total = np.empty(pairs, dtype=np.float32)
        ids = np.empty((pairs, n), dtype=np.int32)
        scores = np.empty((pairs, n), dtype=np.float32)
        check(lib().imp_solver_explain(self._h, cui._h, Y._h, weights._h, itemids._h, items_per_row, n, _vp(total), _vp(ids),
                                       _vp(scores)))
        return total, ids, scores

    def calculate_loss(self, cui, X, Y, regularization):
        loss = ctypes.c_float(0)
        check(lib().imp_solver_calculate_loss(self._h, cui._h, X._h, Y._h, float(regularization),
                                              ctypes.byref(loss)))
        return loss.value

    def calculate_yty(self, Y, YtY, regularization):
        check(lib().imp_solver_calculate_yty(self._h, Y._h, YtY._h, float(regularization)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_solver_destroy(self._h)
            self._h = None


def calculate_norms(items):
    """_cuda.pyx:278-281: returns a (1, rows) Matrix."""
    ret = Matrix(None)
    check(lib().imp_matrix_calculate_norms(items._h, ctypes.byref(ret._h)))
    return ret


def get_device_count():
    """_cuda.pyx:284-285: raises RuntimeError when no device is usable."""
    n = ctypes.c_int(0)
    check(lib().imp_get_device_count(ctypes.byref(n)))
    return n.value


def bpr_update(*args, **kwargs):
    """_cuda.pyx:288-297.  Kept raising NotImplementedError (pinned by the tests); BPR training is bpr_epoch."""
    raise NotImplementedError("bpr_update is not part of the MI355X ALS hot path")


def bpr_epoch(userids, itemids, indptr, X, Y, learning_rate, regularization, seed, verify_negative, samples=None):
    """One SGD pass of Bayesian Personalized Ranking (imp_bpr_update, bpr.hip): the first nine arguments are those of the
    reference's bpr_update (_cuda.pyx:288-297), returns (correct, skipped).  `samples`: the number of sampled triples, None
    for one epoch (nnz).  X / Y are updated in place.  Numerics are the reference's CPU update (cpu/bpr.pyx:249-302); the
    sample pairs are a Philox stream of (seed, sample index, nnz), so `skipped` is reproducible.  An id outside its matrix
    raises IndexError before anything is written.  Named apart from bpr_update, which keeps its NotImplementedError."""
    for name, v in (("userids", userids), ("itemids", itemids), ("indptr", indptr)):
        if not isinstance(v, IntVector):
            raise TypeError(f"bpr_epoch: {name} must be an implicit_amd.gpu.IntVector")
    if not isinstance(X, Matrix) or not isinstance(Y, Matrix):
        raise TypeError("bpr_epoch: X and Y must be implicit_amd.gpu.Matrix objects")
    correct, skipped = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().imp_bpr_update(userids._h, itemids._h, indptr._h, X._h, Y._h, float(learning_rate), float(regularization),
                               int(seed), 1 if verify_negative else 0, -1 if samples is None else int(samples),
                               ctypes.byref(correct), ctypes.byref(skipped)))
    return correct.value, skipped.value


def warp_epoch(userids, itemids, indptr, X, Y, learning_rate, regularization, seed, max_sampled=10, samples=None):
    """NEW: one SGD pass of WARP-loss matrix factorization (imp_warp_update, warp.hip), returns (satisfied, trials).  The
    arrays and matrices are those of bpr_epoch (row indices sorted); `samples`: the number of sampled positives, None for one
    epoch (nnz).  Every positive meets up to `max_sampled` (1 .. 4096) uniformly drawn items; the first that scores within
    1 of the positive ends the sample with a step weighted by the rank estimate; `satisfied` counts the samples that found
    none, `trials` the draws consumed.  X / Y are updated in place.  Positives and candidates are Philox streams of (seed,
    sample index).  Bad arguments raise ValueError, an id outside its matrix IndexError before anything is written."""
    for name, v in (("userids", userids), ("itemids", itemids), ("indptr", indptr)):
        if not isinstance(v, IntVector):
            raise TypeError(f"warp_epoch: {name} must be an implicit_amd.gpu.IntVector")
    if not isinstance(X, Matrix) or not isinstance(Y, Matrix):
        raise TypeError("warp_epoch: X and Y must be implicit_amd.gpu.Matrix objects")
    max_sampled = int(max_sampled)
    if not 1 <= max_sampled <= 4096:
        raise ValueError("warp_epoch: max_sampled must lie in 1 .. 4096")
    satisfied, trials = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().imp_warp_update(userids._h, itemids._h, indptr._h, X._h, Y._h, float(learning_rate), float(regularization),
                                int(seed), max_sampled, -1 if samples is None else int(samples),
                                ctypes.byref(satisfied), ctypes.byref(trials)))
    return satisfied.value, trials.value


def lmf_update(cui, X, Y, deriv_sum_sq, learning_rate, regularization, neg_prop, seed, one_col=-1):
    """One Adagrad half-sweep of Logistic Matrix Factorization (imp_lmf_update, lmf.hip): X is updated in place against
    the read-only Y over the CSRMatrix `cui` (rows of X x rows of Y, values = confidences), deriv_sum_sq (the shape of X)
    accumulates the squared gradients.  Numerics are the reference's CPU update (cpu/lmf.pyx lmf_update), with at most
    C = X.shape[1] negatives per row as there; the negatives are a Philox stream of (seed, row, k), so the result is
    deterministic.  Afterwards column `one_col` of X is 1.0 in every row (-1: none).  Bad shapes, dtypes or arguments
    raise ValueError with X and deriv_sum_sq untouched."""
    if not isinstance(cui, CSRMatrix):
        raise TypeError("lmf_update: cui must be an implicit_amd.gpu.CSRMatrix")
    for name, v in (("X", X), ("Y", Y), ("deriv_sum_sq", deriv_sum_sq)):
        if not isinstance(v, Matrix):
            raise TypeError(f"lmf_update: {name} must be an implicit_amd.gpu.Matrix")
    neg_prop, one_col = int(neg_prop), int(one_col)
    if not (0 <= neg_prop < 2**31 and -1 <= one_col < 2**31):
        raise ValueError("lmf_update: neg_prop must lie in [0, 2^31) and one_col in [-1, C)")
    check(lib().imp_lmf_update(cui._h, X._h, Y._h, deriv_sum_sq._h, float(learning_rate), float(regularization), neg_prop,
                               int(seed), one_col))


class SpMat:
    """NEW: an fp64-valued CSR on the device (imp_spmat), an operand of sparse_topk_product.  Any scipy sparse matrix is
    taken as CSR (converted without a warning); values become float64, offsets int64, column ids int32.  The stored order
    of every row's entries is kept: it is the summation order of the product."""

    def __init__(self, X):
        import scipy.sparse

        X = X if isinstance(X, scipy.sparse.csr_matrix) else scipy.sparse.csr_matrix(X)
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.asarray(X.indices)
        if indices.dtype != np.int32:
            if len(indices) and (indices.max() > np.iinfo(np.int32).max or indices.min() < 0):
                raise ValueError("column index out of range for SpMat")
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(X.data, dtype=np.float64)
        self.shape = (int(X.shape[0]), int(X.shape[1]))
        if max(self.shape) > np.iinfo(np.int32).max:
            raise ValueError("SpMat: dimensions must fit int32")
        self.nnz = len(data)
        self._h = ctypes.c_void_p()
        check(lib().imp_spmat_create(self.shape[0], self.shape[1], self.nnz, _vp(indptr), _vp(indices), _vp(data),
                                     ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_spmat_destroy(self._h)
            self._h = None


def sparse_topk_product(A, B, k, zero_own_columns=False):
    """NEW: row r of A.B over its touched columns, the k best under (score, id) descending (imp_sparse_topk_product,
    knn.hip).  A and B are SpMat handles; returns (ids int32, scores float64, counts int32) with ids / scores of shape
    (A.rows, k), counts[r] = min(k, touched columns of row r), entries past counts[r] = (-1, -inf).  zero_own_columns sets
    every touched column of A[r] to 0.0 (it stays a candidate).  Argument errors raise ValueError."""
    if not isinstance(A, SpMat) or not isinstance(B, SpMat):
        raise TypeError("sparse_topk_product: A and B must be implicit_amd.gpu.SpMat")
    k = int(k)
    if not 1 <= k < 2**31:
        raise ValueError("sparse_topk_product: k must be >= 1")
    rows = A.shape[0]
    ids = np.empty((rows, k), dtype=np.int32)
    scores = np.empty((rows, k), dtype=np.float64)
    counts = np.empty(rows, dtype=np.int32)
    check(lib().imp_sparse_topk_product(A._h, B._h, k, 1 if zero_own_columns else 0, _vp(ids), _vp(scores), _vp(counts)))
    return ids, scores, counts


def ease_gram(item_users, user_items, regularization, G=None):
    """NEW: G = X^T X + regularization I as a float32 items x items device Matrix (imp_ease_gram, ease.hip) from the two
    orientations of X as CSRMatrix handles: item_users (items x users) and user_items (users x items, duplicates summed).
    Every entry is the fp32 sum over the co-occurring users in item_users' stored order; G is exactly symmetric.  `G`: a
    Matrix to write into (default: a new one).  Shapes that do not agree raise ValueError."""
    if not isinstance(item_users, CSRMatrix) or not isinstance(user_items, CSRMatrix):
        raise TypeError("ease_gram: item_users and user_items must be implicit_amd.gpu.CSRMatrix")
    if G is None:
        G = Matrix.zeros(item_users.shape[0], item_users.shape[0])
    elif not isinstance(G, Matrix):
        raise TypeError("ease_gram: G must be an implicit_amd.gpu.Matrix")
    check(lib().imp_ease_gram(item_users._h, user_items._h, float(regularization), G._h))
    return G


def spd_inverse(A):
    """NEW: replaces the symmetric positive definite float32 Matrix A by its inverse (imp_spd_inverse, spd_inverse.hip: a
    blocked Cholesky inverse on the fp32 matrix cores).  Only the lower triangle is read; the result is exactly symmetric.
    A pivot that is not positive raises ValueError with .failed_pivot = the smallest failing index (A is then unspecified);
    a workspace that cannot be allocated raises RuntimeError naming the bytes."""
    if not isinstance(A, Matrix):
        raise TypeError("spd_inverse: A must be an implicit_amd.gpu.Matrix")
    _check_failing(lib().imp_spd_inverse, A._h, attr="failed_pivot")
    return A


def ease_weights(P):
    """NEW: in place B[i, j] = -(P[i, j] / P[j, j]), B[j, j] = 0 on a square float32 Matrix (imp_ease_weights): one IEEE
    division and a sign flip per entry.  A zero or non-finite diagonal entry raises ValueError with P untouched."""
    if not isinstance(P, Matrix):
        raise TypeError("ease_weights: P must be an implicit_amd.gpu.Matrix")
    check(lib().imp_ease_weights(P._h))
    return P


def ease_topk(knn, B, rows, k, filter_liked=False, item_filter=None):
    """NEW: the k best columns of x B for every row x of the scipy CSR matrix `rows` (imp_ease_topk, ease.hip).  B: a float32
    items x items Matrix; rows: one query per row, canonical (columns strictly increasing), values taken as float32.  A score
    is the fp32 sum of the row's products x_i B[i, j] in stored order.  filter_liked: the row's own columns score -FLT_MAX
    (they stay candidates); item_filter: an IntVector (or int32 array) of ids treated likewise.  Returns (ids int32, scores
    float32), rows x k, best first under (score, id) descending, padded with (-1, -FLT_MAX) past min(k, items).  k outside
    1 .. 1024, columns outside the model or not increasing raise ValueError."""
    if not isinstance(knn, KnnQuery) or not isinstance(B, Matrix):
        raise TypeError("ease_topk expects a KnnQuery and an implicit_amd.gpu.Matrix")
    k = int(k)
    n = int(rows.shape[0])
    indptr = np.ascontiguousarray(rows.indptr, dtype=np.int64)
    indices = np.asarray(rows.indices)
    if indices.dtype != np.int32 and len(indices) and (indices.max() > np.iinfo(np.int32).max or indices.min() < 0):
        raise ValueError("ease_topk: column index out of range")
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(rows.data, dtype=np.float32)
    if item_filter is not None and not isinstance(item_filter, IntVector):
        item_filter = IntVector(np.ascontiguousarray(item_filter, dtype=np.int32))
    ids = np.empty((n, max(k, 0)), dtype=np.int32)
    scores = np.empty((n, max(k, 0)), dtype=np.float32)
    check(lib().imp_ease_topk(knn._h, B._h, n, _vp(indptr), _vp(indices), _vp(data), k, 1 if filter_liked else 0,
                              item_filter._h if item_filter is not None else None, _vp(ids), _vp(scores)))
    return ids, scores


SLIM_MAX_ITEMS = 40000  # IMP_SLIM_MAX_ITEMS: a column's running product has to fit one workgroup's LDS


def slim_workspace_bytes(items):
    """Device bytes imp_slim_solve reserves besides A and W: the diagonal, the column order, the sweep counts, eight words."""
    return 4 * (3 * int(items) + 8)


def slim_solve(A, l1, positive=True, max_sweeps=100, tol=1e-4, W=None):
    """NEW: the SLIM weights of a Gram matrix (imp_slim_solve, slim.hip).  A: the float32 items x items Matrix ease_gram returns
    for regularization = l2.  Column j of the result minimises 1/2 w^T A w - sum_i A[j, i] w_i + l1 sum_i |w_i| subject to
    w_j = 0 (and w >= 0 when `positive`) by cyclic coordinate descent, at most `max_sweeps` sweeps, stopped when the largest
    change of a sweep is <= tol times the largest weight; defined operation for operation in fp32 (include/implicit_hip.h;
    tests/slim_reference.py restates it in numpy).  Returns (W, sweeps): W a float32 items x items Matrix in the layout of
    EASE's B (W[i, j] = weight of source i for target j, zero diagonal; `W`: a Matrix to write into, default a new one), sweeps
    an int32 array of the sweeps each column ran.  At most 40 000 items.  Arguments the library refuses raise ValueError with
    W untouched; a diagonal entry of A that is not finite or not > 0 names the smallest such item."""
    if not isinstance(A, Matrix):
        raise TypeError("slim_solve: A must be an implicit_amd.gpu.Matrix")
    if W is None:
        if A.shape[0] > SLIM_MAX_ITEMS:
            raise ValueError(f"slim_solve: {A.shape[0]} items, at most {SLIM_MAX_ITEMS} are supported")
        W = Matrix.zeros(A.shape[0], A.shape[0])
    elif not isinstance(W, Matrix):
        raise TypeError("slim_solve: W must be an implicit_amd.gpu.Matrix")
    sweeps = np.zeros(A.shape[0], dtype=np.int32)
    check(lib().imp_slim_solve(A._h, float(l1), 1 if positive else 0, int(max_sweeps), float(tol), W._h, _vp(sweeps)))
    return W, sweeps


def slim_stats():
    """Measurement aid (imp_slim_stats): (updates applied by the last slim_solve on this device, the longest time one column held
    its workgroup in seconds)."""
    updates, longest = ctypes.c_ulonglong(0), ctypes.c_double(0.0)
    check(lib().imp_slim_stats(ctypes.byref(updates), ctypes.byref(longest)))
    return int(updates.value), float(longest.value)


def spmm(csr, dense, out=None):
    """NEW: out = csr @ dense as a float32 device Matrix (imp_csr_spmm, svd.hip).  csr: a CSRMatrix (rows x cols); dense: a
    float32 Matrix (cols x l), 1 <= l <= 1024.  Every entry is the fp32 sum of the row's products in stored order, rows of more
    than 1024 entries in runs of 1024 that are added in order: defined bit for bit (tests/svd_reference.py restates it in
    numpy).  `out`: a rows x l Matrix to write into (default: a new one); it must not overlap `dense`.  Shapes or dtypes that do
    not agree raise ValueError with `out` untouched."""
    if not isinstance(csr, CSRMatrix) or not isinstance(dense, Matrix):
        raise TypeError("spmm expects an implicit_amd.gpu.CSRMatrix and an implicit_amd.gpu.Matrix")
    if out is None:
        out = Matrix.zeros(csr.shape[0], dense.shape[1])
    elif not isinstance(out, Matrix):
        raise TypeError("spmm: out must be an implicit_amd.gpu.Matrix")
    check(lib().imp_csr_spmm(csr._h, dense._h, out._h))
    return out


def multiply_small(Y, W, out=None):
    """NEW: out = Y @ W for a tall float32 Matrix Y (rows x l) and a small one W (l x m), 1 <= l, m <= 1024
    (imp_matrix_multiply_small, svd.hip): exact fp32 products on the matrix cores in a fixed order, |out - exact| <=
    (l + 1) 2^-24 sum |y w| per entry.  `out`: a rows x m Matrix to write into (default: a new one); it must not overlap Y
    or W.  Shapes or dtypes that do not agree raise ValueError with `out` untouched."""
    if not isinstance(Y, Matrix) or not isinstance(W, Matrix):
        raise TypeError("multiply_small expects two implicit_amd.gpu.Matrix operands")
    if out is None:
        out = Matrix.zeros(Y.shape[0], W.shape[1])
    elif not isinstance(out, Matrix):
        raise TypeError("multiply_small: out must be an implicit_amd.gpu.Matrix")
    check(lib().imp_matrix_multiply_small(Y._h, W._h, out._h))
    return out


def mem_get_info():
    """(free, total) device memory in bytes (imp_mem_get_info)."""
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib().imp_mem_get_info(ctypes.byref(free), ctypes.byref(total)))
    return free.value, total.value


def _eval_pattern(test_user_items, k):
    """The arguments imp_eval_create and imp_host_ranking_metrics share: the held-out CSR pattern (rows strictly increasing:
    sorted, duplicates merged) and the two discount tables of length k (evaluation.pyx:408-409)."""
    k = int(k)
    if not 1 <= k < 2**31:
        raise ValueError("ranking metrics: K must be >= 1")
    rows, cols = (int(d) for d in test_user_items.shape)
    if max(rows, cols) > np.iinfo(np.int32).max:
        raise ValueError("ranking metrics: dimensions must fit int32")
    indptr = np.ascontiguousarray(test_user_items.indptr)
    if indptr.dtype not in (np.int32, np.int64):
        indptr = indptr.astype(np.int64)
    indices = np.asarray(test_user_items.indices)
    if indices.dtype != np.int32:
        if len(indices) and (indices.max() > np.iinfo(np.int32).max or indices.min() < 0):
            raise ValueError("ranking metrics: column index out of range")
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    cg = 1.0 / np.log2(np.arange(2, k + 2))
    cg_sum = np.cumsum(cg)
    return rows, cols, indptr, int(indptr.dtype == np.int64), indices, k, cg, cg_sum


_SUM_NAMES = ("relevant", "pr_div", "sum_ap", "sum_ndcg", "sum_auc", "total")


class RankingMetrics:
    """NEW: running sums of P@K / MAP@K / NDCG@K / AUC@K over recommendation rows that stay on the device (imp_eval,
    csrc/evaluation.hip; the reference computes them in a host loop, evaluation.pyx:437-466).  `test_user_items`: the
    held-out scipy CSR matrix in canonical form (sorted rows, no duplicates; ValueError otherwise); only its pattern is
    read, every stored entry is a like."""

    def __init__(self, test_user_items, K):
        rows, cols, indptr, is64, indices, k, cg, cg_sum = _eval_pattern(test_user_items, K)
        self.K, self.shape = k, (rows, cols)
        self._h = ctypes.c_void_p()
        check(lib().imp_eval_create(rows, cols, _vp(indptr), is64, _vp(indices), k, _vp(cg), _vp(cg_sum), ctypes.byref(self._h)))

    def add(self, ids, userids, per_row=False):
        """ids: the n x K device Matrix KnnQuery.topk_device returns (int32 bit patterns), or a host int32 array (uploaded);
        userids: the n rows of the test matrix they belong to (IntVector or int32 array).  Users with nothing held out, or
        outside the matrix, add nothing.  Only queues work, unless per_row is set: then returns an n x 4 float64 array of
        each row's (hits, ap, ndcg, auc) terms."""
        if not isinstance(ids, Matrix):
            ids = np.ascontiguousarray(ids)
            if ids.dtype != np.int32 or ids.ndim != 2:
                raise ValueError("RankingMetrics.add expects a 2-d int32 array of ids")
            ids = Matrix(ids.view(np.float32))  # the bits travel untouched
        if not isinstance(userids, IntVector):
            userids = IntVector(np.ascontiguousarray(userids, dtype=np.int32))
        out = np.empty((userids.size, 4), dtype=np.float64) if per_row else None
        check(lib().imp_eval_add(self._h, ids._h, userids._h, _vp(out) if per_row else None))
        return out

    def sums(self):
        """Waits for the queued work; {relevant, pr_div, sum_ap, sum_ndcg, sum_auc, total} as floats."""
        out = np.zeros(6, dtype=np.float64)
        check(lib().imp_eval_result(self._h, _vp(out)))
        return dict(zip(_SUM_NAMES, out.tolist()))

    def reset(self):
        check(lib().imp_eval_reset(self._h))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_eval_destroy(self._h)
            self._h = None


def host_ranking_metrics(test_user_items, K, ids, userids, per_row=False):
    """NEW: the sums of RankingMetrics for host ids (n x K int32) in plain host code (imp_host_ranking_metrics; no device
    involved).  Returns the dict of six sums, and with per_row also the n x 4 array of (hits, ap, ndcg, auc) terms.  A
    non-canonical test matrix raises ValueError, a user id outside it IndexError."""
    rows, cols, indptr, is64, indices, k, cg, cg_sum = _eval_pattern(test_user_items, K)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    userids = np.ascontiguousarray(userids, dtype=np.int32)
    if ids.ndim != 2 or ids.shape != (len(userids), k):
        raise ValueError("host_ranking_metrics: ids must have one row of K ids per user id")
    sums = np.zeros(6, dtype=np.float64)
    out = np.empty((len(userids), 4), dtype=np.float64) if per_row else None
    check(lib().imp_host_ranking_metrics(rows, cols, _vp(indptr), is64, _vp(indices), k, _vp(cg), _vp(cg_sum), _vp(ids),
                                         _vp(userids), len(userids), _vp(sums), _vp(out) if per_row else None))
    sums = dict(zip(_SUM_NAMES, sums.tolist()))
    return (sums, out) if per_row else sums


class IVFIndex:
    """NEW: a native IVF-Flat index over the rows of a factor matrix (imp_ivf, csrc/ivf.hip) -- what the reference builds
    with faiss.GpuIndexIVFFlat (implicit/ann/faiss.py).  Build it with IVFIndex.build; search returns, per query, the k best
    vectors among the `nprobe` lists whose centroids are nearest by inner product."""

    def __init__(self):
        self._h = ctypes.c_void_p()

    @classmethod
    def build(cls, vectors, nlist, iterations=10, init_rows=None, random_state=None, max_temp_memory=0):
        """vectors: a Matrix or a float32 / float16 array (rows x factors, 1 .. 1024 factors; the index stores fp32).
        init_rows: the `nlist` distinct rows the centroids start from; by default drawn without replacement from
        numpy.random.default_rng(random_state).  iterations: rounds of spherical k-means.  max_temp_memory: bytes of
        temporaries of one chunk of queries, 0 = min(free / 2, 4 GiB) as KnnQuery.  Deterministic for equal arguments."""
        if not isinstance(vectors, Matrix):
            vectors = Matrix(vectors)
        nlist = int(nlist)
        rows = vectors.shape[0]
        if not 1 <= nlist <= rows:
            raise ValueError("IVFIndex.build: nlist must lie in 1 .. rows")
        if init_rows is None:
            init_rows = np.random.default_rng(random_state).choice(rows, size=nlist, replace=False)
        init_rows = np.ascontiguousarray(init_rows, dtype=np.int32)
        if init_rows.shape != (nlist,):
            raise ValueError("IVFIndex.build: init_rows must hold nlist row ids")
        self = cls()
        check(lib().imp_ivf_build(vectors._h, nlist, int(iterations), _vp(init_rows), ctypes.byref(self._h)))
        if max_temp_memory:
            check(lib().imp_ivf_set_temp_memory(self._h, int(max_temp_memory)))
        return self

    def set_temp_memory(self, max_temp_memory=0):
        check(lib().imp_ivf_set_temp_memory(self._h, int(max_temp_memory)))

    def _shape(self):
        r, c, n = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
        check(lib().imp_ivf_shape(self._h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(n)))
        return r.value, c.value, n.value

    @property
    def shape(self):
        return self._shape()[:2]

    @property
    def nlist(self):
        return self._shape()[2]

    @property
    def centroids(self):
        """nlist x factors float32: unit rows, or zero rows."""
        _, c, n = self._shape()
        out = np.empty((n, c), dtype=np.float32)
        check(lib().imp_ivf_lists(self._h, _vp(out), None, None))
        return out

    @property
    def list_offsets(self):
        out = np.empty(self.nlist + 1, dtype=np.int64)
        check(lib().imp_ivf_lists(self._h, None, _vp(out), None))
        return out

    @property
    def list_ids(self):
        """The row ids list by list: list l is list_ids[list_offsets[l]:list_offsets[l + 1]], ascending."""
        out = np.empty(self.shape[0], dtype=np.int32)
        check(lib().imp_ivf_lists(self._h, None, None, _vp(out)))
        return out

    def search(self, queries, k, nprobe, return_probes=False):
        """(ids int32, scores float32), each queries x k, best first under (score desc, id desc); where the probed lists hold
        fewer than k vectors the tail is (-1, -FLT_MAX).  nprobe above nlist is nlist.  return_probes adds the
        queries x min(nprobe, nlist) probed list ids.  k outside 1 .. 1024 or nprobe < 1 raise ValueError.  So does
        min(nprobe, nlist) > 1024: a search probes at most 1024 lists, and an index of more lists refuses a larger nprobe
        instead of clamping it, whatever the number of queries (zero included); the refusal touches neither the index nor
        its temporaries.  Zero queries give two (0, k) arrays."""
        if not isinstance(queries, Matrix):
            queries = Matrix(queries)
        k, nprobe = int(k), int(nprobe)
        if k < 1 or nprobe < 1:
            raise ValueError("IVFIndex.search: k and nprobe must be >= 1")
        rows = queries.shape[0]
        ids = np.empty((rows, k), dtype=np.int32)
        dist = np.empty((rows, k), dtype=np.float32)
        probes = np.empty((rows, min(nprobe, self.nlist)), dtype=np.int32) if return_probes else None
        check(lib().imp_ivf_search(self._h, queries._h, k, min(nprobe, 2**31 - 1), _vp(ids), _vp(dist),
                                   _vp(probes) if return_probes else None))
        return (ids, dist, probes) if return_probes else (ids, dist)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_ivf_destroy(self._h)
            self._h = None


class Comm:
    """NEW: RCCL communicator, one process per GPU (include/implicit_hip.h, imp_comm_*)."""

    UNIQUE_ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(Comm.UNIQUE_ID_BYTES)
        check(lib().imp_comm_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id, nranks, rank):
        self._h = ctypes.c_void_p()
        self.nranks, self.rank = int(nranks), int(rank)
        buf = ctypes.create_string_buffer(bytes(unique_id), Comm.UNIQUE_ID_BYTES)
        check(lib().imp_comm_init_rank(buf, self.nranks, self.rank, ctypes.byref(self._h)))

    def allreduce_sum(self, m):
        check(lib().imp_comm_allreduce_sum(self._h, m._h))

    def allgather_rows(self, full, row_offsets):
        offs = (ctypes.c_int64 * (self.nranks + 1))(*[int(o) for o in row_offsets])
        check(lib().imp_comm_allgather_rows(self._h, full._h, offs))

    def allgather_rows_begin(self, full, row_lo, row_hi):
        """Queue the exchange of rows [row_lo[r], row_hi[r]) (owner: rank r) behind the work queued so far; returns
        immediately.  Pair with allgather_rows_end()."""
        lo = (ctypes.c_int64 * self.nranks)(*[int(o) for o in row_lo])
        hi = (ctypes.c_int64 * self.nranks)(*[int(o) for o in row_hi])
        check(lib().imp_comm_allgather_rows_begin(self._h, full._h, lo, hi))

    def allgather_rows_end(self):
        check(lib().imp_comm_allgather_rows_end(self._h))

    def alltoall_rows(self, send, send_lo, send_hi, recv, recv_lo, recv_hi):
        """Rows [send_lo[p], send_hi[p]) of `send` go to rank p and land in rows [recv_lo[q], recv_hi[q]) of its `recv`
        (q = the sender).  Blocking; bytes travel untouched."""
        arr = lambda v: (ctypes.c_int64 * self.nranks)(*[int(o) for o in v])  # noqa: E731
        check(lib().imp_comm_alltoall_rows(self._h, send._h, arr(send_lo), arr(send_hi), recv._h, arr(recv_lo), arr(recv_hi)))

    def barrier(self):
        check(lib().imp_comm_barrier(self._h))

    def ranks_seen(self):
        """(ranks counted on the library stream's communicator, ranks counted on the exchange stream's): both must equal
        `nranks`, else the rendezvous wired fewer processes together than were launched."""
        out = (ctypes.c_int * 2)(0, 0)
        check(lib().imp_comm_ranks_seen(self._h, out))
        return int(out[0]), int(out[1])

    def __del__(self):
        if getattr(self, "_h", None):
            lib().imp_comm_destroy(self._h)
            self._h = None


def set_device(device):
    check(lib().imp_set_device(int(device)))


def get_device():
    d = ctypes.c_int(0)
    check(lib().imp_get_device(ctypes.byref(d)))
    return d.value


def set_oversubscribe(factor):
    """Workgroups launched per resident slot by the persistent row kernels (1 = exactly what the device holds; the
    multi-GPU driver uses 4 so that slots held by RCCL's kernels only delay small shares)."""
    check(lib().imp_set_oversubscribe(int(factor)))


def get_oversubscribe():
    n = ctypes.c_int(0)
    check(lib().imp_get_oversubscribe(ctypes.byref(n)))
    return n.value


def set_deferred_sync(on):
    """Deferred mode of the current device: calculate_yty / least_squares / Comm.allreduce_sum only queue their work; one
    synchronize() orders (and checks) everything queued.  set_deferred_sync(False) waits and restores the default."""
    check(lib().imp_set_deferred_sync(1 if on else 0))


def release_workspaces():
    """Free the library's per-device scratch buffers (they are re-allocated on demand); fit() calls it when it returns."""
    check(lib().imp_release_workspaces())


def debug_occupy(workgroups, microseconds):
    """Measurement aid: park `workgroups` spinning workgroups on the device for about `microseconds`."""
    check(lib().imp_debug_occupy(int(workgroups), int(microseconds)))


def core_clock_mhz(microseconds=50):
    """Measurement aid: the shader core clock (MHz) seen by a probe kernel queued behind the work already on the stream;
    microseconds < 0: by a probe running BESIDE the work queued in deferred mode (the clock those kernels run at)."""
    mhz = ctypes.c_double(0.0)
    check(lib().imp_debug_core_clock(int(microseconds), ctypes.byref(mhz)))
    return mhz.value


def synchronize():
    check(lib().imp_device_synchronize())


def fixup_rows(reset=True):
    """Rows of CG sweeps on the current device that a fast kernel handed to the fp32 fix-up kernel since the last reset (a lost
    cluster exchange, or long rows whose matrix-core operands left the fp16 range): results are correct either way, a non-zero
    count is a performance signal."""
    n = ctypes.c_ulonglong(0)
    check(lib().imp_solver_fixup_rows(ctypes.byref(n), 1 if reset else 0))
    return int(n.value)


class Profiler:
    """Per-kernel HIP-event timing on the library stream (imp_prof_*), for bench.py's roofline leg."""

    @staticmethod
    def enable(on=True, only=None):
        """`only`: time just the kernels whose name contains this substring (an event pair costs stream time)."""
        check(lib().imp_prof_filter((only or "").encode()))
        check(lib().imp_prof_enable(1 if on else 0))

    @staticmethod
    def reset():
        check(lib().imp_prof_reset())

    @staticmethod
    def get(kernel):
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        check(lib().imp_prof_get(kernel.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    @staticmethod
    def names():
        buf = ctypes.create_string_buffer(4096)
        check(lib().imp_prof_names(buf, 4096))
        return [s for s in buf.value.decode().split("\n") if s]
