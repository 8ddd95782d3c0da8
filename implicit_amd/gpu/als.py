"""AlternatingLeastSquares on MI355X.

Public surface of implicit/gpu/als.py:14-341 (fit / recalculate_user / recalculate_item /
partial_fit_users / partial_fit_items / YtY / XtX / save / load / pickle, fit_callback), plus the CPU
class's explain (cpu/als.py:351-416) and a batched explain_batch, with the
numerics of the reference's *CPU* path, which is the parity oracle (implicit/cpu/als.py:98-202):

  * `alpha` scales the confidence matrix inside fit (cpu/als.py:133-134; the reference GPU fit
    silently ignores alpha -- SURVEY 3.2);
  * factors start as rng.random((n, f), float32) * 0.01, users first then items, from
    numpy.random.default_rng(random_state) (cpu/als.py:144-147) unless `init="device"` asks for the
    reference-GPU style U(-0.5/f, 0.5/f) drawn on the device (gpu/als.py:129-139);
  * `use_cg=False` selects the Cholesky solver (cpu/als.py:418-423), which the reference GPU path
    does not have; recalculate_user/item use Cholesky as the CPU path does (cpu/als.py:221-241)
    (any factors <= 1024; the reference GPU path runs CG to `factors` steps there, gpu/als.py:188-195);
  * `block_size=k` (1 .. 32, with `subspace_sweeps`) replaces the CG half sweep of fit() by the block-subspace solver of
    iALS++ (csrc/als_subspace.hip; no reference counterpart): meant for factors >= 256, float32 factors, one GPU,
    use_cg=True; block_size=None is the CG / Cholesky path, bit for bit;
  * NaN factors after fit raise ModelFitError (cpu/als.py:202).

Multi-GPU: `AlternatingLeastSquares(..., comm=implicit_amd.gpu.Comm(...))`, one process per GPU, every rank calling
fit() with ITS contiguous block of user rows (blocks in rank order; implicit_amd/gpu/sharded.py: the item-side shard is
exchanged at set-up, RCCL all-reduce of the gramian and all-gather of the solved factor rows per half sweep; all ranks
end with identical full factors).  `rendezvous.init_comm(gpu)` builds the
communicator from the launcher's RANK / WORLD_SIZE / MASTER_* environment.  No reference counterpart
(implicit/gpu/als.cu:169 "TODO: multi-gpu support").
"""
import logging
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import implicit_amd.gpu as gpu

from ..utils import check_csr, check_random_state, random_factors, transpose_csr
from .matrix_factorization_base import MatrixFactorizationBase

log = logging.getLogger("implicit_amd")

_CHOLESKY_MAX_FACTORS = 1024  # what the library's Cholesky takes (beyond 256: the triangle in a device workspace)
_EXPLAIN_MAX_FACTORS = 256     # explain / explain_batch: the triangle stays in the LDS (csrc/explain.hip)


class AlternatingLeastSquares(MatrixFactorizationBase):
    def __init__(self, factors=64, regularization=0.01, alpha=1.0, dtype=np.float32, iterations=15,
                 calculate_training_loss=False, random_state=None, use_cg=True, cg_steps=3, init="numpy", comm=None,
                 block_size=None, subspace_sweeps=1):
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        if block_size is not None:
            # the block-subspace solver of iALS++ takes the place of the CG half sweep in fit()
            if not 1 <= int(block_size) <= 32:
                raise ValueError("block_size must be between 1 and 32")
            if int(subspace_sweeps) < 1:
                raise ValueError("subspace_sweeps must be >= 1")
            if not use_cg:
                raise ValueError("block_size replaces the CG half sweep: it cannot be combined with use_cg=False")
            if np.dtype(dtype) != np.float32:
                raise ValueError("the block-subspace solver (block_size) keeps float32 factors")
            if comm is not None and comm.nranks > 1:
                raise ValueError("the block-subspace solver (block_size) runs on one GPU: no multi-rank comm")
            block_size, subspace_sweeps = int(block_size), int(subspace_sweeps)
        super().__init__()
        self.factors = factors
        self.regularization = regularization
        self.alpha = alpha
        self.dtype = np.dtype(dtype)
        self.iterations = iterations
        self.calculate_training_loss = calculate_training_loss
        self.random_state = random_state
        self.use_cg = use_cg
        self.cg_steps = cg_steps
        self.init = init
        self.comm = comm
        self.block_size = block_size
        self.subspace_sweeps = subspace_sweeps
        self.fit_callback = None
        self._solver = None
        self._YtY = self._XtX = None      # regularised gramians (the reference's cached properties)
        self._YtY0 = self._XtX0 = None    # unregularised ones, for the Cholesky fold-in

    # ---- training ----------------------------------------------------------------------------------
    def _initial_factors(self, users, items):
        if self.init == "device":
            from .matrix_factorization_base import check_random_state as device_rs

            rs = device_rs(self.random_state)
            lo, hi = -0.5 / self.factors, 0.5 / self.factors
            if self.user_factors is None:
                self.user_factors = rs.uniform(users, self.factors, low=lo, high=hi).astype(self.dtype)
            if self.item_factors is None:
                self.item_factors = rs.uniform(items, self.factors, low=lo, high=hi).astype(self.dtype)
            return
        rng = check_random_state(self.random_state)
        if self.user_factors is None:
            x0 = random_factors(rng, users, self.factors)
            self.user_factors = gpu.Matrix(x0.astype(self.dtype, copy=False))
        if self.item_factors is None:
            y0 = random_factors(rng, items, self.factors)
            self.item_factors = gpu.Matrix(y0.astype(self.dtype, copy=False))

    def fit(self, user_items, show_progress=True, callback=None):
        Cui = check_csr(user_items)
        if Cui.dtype != np.float32:
            Cui = Cui.astype(np.float32)
        if self.alpha != 1.0:
            Cui = self.alpha * Cui
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None
        self._YtY = self._XtX = self._YtY0 = self._XtX0 = None
        if self.comm is not None and self.comm.nranks > 1:
            return self._fit_sharded(Cui, callback)  # `user_items` = THIS RANK's block of user rows

        # set-up: the transpose (threaded counting transpose in the library, host only, no device lock; scipy for
        # non-canonical input) runs on a worker thread while this one uploads the user-side matrix with its row schedule
        # and draws / uploads the initial factors; ctypes and numpy drop the GIL in all of them
        t0 = time.time()
        users, items = Cui.shape
        with ThreadPoolExecutor(max_workers=1) as worker:
            transposed = worker.submit(transpose_csr, Cui)
            Cui_dev = gpu.CSRMatrix(Cui)
            self._initial_factors(users, items)
            Ciu = transposed.result()
        log.debug("Transpose, user-side upload and initial factors in %.3fs", time.time() - t0)
        Ciu_dev = gpu.CSRMatrix(Ciu)
        X, Y = self.user_factors, self.item_factors
        gram = gpu.Matrix.zeros(self.factors, self.factors)
        loss = None
        progress = _progress(self.iterations, show_progress)
        # the four solver calls of an iteration are queued back to back (deferred mode) and waited for once: no host round
        # trip between a gramian and the sweep that uses it (-1 % per iteration at configs[2]; errors surface at that wait)
        gpu.set_deferred_sync(True)
        fixups_before = gpu.fixup_rows(reset=False)
        try:
            for iteration in range(self.iterations):
                t0 = time.time()
                self._half_sweep(Cui_dev, X, Y, gram)
                self._half_sweep(Ciu_dev, Y, X, gram)
                gpu.synchronize()
                if self.calculate_training_loss:
                    loss = self.solver.calculate_loss(Cui_dev, X, Y, self.regularization)
                    if not show_progress:
                        log.info("loss %.4f", loss)
                progress.update(loss)
                cb = callback or self.fit_callback
                if cb:
                    cb(iteration, time.time() - t0, loss)
        finally:
            gpu.set_deferred_sync(False)
            if self.factors not in (64, 128, 256):
                gpu.release_workspaces()  # the zero-padded factor copies: rows x F floats per side, not worth keeping
        progress.close()
        # rows > 512 nonzeros run fp16-split operands on the matrix cores; an operand that leaves the fp16 range (very large
        # confidences x alpha on un-normalised factors) sends its row to the one-wavefront fp32 kernel instead: correct, and
        # ~1 ms per 4096-nonzero row -- a slowdown nobody would otherwise see
        refits = gpu.fixup_rows(reset=False) - fixups_before
        if refits > max(64, 0.001 * (users + items) * self.iterations):
            log.warning("%d long-row solves of this fit were re-done by the fp32 fix-up kernel (operands beyond the fp16 range of "
                        "the matrix-core path): scale the confidences (alpha) or the factors down, or expect slow iterations", refits)
        if self.calculate_training_loss:
            log.info("Final training loss %s", loss)
        self._check_fit_errors()

    def _fit_sharded(self, Cui_rows, callback):
        """Multi-GPU fit: `Cui_rows` is this rank's contiguous block of user rows (all item columns, blocks in rank
        order; `sharded.take_rank_rows(full, comm)` cuts one out of a full matrix).  Nothing of full-matrix size is
        built on any rank: the item-side shard comes from a transpose of the block plus one personalised exchange."""
        from . import sharded

        if not self.use_cg:
            raise ValueError("the multi-GPU fit runs the CG solver (use_cg=True)")
        if self.dtype != np.float32:
            raise ValueError("the multi-GPU fit keeps float32 factor replicas")
        backend = sharded.GpuBackend(gpu, solver=self.solver, nranks=self.comm.nranks)
        try:  # whatever fails below, the device gets its launch shape and synchronous calls back (backend.close)
            sizes = np.zeros(self.comm.nranks, dtype=np.int64)
            sizes[self.comm.rank] = Cui_rows.shape[0]
            users = int(sharded.allreduce_ints(self.comm, backend, sizes).sum())
            self._initial_factors(users, Cui_rows.shape[1])
            # every rank must start from the same factors whatever its random_state: rank 0's win (the others contribute
            # zeros to a sum all-reduce)
            for m in (self.user_factors, self.item_factors):
                if self.comm.rank != 0:
                    m.copy_from_numpy(np.zeros(m.shape, dtype=np.float32))
                self.comm.allreduce_sum(m)
            u_off, _ = sharded.fit_sharded(self, Cui_rows, self.comm, callback or self.fit_callback, backend=backend,
                                           csr=gpu.CSRMatrix, users=users)
        finally:
            backend.close()
            if self.factors not in (64, 128, 256):
                gpu.release_workspaces()
        if self.calculate_training_loss:
            # the objective restricted to this rank's user rows (each rank logs its own; there is no global reduction)
            r = self.comm.rank
            loss = self.solver.calculate_loss(gpu.CSRMatrix(Cui_rows), self.user_factors[int(u_off[r]):int(u_off[r + 1])],
                                              self.item_factors, self.regularization)
            log.info("Final training loss over rank %d's user rows %s", r, loss)
        self._check_fit_errors()

    def _half_sweep(self, C, X, Y, gram):
        """One half iteration: X <- argmin given Y (gramian + per-row solves)."""
        if getattr(self, "block_size", None) is not None:
            self.solver.calculate_yty(Y, gram, 0.0)
            self.solver.least_squares_subspace(C, X, gram, Y, self.regularization, self.block_size, self.subspace_sweeps)
        elif self.use_cg:
            self.solver.calculate_yty(Y, gram, self.regularization)
            self.solver.least_squares(C, X, gram, Y, self.cg_steps)
        else:
            self.solver.calculate_yty(Y, gram, 0.0)
            self.solver.least_squares_cholesky(C, X, gram, Y, self.regularization)

    # ---- fold-in -----------------------------------------------------------------------------------
    def _recalculate(self, ids, rows_csr, other_factors, gram_reg_fn, gram_unreg_fn):
        rows_csr = check_csr(rows_csr)
        count = 1 if np.isscalar(ids) else len(ids)
        if rows_csr.shape[0] != count:
            raise ValueError("expected one sparse row for every id to recalculate")
        if self.alpha != 1.0:
            rows_csr = self.alpha * rows_csr
        out = gpu.Matrix.zeros(count, self.factors).astype(self.dtype)
        C = gpu.CSRMatrix(rows_csr.astype(np.float32))
        # only the gramian the chosen solver needs is evaluated, and both are cached until the factors change
        if self.factors <= _CHOLESKY_MAX_FACTORS:
            self.solver.least_squares_cholesky(C, out, gram_unreg_fn(), other_factors, self.regularization)
        else:
            self.solver.least_squares(C, out, gram_reg_fn(), other_factors, self.factors)
        return out[0] if np.isscalar(ids) else out

    def recalculate_user(self, userid, user_items):
        return self._recalculate(userid, user_items, self.item_factors, lambda: self.YtY, lambda: self._YtY_unreg)

    def recalculate_item(self, itemid, item_users):
        return self._recalculate(itemid, item_users, self.user_factors, lambda: self.XtX, lambda: self._XtX_unreg)

    def partial_fit_users(self, userids, user_items):
        if len(userids) != user_items.shape[0]:
            raise ValueError("user_items must contain 1 row for every user in userids")
        new_rows = self.recalculate_user(userids, user_items)
        rows, factors = self.user_factors.shape
        if max(userids) >= rows:
            self.user_factors.resize(max(userids) + 1, factors)
        self.user_factors.assign_rows(userids, new_rows)  # same dtype on both sides (fp16 models: scattered on the device)
        self._user_norms = self._user_norms_host = None
        self._XtX = self._XtX0 = None

    def partial_fit_items(self, itemids, item_users):
        if len(itemids) != item_users.shape[0]:
            raise ValueError("item_users must contain 1 row for every user in itemids")
        new_rows = self.recalculate_item(itemids, item_users)
        rows, factors = self.item_factors.shape
        if max(itemids) >= rows:
            self.item_factors.resize(max(itemids) + 1, factors)
        self.item_factors.assign_rows(itemids, new_rows)
        self._item_norms = self._item_norms_host = None
        self._YtY = self._YtY0 = None

    # ---- explanations (implicit/cpu/als.py:351-416; the reference's GPU class has none) ---------------------------
    def explain(self, userid, user_items, itemid, user_weights=None, N=10):
        """Which liked items produced the score of `itemid` for `userid`, and how much each contributed.

        `user_items` is the full users x items matrix, indexed by `userid` as in the reference.  Returns
        (total_score, top_contributions, user_weights): the predicted score y_i . x_u (x_u as recalculate_user gives it),
        the N largest contributions as a list of (itemid, score), best first under (score, itemid) descending, and the
        user's weights.  UNLIKE the reference, whose user_weights is scipy's cho_factor tuple, this is a gpu.Matrix: the
        lower-triangular Cholesky factor L (factors x factors, zeros above the diagonal) of
        YtY + regularization I + sum (|c| - 1) y y^T.  Passing it back skips the factorisation and gives the same bits."""
        user_items = check_csr(user_items)
        total, ids, scores, user_weights = self.explain_batch([userid], user_items[userid], [itemid], N=N,
                                                              user_weights=user_weights)
        keep = ids[0, 0] >= 0
        top = [(int(i), float(s)) for i, s in zip(ids[0, 0][keep], scores[0, 0][keep])]
        return float(total[0, 0]), top, user_weights

    def explain_batch(self, userids, user_items, itemids, N=10, user_weights=None):
        """explain() for M items of each of B users in one call.  `user_items` has one row per entry of `userids`, as
        recommend takes it; `itemids` is [B] or [B, M] (the ids recommend returns plug in).  Returns (total_scores [B, M]
        float32, ids [B, M, N] int32, scores [B, M, N] float32, user_weights): lists shorter than N are padded with
        (-1, -FLT_MAX); user_weights is a gpu.Matrix of B stacked factors, (B * factors) x factors, to pass back."""
        user_items = check_csr(user_items)
        userids = np.asarray(userids).reshape(-1)
        count, f = len(userids), self.factors
        if user_items.shape[0] != count:
            raise ValueError("user_items must contain 1 row for every user in userids")
        itemids = np.asarray(itemids)
        if itemids.ndim == 1:
            itemids = itemids[:, None]
        if itemids.ndim != 2 or itemids.shape[0] != count or itemids.shape[1] < 1:
            raise ValueError("itemids must be [len(userids)] or [len(userids), M] item ids")
        items = self.item_factors.shape[0]
        if itemids.size and (itemids.min() < 0 or itemids.max() >= items):
            raise ValueError(f"item id out of range for explain: the model has {items} items")
        if int(N) < 1:
            raise ValueError("explain: N must be >= 1")
        if f > _EXPLAIN_MAX_FACTORS:
            raise ValueError(f"explain keeps a user's triangle on chip: factors must be <= {_EXPLAIN_MAX_FACTORS}, got {f}")
        if self.alpha != 1.0:
            user_items = self.alpha * user_items
        C = gpu.CSRMatrix(user_items.astype(np.float32))
        Y = _as_f32(self.item_factors)
        if user_weights is None:
            user_weights = gpu.Matrix.zeros(count * f, f)
            try:
                self.solver.explain_factor(C, self._YtY_unreg, Y, self.regularization, user_weights)
            except ValueError as e:
                row = getattr(e, "failed_row", -1)
                if row < 0:
                    raise
                raise ValueError(f"the normal matrix of user {userids[row]} (row {row} of the batch) is not positive definite. "
                                 "Try increasing the regularization parameter.") from e
        elif not isinstance(user_weights, gpu.Matrix) or user_weights.shape != (count * f, f) or user_weights.itemsize != 4:
            raise ValueError(f"user_weights must be the float32 gpu.Matrix of shape ({count * f}, {f}) an earlier call returned")
        M = itemids.shape[1]
        ids_dev = gpu.IntVector(np.ascontiguousarray(itemids, dtype=np.int32).reshape(-1))
        total, ids, scores = self.solver.explain(C, Y, user_weights, ids_dev, M, int(N))
        return total.reshape(count, M), ids.reshape(count, M, int(N)), scores.reshape(count, M, int(N)), user_weights

    # ---- cached gramians ------------------------------------------------------------------------------
    @property
    def solver(self):
        if self._solver is None:
            self._solver = gpu.LeastSquaresSolver()
        return self._solver

    def _gram(self, factors, reg):
        out = gpu.Matrix.zeros(self.factors, self.factors)
        self.solver.calculate_yty(factors, out, reg)
        return out

    @property
    def YtY(self):
        if self._YtY is None:
            self._YtY = self._gram(self.item_factors, self.regularization)
        return self._YtY

    @property
    def XtX(self):
        if self._XtX is None:
            self._XtX = self._gram(self.user_factors, self.regularization)
        return self._XtX

    @property
    def _YtY_unreg(self):
        if self._YtY0 is None:
            self._YtY0 = self._gram(self.item_factors, 0.0)
        return self._YtY0

    @property
    def _XtX_unreg(self):
        if self._XtX0 is None:
            self._XtX0 = self._gram(self.user_factors, 0.0)
        return self._XtX0

    def to_cpu(self):
        """implicit/gpu/als.py:300-313: the same model as the reference's CPU class."""
        return self._cpu_twin("als", "AlternatingLeastSquares", factors=self.factors, regularization=self.regularization,
                              alpha=self.alpha, dtype=np.float32, iterations=self.iterations, use_cg=self.use_cg,
                              calculate_training_loss=self.calculate_training_loss, random_state=self.random_state)

    # ---- persistence (same .npz keys as implicit/cpu/als.py:458-477 so stock implicit can load it; save / load:
    # MatrixFactorizationBase); num_threads and use_native are keys written by the CPU model ----
    _npz_keys = ("regularization", "factors", "iterations", "use_cg", "cg_steps", "calculate_training_loss", "dtype",
                 "random_state", "alpha")
    _npz_stale = ("num_threads", "use_native")

    def __getstate__(self):
        state = super().__getstate__()
        state["_solver"] = None
        state["comm"] = None  # a communicator belongs to a process group, not to a model file
        state["_XtX0"] = state["_YtY0"] = None
        state["_XtX"] = self._XtX.to_numpy() if self._XtX is not None else None
        state["_YtY"] = self._YtY.to_numpy() if self._YtY is not None else None
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        if self._XtX is not None:
            self._XtX = gpu.Matrix(self._XtX)
        if self._YtY is not None:
            self._YtY = gpu.Matrix(self._YtY)


def _as_f32(m):
    return m if m.itemsize == 4 else m.astype(np.float32)


class _progress:
    """tqdm when available and asked for, otherwise a no-op."""

    def __init__(self, total, show):
        self.bar = None
        if show:
            try:
                from tqdm.auto import tqdm

                self.bar = tqdm(total=total)
            except ImportError:
                pass

    def update(self, loss):
        if self.bar is not None:
            self.bar.update(1)
            if loss is not None:
                self.bar.set_postfix({"loss": loss})

    def close(self):
        if self.bar is not None:
            self.bar.close()


def calculate_loss(Cui, X, Y, regularization, solver=None):
    """Module-level helper of implicit/gpu/als.py:330-341."""
    if not isinstance(Cui, gpu.CSRMatrix):
        Cui = gpu.CSRMatrix(Cui)
    if not isinstance(X, gpu.Matrix):
        X = gpu.Matrix(X)
    if not isinstance(Y, gpu.Matrix):
        Y = gpu.Matrix(Y)
    if solver is None:
        solver = gpu.LeastSquaresSolver()
    return solver.calculate_loss(Cui, X, Y, regularization)
