"""WARP-loss matrix factorization on MI355X.

No reference counterpart: the loss is Weston, Bengio and Usunier, "WSABIE: Scaling Up To Large Vocabulary Image
Annotation" (IJCAI 2011).  Training runs one imp_warp_update call per epoch (warp_epoch, csrc/warp.hip, which states the
update); recommend / similar_* / rank_items / pickling come from MatrixFactorizationBase.  Factors have `factors + 1`
columns: the last is the item bias, 1.0 in every user row.

Initial factors are those of BayesianPersonalizedRanking bit for bit: numpy Generator draws, items before users,
(U[0, 1) - 0.5) / factors, zero rows for users and items without a nonzero, user bias 1.0.  Each epoch then takes one
`rs.integers(2**31)` seed.  Factors are float32 only.
"""
import logging
import time

import numpy as np

import implicit_amd.gpu as gpu

from ..utils import check_csr, check_random_state
from .als import _progress
from .bpr import initial_bias_factors
from .matrix_factorization_base import MatrixFactorizationBase

log = logging.getLogger("implicit_amd")


class WARPMatrixFactorization(MatrixFactorizationBase):
    """Matrix factorization under the WARP ranking loss.

    For every positive (user, item), up to `max_sampled` (1 .. 4096) items are drawn uniformly until one the user has not
    liked scores within a margin of 1 of the positive; the SGD step is weighted by a rank estimate taken from the number of
    draws that took, so mistakes near the top of the list weigh most.  factors, learning_rate, regularization, iterations:
    as BayesianPersonalizedRanking.  random_state: int, numpy RandomState / Generator or None -- seeds the initial factors
    and the per-epoch sample streams.
    """

    def __init__(self, factors=100, learning_rate=0.02, regularization=0.01, iterations=30, max_sampled=10, random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        if not 1 <= int(max_sampled) <= 4096:
            raise ValueError("max_sampled must lie in 1 .. 4096")
        self.factors = factors
        self.learning_rate = learning_rate
        self.iterations = iterations
        self.regularization = regularization
        self.max_sampled = int(max_sampled)
        self.random_state = random_state

    def fit(self, user_items, show_progress=True, callback=None):
        """Trains on a (users x items) CSR matrix; every nonzero is a positive, its value is ignored.  `callback(epoch,
        elapsed, satisfied, trials)` after every epoch: the samples that found no violating negative and the draws consumed."""
        rs = check_random_state(self.random_state)
        user_items = check_csr(user_items)
        if user_items.dtype != np.float32:
            user_items = user_items.astype(np.float32)
        if not user_items.has_sorted_indices:
            user_items = user_items.copy()  # the caller's matrix stays as it was
            user_items.sort_indices()
        users, _ = user_items.shape
        indptr = np.ascontiguousarray(user_items.indptr, dtype=np.int32)
        itemids = np.ascontiguousarray(user_items.indices, dtype=np.int32)
        user_counts = np.ediff1d(indptr)
        userids = np.repeat(np.arange(users, dtype=np.int32), user_counts)

        initial_bias_factors(self, rs, user_items, user_counts)
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None

        d_userids, d_itemids, d_indptr = gpu.IntVector(userids), gpu.IntVector(itemids), gpu.IntVector(indptr)
        X, Y = self.user_factors, self.item_factors
        total = len(itemids)
        log.debug("Running %i WARP training epochs", self.iterations)
        progress = _progress(self.iterations, show_progress)
        for epoch in range(self.iterations):
            t0 = time.time()
            satisfied, trials = gpu.warp_epoch(d_userids, d_itemids, d_indptr, X, Y, self.learning_rate, self.regularization,
                                               rs.integers(2**31), self.max_sampled)
            progress.update(None)
            if progress.bar is not None and total:
                progress.bar.set_postfix({"satisfied": f"{100.0 * satisfied / total:0.2f}%", "trials": f"{trials / total:0.2f}"})
            if callback:
                callback(epoch, time.time() - t0, satisfied, trials)
        progress.close()
        self._check_fit_errors()

    # ---- persistence (the .npz keys of BayesianPersonalizedRanking.save, max_sampled in place of verify_negative_samples) ----
    def save(self, fileobj_or_path):
        args = {
            "user_factors": None if self.user_factors is None else self.user_factors.to_numpy(),
            "item_factors": None if self.item_factors is None else self.item_factors.to_numpy(),
            "regularization": self.regularization,
            "factors": self.factors,
            "learning_rate": self.learning_rate,
            "max_sampled": self.max_sampled,
            "iterations": self.iterations,
            "dtype": "float32",
            "random_state": self.random_state if isinstance(self.random_state, (int, np.integer)) else None,
        }
        np.savez(fileobj_or_path, **{k: v for k, v in args.items() if v is not None})

    @classmethod
    def load(cls, fileobj_or_path):
        model = super().load(fileobj_or_path)
        for name in ("user_factors", "item_factors"):
            value = getattr(model, name, None)
            if isinstance(value, np.ndarray):
                setattr(model, name, gpu.Matrix(np.ascontiguousarray(value, dtype=np.float32)))
        if hasattr(model, "dtype"):  # written for the file's readers, not a constructor argument
            delattr(model, "dtype")
        return model
