"""BayesianPersonalizedRanking on MI355X.

Public surface of implicit/gpu/bpr.py:15-160 (constructor, fit, to_cpu) plus save / load with the .npz keys of
implicit/cpu/bpr.pyx:228-244 (without num_threads).  Training runs one imp_bpr_update call per epoch (bpr_epoch,
csrc/bpr.hip) with the numerics of the reference's CPU update; recommend / similar_* / pickling come from
MatrixFactorizationBase.  Factors have `factors + 1` columns: the last is the item bias, 1.0 in every user row.

Initial factors follow implicit/gpu/bpr.py:99-128 bit for bit: numpy Generator draws, items before users,
(U[0, 1) - 0.5) / factors, zero rows for users and items without a nonzero, user bias 1.0.  Each epoch then takes one
`rs.integers(2**31)` seed.  Factors are float32 only (the reference's GPU class ignores `dtype` as well).
"""
import logging
import time

import numpy as np

import implicit_amd.gpu as gpu

from ..utils import check_csr, check_random_state
from .als import _progress
from .matrix_factorization_base import MatrixFactorizationBase

log = logging.getLogger("implicit_amd")


def initial_bias_factors(model, rs, user_items, user_counts):
    """Sets the factors `model` does not have yet (implicit/gpu/bpr.py:99-128): items before users, (U[0, 1) - 0.5) / factors
    over factors + 1 columns, zero rows for items and users without a nonzero, the user bias column 1.0.  Shared by the
    pairwise models (BPR here, WARP in warp.py)."""
    users, items = user_items.shape
    if model.item_factors is None:
        item_factors = rs.random((items, model.factors + 1), "float32") - 0.5
        item_factors /= model.factors
        item_counts = np.bincount(user_items.indices, minlength=items)
        item_factors[item_counts == 0] = np.zeros(model.factors + 1)
        model.item_factors = gpu.Matrix(item_factors)
    if model.user_factors is None:
        user_factors = rs.random((users, model.factors + 1), "float32") - 0.5
        user_factors /= model.factors
        user_factors[user_counts == 0] = np.zeros(model.factors + 1)
        user_factors[:, model.factors] = 1.0
        model.user_factors = gpu.Matrix(user_factors)


class BayesianPersonalizedRanking(MatrixFactorizationBase):
    """Bayesian Personalized Ranking (Rendle et al., "BPR: Bayesian Personalized Ranking from Implicit Feedback").

    factors, learning_rate, regularization, iterations: as the reference.  verify_negative_samples: skip a sampled negative
    the user has liked (costs a search of the user's row per sample).  random_state: int, numpy RandomState / Generator or
    None -- seeds the initial factors and the per-epoch sample streams.
    """

    def __init__(self, factors=100, learning_rate=0.01, regularization=0.01, dtype=np.float32, iterations=100,
                 verify_negative_samples=True, random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        self.factors = factors
        self.learning_rate = learning_rate
        self.iterations = iterations
        self.regularization = regularization
        self.verify_negative_samples = verify_negative_samples
        self.random_state = random_state

    def fit(self, user_items, show_progress=True, callback=None):
        """Trains on a (users x items) CSR matrix; every nonzero is a positive, its value is ignored.  `callback(epoch,
        elapsed, correct, skipped)` after every epoch."""
        rs = check_random_state(self.random_state)
        user_items = check_csr(user_items)
        if user_items.dtype != np.float32:
            user_items = user_items.astype(np.float32)
        if self.verify_negative_samples and not user_items.has_sorted_indices:
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
        log.debug("Running %i BPR training epochs", self.iterations)
        progress = _progress(self.iterations, show_progress)
        for epoch in range(self.iterations):
            t0 = time.time()
            correct, skipped = gpu.bpr_epoch(d_userids, d_itemids, d_indptr, X, Y, self.learning_rate, self.regularization,
                                             rs.integers(2**31), self.verify_negative_samples)
            progress.update(None)
            if progress.bar is not None and total and total != skipped:
                progress.bar.set_postfix({"train_auc": f"{100.0 * correct / (total - skipped):0.2f}%",
                                          "skipped": f"{100.0 * skipped / total:0.2f}%"})
            if callback:
                callback(epoch, time.time() - t0, correct, skipped)
        progress.close()
        self._check_fit_errors()

    def to_cpu(self):
        """implicit/gpu/bpr.py:147-160: the same model as the reference's CPU class.  This package does not ship a CPU model,
        so stock `implicit` has to be importable."""
        try:
            import implicit.cpu.bpr as cpu_bpr
        except ImportError as e:
            raise ImportError("to_cpu() builds implicit.cpu.bpr.BayesianPersonalizedRanking: install benfred/implicit for the "
                              "CPU model (implicit_amd ships the MI355X path only)") from e
        ret = cpu_bpr.BayesianPersonalizedRanking(factors=self.factors, learning_rate=self.learning_rate,
                                                  regularization=self.regularization, iterations=self.iterations,
                                                  verify_negative_samples=self.verify_negative_samples,
                                                  random_state=self.random_state)
        ret.user_factors = None if self.user_factors is None else self.user_factors.to_numpy()
        ret.item_factors = None if self.item_factors is None else self.item_factors.to_numpy()
        return ret

    # ---- persistence (the .npz keys of implicit/cpu/bpr.pyx:228-244, without num_threads) ----------------
    def save(self, fileobj_or_path):
        args = {
            "user_factors": None if self.user_factors is None else self.user_factors.to_numpy(),
            "item_factors": None if self.item_factors is None else self.item_factors.to_numpy(),
            "regularization": self.regularization,
            "factors": self.factors,
            "learning_rate": self.learning_rate,
            "verify_negative_samples": self.verify_negative_samples,
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
        for stale in ("num_threads", "dtype"):  # written by the CPU model / not a constructor argument here
            if hasattr(model, stale):
                delattr(model, stale)
        return model
