"""LogisticMatrixFactorization on MI355X.

The reference has no GPU LMF (implicit/lmf.py raises NotImplementedError for use_gpu=True); this is its CPU model,
implicit/cpu/lmf.pyx (constructor, fit, save with the same .npz keys without num_threads), trained through one
imp_lmf_update call per half-sweep (lmf_update, csrc/lmf.hip).  recommend / similar_* / save / load / pickling come from
MatrixFactorizationBase.  Factors have `factors + 2` columns: the item matrix holds 1.0 in column C-1 (a user's C-1 is the
user bias), the user matrix 1.0 in column C-2 (an item's C-2 is the item bias).

Initial factors follow lmf.pyx's fit bit for bit: numpy Generator draws, items before users, standard normal float32, the
constant column set to 1.0, zero rows for users and items without a nonzero.  Each half-sweep then takes one
`rs.integers(2**31)` seed (the reference seeds per-thread mt19937 streams instead, which cannot be reproduced).  The
Adagrad accumulators start at zero on every fit().  Factors are float32 only.
"""
import logging
import time

import numpy as np

import implicit_amd.gpu as gpu

from ..utils import check_csr, check_random_state
from .als import _progress
from .matrix_factorization_base import MatrixFactorizationBase

log = logging.getLogger("implicit_amd")


class LogisticMatrixFactorization(MatrixFactorizationBase):
    """Logistic Matrix Factorization (Johnson, "Logistic Matrix Factorization for Implicit Feedback Data").

    factors, learning_rate, regularization, iterations: as the reference.  neg_prop: negatives per positive, capped at
    factors + 2 per row as in the reference's CPU model.  random_state: int, numpy RandomState / Generator or None -- seeds
    the initial factors and the per-half-sweep negative streams.
    """

    def __init__(self, factors=30, learning_rate=1.00, regularization=0.6, dtype=np.float32, iterations=30, neg_prop=30,
                 random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        self.factors = factors
        self.learning_rate = learning_rate
        self.iterations = iterations
        self.regularization = regularization
        self.neg_prop = neg_prop
        self.random_state = random_state

    def _initial_factors(self, rs, users, items, user_counts, item_counts):
        C = self.factors + 2
        if self.item_factors is None:
            item_factors = rs.standard_normal(size=(items, C), dtype=np.float32)
            item_factors[:, -1] = 1.0
            item_factors[item_counts == 0] = np.zeros(C)
            self.item_factors = gpu.Matrix(item_factors)
        if self.user_factors is None:
            user_factors = rs.standard_normal(size=(users, C), dtype=np.float32)
            user_factors[:, -2] = 1.0
            user_factors[user_counts == 0] = np.zeros(C)
            self.user_factors = gpu.Matrix(user_factors)

    def fit(self, user_items, show_progress=True, callback=None):
        """Trains on a (users x items) CSR matrix of confidences.  `callback(epoch, elapsed)` after every epoch."""
        rs = check_random_state(self.random_state)
        if user_items.dtype != np.float32:
            user_items = user_items.astype(np.float32)
        user_items = check_csr(user_items)
        if not user_items.has_sorted_indices:
            user_items = user_items.copy()  # the caller's matrix stays as it was
            user_items.sort_indices()
        item_users = user_items.T.tocsr()
        item_users.sort_indices()
        users, items = user_items.shape
        user_counts = np.ediff1d(user_items.indptr)
        item_counts = np.bincount(user_items.indices, minlength=items)

        self._initial_factors(rs, users, items, user_counts, item_counts)
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None

        X, Y = self.user_factors, self.item_factors
        C = X.shape[1]
        user_deriv_sum = gpu.Matrix.zeros(users, C)
        item_deriv_sum = gpu.Matrix.zeros(items, C)
        cui, ciu = gpu.CSRMatrix(user_items), gpu.CSRMatrix(item_users)
        log.debug("Running %i LMF training epochs", self.iterations)
        progress = _progress(self.iterations, show_progress)
        for epoch in range(self.iterations):
            t0 = time.time()
            gpu.lmf_update(cui, X, Y, user_deriv_sum, self.learning_rate, self.regularization, self.neg_prop,
                           rs.integers(2**31), one_col=C - 2)
            gpu.lmf_update(ciu, Y, X, item_deriv_sum, self.learning_rate, self.regularization, self.neg_prop,
                           rs.integers(2**31), one_col=C - 1)
            progress.update(None)
            if callback:
                callback(epoch, time.time() - t0)
        progress.close()
        self._check_fit_errors()

    def to_cpu(self):
        """The same model as the reference's CPU class."""
        return self._cpu_twin("lmf", "LogisticMatrixFactorization", factors=self.factors, learning_rate=self.learning_rate,
                              regularization=self.regularization, iterations=self.iterations, neg_prop=self.neg_prop,
                              random_state=self.random_state)

    # the .npz keys of implicit/cpu/lmf.pyx save, without num_threads; `dtype` is written for the file's readers
    _npz_keys = ("regularization", "factors", "learning_rate", "neg_prop", "iterations", "dtype", "random_state")
    _npz_stale = ("num_threads", "dtype")
    _npz_dtype = np.float32
