"""What the two sampled pairwise models (BayesianPersonalizedRanking, WARPMatrixFactorization) share: the initial factors
and fit().  Factors have `factors + 1` columns: the last is the item bias, 1.0 in every user row.

Initial factors follow implicit/gpu/bpr.py:99-128 bit for bit: numpy Generator draws, items before users,
(U[0, 1) - 0.5) / factors, zero rows for users and items without a nonzero, user bias 1.0.  Each epoch then takes one
`rs.integers(2**31)` seed.  Factors are float32 only.
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
    over factors + 1 columns, zero rows for items and users without a nonzero, the user bias column 1.0."""
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


class PairwiseSGDBase(MatrixFactorizationBase):
    """fit() of a model trained by one sampled SGD epoch call per iteration.  A subclass gives `_log_name`, `_epoch` and
    `_postfix`, and says through `_needs_sorted_indices` whether its kernel searches the rows of the matrix."""

    _log_name = None

    def _needs_sorted_indices(self):
        return True

    def _epoch(self, userids, itemids, indptr, seed):
        """One epoch on self.user_factors / self.item_factors; returns the two counts the callback gets."""
        raise NotImplementedError

    def _postfix(self, total, count0, count1):
        """The progress bar's postfix for an epoch's counts over `total` nonzeros, None for none."""
        raise NotImplementedError

    def fit(self, user_items, show_progress=True, callback=None):
        """Trains on a (users x items) CSR matrix; every nonzero is a positive, its value is ignored.  `callback(epoch,
        elapsed, count0, count1)` after every epoch, with the two counts of the model's epoch call."""
        rs = check_random_state(self.random_state)
        user_items = check_csr(user_items)
        if user_items.dtype != np.float32:
            user_items = user_items.astype(np.float32)
        if self._needs_sorted_indices() and not user_items.has_sorted_indices:
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
        total = len(itemids)
        log.debug("Running %i %s training epochs", self.iterations, self._log_name)
        progress = _progress(self.iterations, show_progress)
        for epoch in range(self.iterations):
            t0 = time.time()
            count0, count1 = self._epoch(d_userids, d_itemids, d_indptr, rs.integers(2**31))
            progress.update(None)
            postfix = self._postfix(total, count0, count1) if progress.bar is not None else None
            if postfix:
                progress.bar.set_postfix(postfix)
            if callback:
                callback(epoch, time.time() - t0, count0, count1)
        progress.close()
        self._check_fit_errors()
