"""PureSVD (Cremonesi, Koren, Turrin, "Performance of Recommender Algorithms on Top-N Recommendation Tasks", RecSys 2010):
the rank-k truncated SVD of the (weighted) interaction matrix served as a matrix-factorization model, fitted on MI355X by
randomized subspace iteration.  The reference has no such model.

With A the users x items matrix and A ~ U S V^T its k leading singular triplets:

    U, S, V = implicit_amd.gpu.randomized_svd      (csrc/svd.hip: spmm, multiply_small; the gramian kernel)
    item_factors = V                               items x k, orthonormal columns
    user_factors = A V                             implicit_amd.gpu.spmm: the fold-in of every training row (~ U S)
    score(u, i)  = user_factors[u] . item_factors[i]

There is nothing to tune except `factors`.  The model is float32 and GPU only; there is no to_cpu().
"""
import numpy as np

import implicit_amd.gpu as gpu

from .gpu.matrix_factorization_base import MatrixFactorizationBase, check_random_state
from .utils import check_csr, transpose_csr


def _canonical_f32(m):
    m = check_csr(m)
    if not m.has_canonical_format:
        m = m.copy()
        m.sum_duplicates()
    if m.dtype != np.float32:
        m = m.astype(np.float32)
    return m


class PureSVD(MatrixFactorizationBase):
    """factors: the rank k of the truncated SVD.  oversample, power_iterations: the extra sketch columns and the power
    iterations of the randomized method (factors + oversample <= 1024).  random_state: int, numpy RandomState / Generator
    or None -- seeds the Gaussian test matrix.

    After fit(): item_factors (V, items x factors), user_factors (A V, users x factors) and singular_values (float64, length
    factors).  Directions whose singular value is below 2^-8 of the largest are given up: a matrix of rank r < factors yields
    r non-zero singular values and zero columns in both factor matrices beyond them."""

    def __init__(self, factors=100, oversample=10, power_iterations=2, random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension: implicit_amd's PureSVD model runs on the GPU only")
        if factors < 1 or oversample < 0 or power_iterations < 0:
            raise ValueError("PureSVD: factors must be >= 1, oversample and power_iterations >= 0")
        if factors + oversample > 1024:
            raise ValueError(f"PureSVD: factors + oversample = {factors + oversample} exceeds 1024")
        self.factors = factors
        self.oversample = oversample
        self.power_iterations = power_iterations
        self.random_state = random_state
        self.singular_values = None

    def fit(self, user_items, show_progress=True, callback=None):
        """Factorizes a users x items CSR matrix (duplicates are summed, values taken as float32)."""
        if callback:
            raise NotImplementedError("callback isn't supported on PureSVD.fit")
        user_items = _canonical_f32(user_items)
        item_users = transpose_csr(user_items)
        A, At = gpu.CSRMatrix(user_items), gpu.CSRMatrix(item_users)
        _, sigma, V = gpu.randomized_svd(A, At, self.factors, oversample=self.oversample, power_iterations=self.power_iterations,
                                         random_state=check_random_state(self.random_state))
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None
        self.item_factors = V
        self.singular_values = sigma
        self.user_factors = gpu.spmm(A, V)
        self._check_fit_errors()

    # ---- fold-in ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _fold_in(ids, rows_csr, other_factors):
        rows_csr = _canonical_f32(rows_csr)
        count = 1 if np.isscalar(ids) else len(ids)
        if rows_csr.shape[0] != count:
            raise ValueError("expected one sparse row for every id to recalculate")
        if rows_csr.shape[1] != other_factors.shape[0]:
            raise ValueError("the rows to fold in must have one column per row of the other side's factors")
        out = gpu.spmm(gpu.CSRMatrix(rows_csr), other_factors)
        return out[0] if np.isscalar(ids) else out

    def recalculate_user(self, userid, user_items):
        """user_items (one row per id in `userid`) times item_factors.  The products of a row are summed in stored order
        whatever else the matrix holds, so folding a training row back in returns that user's stored factors bit for bit."""
        return self._fold_in(userid, user_items, self.item_factors)

    def recalculate_item(self, itemid, item_users):
        """item_users (one row per id in `itemid`) times user_factors: A^T A V = V S^2 up to the truncation, i.e. the item's
        factors scaled by the squared singular values -- the direction similar_items needs, NOT bit-identical (nor equal)
        to the stored rows of V."""
        return self._fold_in(itemid, item_users, self.user_factors)

    # ---- persistence -----------------------------------------------------------------------------------------------------
    _npz_keys = ("factors", "oversample", "power_iterations", "singular_values", "random_state")
    _npz_stale = ("dtype",)  # written for the file's readers; the model has no such attribute
    _npz_dtype = np.float32


__all__ = ["PureSVD"]
