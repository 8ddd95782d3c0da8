"""SLIM, the sparse linear item-item model (Ning & Karypis, "SLIM: Sparse Linear Methods for Top-N Recommender Systems", ICDM
2011), fitted and served on MI355X.  The reference has no such model.

With X the users x items matrix, every item j is regressed on all the others under an elastic-net penalty:

    A = X^T X + l2 I                                                   implicit_amd.gpu.ease_gram    (csrc/ease.hip)
    W[:, j] = argmin 1/2 w^T A w - A[j, :] w + l1 |w|_1, w_j = 0       implicit_amd.gpu.slim_solve   (csrc/slim.hip)
              (and w >= 0 when `positive`), by cyclic coordinate descent
    score(u, .) = X[u, :] W                                            implicit_amd.gpu.ease_topk

W has EASE's layout and is served by EASE's code; unlike EASE's B it is sparse and, with `positive`, non-negative.  The fit
needs two float32 items x items matrices of device memory and at most 40 000 items.  There is no CPU fallback."""
import re

import numpy as np
from scipy.sparse import csr_matrix

from .ease import EASE, _gpu
from .utils import check_csr, transpose_csr


class SLIM(EASE):
    """l1_regularization, l2_regularization: the two penalties (l1 sparsifies, l2 is the ridge term on the diagonal of X^T X).
    positive: weights >= 0.  max_sweeps, tol: a column stops after the sweep whose largest change is <= tol times its largest
    weight, and after max_sweeps sweeps at the latest.  The running product of a column is never recomputed, so its rounding
    accumulates: tol = 0 means "exactly max_sweeps sweeps unless a sweep changes nothing", not a fixed point.

    The defaults are placeholders taken from small synthetic problems, not tuned on real data.

    After fit(): item_weights, a float32 items x items implicit_amd.gpu.Matrix W with a zero diagonal (column j holds the
    regression of item j); sweeps_, the sweeps each column ran (int32); density, the nonzero share of the off-diagonal entries;
    sparse_weights() returns W as a scipy CSR matrix."""

    _name = "SLIM"
    _PARAMS = ("l1_regularization", "l2_regularization", "positive", "max_sweeps", "tol")

    def __init__(self, l1_regularization=1.0, l2_regularization=10.0, positive=True, max_sweeps=100, tol=1e-4):
        self.l1_regularization = l1_regularization
        self.l2_regularization = l2_regularization
        self.positive = positive
        self.max_sweeps = max_sweeps
        self.tol = tol
        self.item_weights = None
        self.sweeps_ = None
        self.density = None
        self._sparse = self._sparse_of = None
        self._knn = None

    # ---- training ----------------------------------------------------------------------------------------------------------
    def fit(self, user_items, show_progress=True, callback=None):
        """Computes item_weights from a users x items CSR matrix (duplicates are summed, values taken as float32).
        MemoryError when the device cannot hold the two items x items matrices of the fit and the solver's workspace;
        ValueError naming the item when a diagonal entry of X^T X + l2_regularization I is not positive (an item nobody has,
        with l2_regularization = 0), and when there are more than 40 000 items."""
        if callback:
            raise NotImplementedError("callback isn't supported on SLIM.fit")
        gpu = _gpu()
        user_items = check_csr(user_items)
        if not user_items.has_canonical_format:
            user_items = user_items.copy()
            user_items.sum_duplicates()
        if user_items.dtype != np.float32:
            user_items = user_items.astype(np.float32)
        items = int(user_items.shape[1])
        if items > gpu.SLIM_MAX_ITEMS:
            raise ValueError(f"SLIM.fit: {items} items, at most {gpu.SLIM_MAX_ITEMS} are supported")
        need = 2 * items * items * 4 + gpu.slim_workspace_bytes(items)
        free, _ = gpu.mem_get_info()
        if need > free:
            raise MemoryError(f"SLIM.fit needs {need} bytes of device memory for two float32 {items} x {items} matrices and "
                              f"the solver's workspace, {free} bytes are free")
        item_users = transpose_csr(user_items)
        A = gpu.ease_gram(gpu.CSRMatrix(item_users), gpu.CSRMatrix(user_items), self.l2_regularization)
        try:
            W, sweeps = gpu.slim_solve(A, self.l1_regularization, self.positive, self.max_sweeps, self.tol)
        except ValueError as e:
            bad = re.search(r"diagonal entry of item (\d+)", str(e))
            if not bad:
                raise
            raise ValueError(f"SLIM.fit: the diagonal of X^T X + {self.l2_regularization} I is not positive at item "
                             f"{bad.group(1)}; raise l2_regularization") from e
        self._set_weights(W, sweeps)

    def _set_weights(self, W, sweeps, dense=None):
        """Takes W over; its one copy to the host (the caller's `dense`, where it has one) becomes the CSR form that density,
        sparse_weights(), save and pickling share."""
        self.item_weights = W
        self.sweeps_ = np.ascontiguousarray(sweeps, dtype=np.int32)
        items = W.shape[0]
        self._sparse = csr_matrix(W.to_numpy() if dense is None else dense)
        self._sparse_of = W
        self.density = self._sparse.nnz / (items * (items - 1)) if items > 1 else 0.0  # the diagonal is zero
        self._knn = None

    def sparse_weights(self):
        """W as a float32 scipy CSR matrix (items x items, canonical)."""
        self._items()
        if getattr(self, "_sparse_of", None) is not self.item_weights:  # item_weights was assigned from outside
            self._sparse, self._sparse_of = csr_matrix(self.item_weights.to_numpy()), self.item_weights
        return self._sparse.copy()

    # ---- persistence -------------------------------------------------------------------------------------------------------
    def _params(self):
        return {name: getattr(self, name) for name in self._PARAMS}

    def _state(self):
        """The five parameters and, once fitted, sweeps_ and W as a CSR triple with its shape: never a dense items^2 array."""
        state = self._params()
        if self.item_weights is not None:
            self.sparse_weights()
            W = self._sparse
            state.update(sweeps_=self.sweeps_, indptr=W.indptr.astype(np.int64), indices=W.indices.astype(np.int32),
                         data=W.data.astype(np.float32), shape=np.asarray(W.shape, dtype=np.int64))
        return state

    def _restore(self, state):
        if "indptr" in state:
            shape = tuple(int(x) for x in state["shape"])
            dense = np.ascontiguousarray(csr_matrix((state["data"], state["indices"], state["indptr"]), shape=shape).toarray(),
                                         dtype=np.float32)
            self._set_weights(_gpu().Matrix(dense), state["sweeps_"], dense)

    def __getstate__(self):
        return self._state()

    def __setstate__(self, state):
        self.__init__(**{name: state[name] for name in self._PARAMS})
        self._restore(state)

    def save(self, fileobj_or_path):
        """An .npz with the five parameters and, once fitted, `sweeps_` and the weights as `indptr`, `indices`, `data`, `shape`."""
        np.savez(fileobj_or_path, **self._state())

    @classmethod
    def load(cls, fileobj_or_path):
        if isinstance(fileobj_or_path, str) and not fileobj_or_path.endswith(".npz"):
            fileobj_or_path = fileobj_or_path + ".npz"
        with np.load(fileobj_or_path, allow_pickle=False) as data:
            ret = cls(l1_regularization=float(data["l1_regularization"]), l2_regularization=float(data["l2_regularization"]),
                      positive=bool(data["positive"]), max_sweeps=int(data["max_sweeps"]), tol=float(data["tol"]))
            ret._restore({k: data[k] for k in data.files})
            return ret


__all__ = ["SLIM"]
