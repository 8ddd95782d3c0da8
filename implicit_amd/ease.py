"""EASE, the closed-form linear item-item autoencoder (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", 2019),
fitted and served on MI355X.  The reference has no such model.

With X the users x items matrix:

    G = X^T X + regularization I        implicit_amd.gpu.ease_gram      (csrc/ease.hip)
    P = G^-1                            implicit_amd.gpu.spd_inverse    (csrc/spd_inverse.hip, fp32 matrix cores)
    B[i, j] = -P[i, j] / P[j, j]        implicit_amd.gpu.ease_weights   (B[j, j] = 0)
    score(u, .) = X[u, :] B             implicit_amd.gpu.ease_topk

There is nothing to tune except `regularization`; the fit is one dense inverse of order `items`, so it needs two float32
items x items matrices of device memory.  There is no CPU fallback.
"""
import numpy as np
from scipy.sparse import csr_matrix

from .recommender_base import RecommenderBase
from .utils import check_csr, transpose_csr


def _gpu():
    import implicit_amd.gpu as gpu

    if not gpu.HAS_CUDA:
        raise ValueError("No usable HIP device / extension: implicit_amd's EASE model runs on the GPU only")
    return gpu


class EASE(RecommenderBase):
    """regularization: the ridge term lambda added to the diagonal of X^T X (the model's only parameter).

    After fit(): item_weights, a float32 items x items implicit_amd.gpu.Matrix B with a zero diagonal; column j holds the
    ridge regression of item j on every other item."""

    _name = "EASE"  # what the error texts call the model (SLIM shares the serving half)

    def __init__(self, regularization=500.0):
        self.regularization = regularization
        self.item_weights = None
        self._knn = None

    # ---- training ----------------------------------------------------------------------------------------------------------
    def fit(self, user_items, show_progress=True, callback=None):
        """Computes item_weights from a users x items CSR matrix (duplicates are summed, values taken as float32).
        MemoryError when the device cannot hold the two items x items matrices of the fit; ValueError naming the item when
        X^T X + regularization I is not positive definite in float32."""
        if callback:
            raise NotImplementedError("callback isn't supported on EASE.fit")
        gpu = _gpu()
        user_items = check_csr(user_items)
        if not user_items.has_canonical_format:
            user_items = user_items.copy()
            user_items.sum_duplicates()
        if user_items.dtype != np.float32:
            user_items = user_items.astype(np.float32)
        items = int(user_items.shape[1])
        need = 2 * items * items * 4
        free, _ = gpu.mem_get_info()
        if need > free:
            raise MemoryError(f"EASE.fit needs {need} bytes of device memory for two float32 {items} x {items} matrices, "
                              f"{free} bytes are free")
        item_users = transpose_csr(user_items)
        G = gpu.ease_gram(gpu.CSRMatrix(item_users), gpu.CSRMatrix(user_items), self.regularization)
        try:
            gpu.spd_inverse(G)
        except ValueError as e:
            item = getattr(e, "failed_pivot", -1)
            if item < 0:
                raise
            raise ValueError(f"EASE.fit: X^T X + {self.regularization} I is not positive definite at item {item}; "
                             "raise the regularization") from e
        self.item_weights = gpu.ease_weights(G)
        self._knn = None

    # ---- serving -----------------------------------------------------------------------------------------------------------
    def _query(self):
        if self._knn is None:
            self._knn = _gpu().KnnQuery()
        return self._knn

    def _items(self):
        if self.item_weights is None:
            raise ValueError(f"{self._name}: the model has not been fitted")
        return self.item_weights.shape[0]

    def _topk(self, rows, N, filter_liked, filter_items, items):
        """(ids, scores) of `rows` (a canonical CSR, one query per row): rows x N, padded with (-1, -FLT_MAX)."""
        gpu = _gpu()
        n_items = self._items()
        if filter_items is not None and items is not None:
            raise ValueError("Can't specify both filter_items and items")
        item_filter = None
        if filter_items is not None:
            item_filter = np.unique(np.asarray(filter_items)).astype(np.int32)
            if len(item_filter) and (item_filter.min() < 0 or item_filter.max() >= n_items):
                raise IndexError("Some of the filtered itemids are not in the model")
        elif items is not None:
            items = np.unique(np.asarray(items))
            if len(items) and (items.max() >= n_items or items.min() < 0):
                raise IndexError("Some of selected itemids are not in the model")
            # the complement goes to the device as a filter: no over-fetch, no k = items call
            keep = np.zeros(n_items, dtype=bool)
            keep[items] = True
            item_filter = np.flatnonzero(~keep).astype(np.int32)
        N = int(N)
        k = N if items is None else min(N, len(items))
        out_ids = np.full((rows.shape[0], N), -1, dtype=np.int32)
        out_scores = np.full((rows.shape[0], N), -np.finfo(np.float32).max, dtype=np.float32)
        if k >= 1 and rows.shape[0]:
            if len(rows.indices) and (rows.indices.max() >= n_items or rows.indices.min() < 0):
                raise IndexError("user_items refers to items that are not in the model")
            ids, scores = gpu.ease_topk(self._query(), self.item_weights, rows, k, filter_liked,
                                        item_filter if item_filter is not None and len(item_filter) else None)
            out_ids[:, :k], out_scores[:, :k] = ids, scores
        return out_ids, out_scores

    @staticmethod
    def _canonical(rows):
        if not rows.has_canonical_format:
            rows = rows.copy()
            rows.sum_duplicates()
        return rows

    def recommend(self, userid, user_items, N=10, filter_already_liked_items=True, filter_items=None,
                  recalculate_user=False, items=None):
        """The N best items of each user by X[u, :] B -> (ids int32, scores float32): 1-d for a scalar userid, len(userid) x N
        otherwise, padded with (-1, -FLT_MAX).  The scores always come from the `user_items` rows passed in (one row per
        user, as for the item-item models), so `recalculate_user` is accepted and has no effect.  filter_items: ids never
        returned; items: the only ids that may be returned (N becomes min(N, len(items))); both together raise ValueError."""
        if not isinstance(user_items, csr_matrix):
            raise ValueError("user_items needs to be a CSR sparse matrix")
        scalar = np.isscalar(userid)
        if not scalar and user_items.shape[0] != len(userid):
            raise ValueError("user_items must contain 1 row for every user in userids")
        if filter_items is not None and items is not None:
            raise ValueError("Can't specify both filter_items and items")
        rows = self._canonical(user_items[0:1] if scalar else user_items)
        ids, scores = self._topk(rows, N, filter_already_liked_items, filter_items, items)
        if scalar:
            keep = ids[0] >= 0
            return ids[0][keep], scores[0][keep]
        return ids, scores

    def similar_items(self, itemid, N=10, recalculate_item=False, item_users=None, filter_items=None, items=None):
        """The N largest entries of row `itemid` of B, i.e. the items that `itemid` votes for most strongly -> (ids, scores).
        The item itself is never returned: its own weight is zero by construction (B has a zero diagonal), so it is filtered
        like a liked item.  `recalculate_item` raises NotImplementedError."""
        if recalculate_item:
            raise NotImplementedError("Recalculate_item isn't implemented")
        scalar = np.isscalar(itemid)
        ids_in = np.atleast_1d(np.asarray(itemid)).astype(np.int64)
        n_items = self._items()
        if len(ids_in) and (ids_in.min() < 0 or ids_in.max() >= n_items):
            raise IndexError("Some of the itemids are not in the model")
        rows = csr_matrix((np.ones(len(ids_in), dtype=np.float32), ids_in.astype(np.int32),
                           np.arange(len(ids_in) + 1, dtype=np.int64)), shape=(len(ids_in), n_items))
        ids, scores = self._topk(rows, N, True, filter_items, items)
        # the item's own (filtered) entry can only surface when fewer than N other items exist
        own = ids == ids_in[:, None].astype(np.int32)
        ids = np.where(own, -1, ids).astype(np.int32)
        scores = np.where(own, -np.finfo(np.float32).max, scores).astype(np.float32)
        if scalar:
            keep = ids[0] >= 0
            return ids[0][keep], scores[0][keep]
        return ids, scores

    def similar_users(self, userid, N=10, filter_users=None, users=None):
        raise NotImplementedError(f"similar_users isn't implemented for {self._name}: the model has no user representation")

    # ---- persistence -------------------------------------------------------------------------------------------------------
    def __getstate__(self):
        return {"regularization": self.regularization,
                "item_weights": self.item_weights.to_numpy() if self.item_weights is not None else None}

    def __setstate__(self, state):
        self.regularization = state["regularization"]
        w = state["item_weights"]
        self.item_weights = _gpu().Matrix(w) if w is not None else None
        self._knn = None

    def save(self, fileobj_or_path):
        """An .npz with `regularization` and, once fitted, `item_weights` (float32 items x items)."""
        args = {"regularization": self.regularization}
        if self.item_weights is not None:
            args["item_weights"] = self.item_weights.to_numpy()
        np.savez(fileobj_or_path, **args)

    @classmethod
    def load(cls, fileobj_or_path):
        if isinstance(fileobj_or_path, str) and not fileobj_or_path.endswith(".npz"):
            fileobj_or_path = fileobj_or_path + ".npz"
        with np.load(fileobj_or_path, allow_pickle=False) as data:
            ret = cls(regularization=float(data["regularization"]))
            if "item_weights" in data:
                ret.item_weights = _gpu().Matrix(np.ascontiguousarray(data["item_weights"], dtype=np.float32))
            return ret


__all__ = ["EASE"]
