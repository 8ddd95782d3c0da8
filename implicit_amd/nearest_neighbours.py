"""Item-item nearest-neighbour recommenders on MI355X, at the module path of implicit/nearest_neighbours.py.

The reference computes these models on the CPU only (implicit/_nearest_neighbours.pyx: all_pairs_knn for fit, a per-user
NearestNeighboursScorer loop for recommend).  Here both run through one device primitive, a sparse x sparse product with a
per-row top-k (implicit_amd.gpu.sparse_topk_product, csrc/knn.hip):

  fit        A = the weighted items x users matrix, B = users x items, k = K
  recommend  A = the batch's user rows, B = the similarity matrix, k = N (+ filters), own items zeroed but kept

Every score is the reference's fp64 sum, taken in the same order.  The weighting (normalize, tfidf_weight, bm25_weight)
stays on the host in float64.  `num_threads` is accepted and ignored; there is no CPU fallback.
"""
import numpy as np
from numpy import bincount, log, log1p, sqrt
from scipy.sparse import coo_matrix, csr_matrix

from .recommender_base import RecommenderBase
from .utils import check_csr


def _gpu():
    import implicit_amd.gpu as gpu

    if not gpu.HAS_CUDA:
        raise ValueError("No usable HIP device / extension: implicit_amd's nearest-neighbour models run on the GPU only")
    return gpu


def _topk(A, B, k, zero_own_columns=False):
    gpu = _gpu()
    if not isinstance(A, gpu.SpMat):
        A = gpu.SpMat(A)
    return gpu.sparse_topk_product(A, B, k, zero_own_columns)


def all_pairs_knn(users, K=100, num_threads=0, show_progress=True):
    """The top K nearest neighbours of every column of `users` (users x items), as an items x items COO matrix of
    items * K entries: row i holds its min(K, touched) best (item, score) pairs, then (0, 0, 0.0) padding, as the
    reference's all_pairs_knn returns it.  `num_threads` and `show_progress` are accepted and ignored."""
    users = check_csr(users)
    if not users.has_canonical_format:
        users = users.copy()
        users.sum_duplicates()
    K = int(K)
    items = users.T.tocsr()
    item_count = items.shape[0]
    gpu = _gpu()
    ids, scores, counts = _topk(items, gpu.SpMat(users), K)
    keep = np.arange(K)[None, :] < counts[:, None]
    rows = np.where(keep, np.arange(item_count, dtype=np.int32)[:, None], 0).ravel()
    cols = np.where(keep, ids, 0).ravel().astype(np.int32)
    values = np.where(keep, scores, 0.0).ravel()
    return coo_matrix((values, (rows, cols)), shape=(item_count, item_count))


class ItemItemRecommender(RecommenderBase):
    """Base class of the item-item nearest-neighbour models.

    K: neighbours kept per item in the similarity matrix.  num_threads: accepted for the reference's signature, ignored.
    """

    def __init__(self, K=20, num_threads=0):
        self.similarity = None
        self.K = K
        self.num_threads = num_threads
        self._device_similarity = None

    def fit(self, weighted, show_progress=True, callback=None):
        """Computes and stores the similarity matrix (items x items CSR, float64) from a weighted users x items matrix."""
        if callback:
            raise NotImplementedError("callback isn't support on ItemItemRecommender.fit")
        self.similarity = all_pairs_knn(weighted, self.K, show_progress=show_progress, num_threads=self.num_threads).tocsr()
        self._device_similarity = None

    def _similarity_on_device(self):
        if self._device_similarity is None:
            self._device_similarity = _gpu().SpMat(self.similarity)
        return self._device_similarity

    def _scores(self, user_items, k, remove_own_likes):
        """One device call for every row of user_items: (ids, scores, counts) of the top k."""
        n_items = self.similarity.shape[0]
        indices = user_items.indices
        if len(indices) and (indices.max() >= n_items or indices.min() < 0):
            raise IndexError("user_items refers to items that are not in the model")
        A = csr_matrix((user_items.data.astype(np.float64), indices, user_items.indptr), shape=(user_items.shape[0], n_items))
        return _topk(A, self._similarity_on_device(), k, remove_own_likes)

    def recommend(self, userid, user_items, N=10, filter_already_liked_items=True, filter_items=None,
                  recalculate_user=False, items=None):
        if not isinstance(user_items, csr_matrix):
            raise ValueError("user_items needs to be a CSR sparse matrix")
        if not np.isscalar(userid):
            if user_items.shape[0] != len(userid):
                raise ValueError("user_items must contain 1 row for every user in userids")
        if filter_items is not None and items is not None:
            raise ValueError("Can't specify both filter_items and items")

        scalar = np.isscalar(userid)
        rows = user_items[0:1] if scalar else user_items
        k = N
        if filter_items is not None:
            filter_items = np.asarray(filter_items)
            k = N + len(filter_items)
        elif items is not None:
            items = np.array(items)
            k = self.similarity.shape[0]
            if items.max() >= k or items.min() < 0:
                raise IndexError("Some of selected itemids are not in the model")
        ids, scores, counts = self._scores(rows, max(k, 1), filter_already_liked_items)
        ids, scores = ids[:, :k], scores[:, :k]
        valid = np.arange(k)[None, :] < counts[:, None]

        if scalar:
            row_ids, row_scores = ids[0][valid[0]], scores[0][valid[0]]
            return self._post_filter(row_ids, row_scores, k, filter_items, items)

        if items is None:
            if filter_items is not None:
                valid &= np.isin(ids, filter_items, invert=True)
            # move every row's kept entries to its front, in order, then pad as the reference's _batch_call does
            order = np.argsort(~valid, axis=1, kind="stable")[:, :N]
            out_ids = np.take_along_axis(ids, order, axis=1)
            out_scores = np.take_along_axis(scores, order, axis=1)
            kept = np.take_along_axis(valid, order, axis=1)
            out_ids = np.where(kept, out_ids, -1).astype(np.int32)
            out_scores = np.where(kept, out_scores, -np.finfo(np.float32).max)
            if out_ids.shape[1] < N:
                pad = N - out_ids.shape[1]
                out_ids = np.hstack([out_ids, np.full((len(out_ids), pad), -1, np.int32)])
                out_scores = np.hstack([out_scores, np.full((len(out_ids), pad), -np.finfo(np.float32).max)])
            return out_ids, out_scores

        out_ids = np.full((len(userid), N), -1, dtype=np.int32)
        out_scores = np.full((len(userid), N), -np.finfo(np.float32).max, dtype=np.float64)
        for i in range(len(userid)):
            row_ids, row_scores = self._post_filter(ids[i][valid[i]], scores[i][valid[i]], k, None, items)
            n = min(N, len(row_ids))
            out_ids[i, :n], out_scores[i, :n] = row_ids[:n], row_scores[:n]
        return out_ids, out_scores

    @staticmethod
    def _post_filter(ids, scores, k, filter_items, items):
        """The reference's handling of one user's ranked (ids, scores)."""
        if filter_items is not None:
            mask = np.isin(ids, filter_items, invert=True)
            ids, scores = ids[mask][:k], scores[mask][:k]
        elif items is not None:
            mask = np.isin(ids, items)
            ids, scores = ids[mask], scores[mask]
            missing = items[np.isin(items, ids, invert=True)]
            if missing.size:
                ids = np.append(ids, missing)
                scores = np.append(scores, np.full(missing.size, -np.finfo(scores.dtype).max))
        return ids, scores

    def similar_users(self, userid, N=10, filter_users=None, users=None):
        raise NotImplementedError("similar_users isn't implemented for item-item recommenders")

    def similar_items(self, itemid, N=10, recalculate_item=False, item_users=None, filter_items=None, items=None):
        """Reads the stored similarity rows (host CSR), ranked as the reference ranks them."""
        if recalculate_item:
            raise NotImplementedError("Recalculate_item isn't implemented")
        if filter_items is not None and items is not None:
            raise ValueError("Can't specify both filter_items and items")
        if items is not None:
            items = np.array(items)
        if not np.isscalar(itemid):
            out_ids = np.full((len(itemid), N), -1, dtype=np.int32)
            out_scores = np.full((len(itemid), N), -np.finfo(np.float32).max, dtype=np.float64)
            for i, item in enumerate(itemid):
                ids, scores = self._similar_item(item, N, filter_items, items)
                out_ids[i, : len(ids)], out_scores[i, : len(ids)] = ids[:N], scores[:N]
            return out_ids, out_scores
        return self._similar_item(itemid, N, filter_items, items)

    def _similar_item(self, itemid, N, filter_items, items):
        if itemid >= self.similarity.shape[0]:
            return np.array([]), np.array([])
        start, end = self.similarity.indptr[itemid], self.similarity.indptr[itemid + 1]
        ids, scores = self.similarity.indices[start:end], self.similarity.data[start:end]
        ids, scores = self._post_filter(ids, scores, len(ids), filter_items, items)
        best = np.argsort(scores)[::-1][:N]
        return ids[best], scores[best]

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_device_similarity"] = None  # a device handle: rebuilt from `similarity` on first use
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._device_similarity = None

    def save(self, fileobj_or_path):
        """The reference's npz layout: K, and shape / data / indptr / indices of the similarity matrix once fitted."""
        args = {"K": self.K}
        m = self.similarity
        if m is not None:
            args.update({"shape": m.shape, "data": m.data, "indptr": m.indptr, "indices": m.indices})
        np.savez(fileobj_or_path, **args)

    @classmethod
    def load(cls, fileobj_or_path):
        if isinstance(fileobj_or_path, str) and not fileobj_or_path.endswith(".npz"):
            fileobj_or_path = fileobj_or_path + ".npz"
        with np.load(fileobj_or_path, allow_pickle=False) as data:
            ret = cls()
            if data.get("data") is not None:
                ret.similarity = csr_matrix((data["data"], data["indices"], data["indptr"]), shape=tuple(data["shape"]))
            ret.K = int(data["K"])
            return ret


class CosineRecommender(ItemItemRecommender):
    """An item-item recommender on cosine similarity between items."""

    def fit(self, counts, show_progress=True, callback=None):
        ItemItemRecommender.fit(self, normalize(counts.T).T, show_progress, callback)


class TFIDFRecommender(ItemItemRecommender):
    """An item-item recommender on TF-IDF weighted cosine similarity between items."""

    def fit(self, counts, show_progress=True, callback=None):
        ItemItemRecommender.fit(self, normalize(tfidf_weight(counts.T)).T, show_progress, callback)


class BM25Recommender(ItemItemRecommender):
    """An item-item recommender on BM25 weighted similarity between items."""

    def __init__(self, K=20, K1=1.2, B=0.75, num_threads=0):
        super().__init__(K, num_threads)
        self.K1 = K1
        self.B = B

    def fit(self, counts, show_progress=True, callback=None):
        ItemItemRecommender.fit(self, bm25_weight(counts.T, self.K1, self.B).T, show_progress, callback)


def _idf(X):
    """log(N) - log(1 + document frequency) of every column of the COO matrix X (N = its row count)."""
    return log(float(X.shape[0])) - log1p(bincount(X.col, minlength=X.shape[1]))


def tfidf_weight(X):
    """COO copy of X with every entry x of column c weighted to sqrt(x) * idf(c)."""
    X = coo_matrix(X)
    X.data = sqrt(X.data) * _idf(X)[X.col]
    return X


def normalize(X):
    """COO copy of X with every row scaled to unit L2 norm (scipy / sklearn `normalize` on sparse rows)."""
    X = coo_matrix(X)
    X.data = X.data / sqrt(bincount(X.row, X.data**2, minlength=X.shape[0]))[X.row]
    return X


def bm25_weight(X, K1=100, B=0.8):
    """COO copy of X with every entry x of row r, column c weighted by BM25: x (K1 + 1) / (K1 L_r + x) * idf(c), where
    L_r = (1 - B) + B * rowsum(r) / mean rowsum."""
    X = coo_matrix(X)
    idf = _idf(X)
    row_sums = np.ravel(X.sum(axis=1))
    length_norm = (1.0 - B) + B * row_sums / row_sums.mean()
    X.data = X.data * (K1 + 1.0) / (K1 * length_norm[X.row] + X.data) * idf[X.col]
    return X


__all__ = ["ItemItemRecommender", "CosineRecommender", "TFIDFRecommender", "BM25Recommender", "all_pairs_knn", "normalize",
           "tfidf_weight", "bm25_weight"]
