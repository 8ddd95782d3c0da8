"""IVFModel: recommend / similar_items of a matrix-factorisation model through IVF-Flat indexes of its item factors.

Behaves as the reference's FaissModel (implicit/ann/faiss.py) with use_gpu=True, on the native index of
implicit_amd.gpu.IVFIndex instead of faiss: an inner-product index for recommend, a second one over the row-normalised
factors for similar_items, filters applied to an over-fetched result on the host, and the exact model as the fall-back
once a query would need 1024 results or more."""
import logging
import warnings

import numpy as np
from scipy.sparse import csr_matrix

import implicit_amd.gpu as gpu

from ..recommender_base import RecommenderBase
from ..utils import ParameterWarning

log = logging.getLogger("implicit")

MAX_RESULTS = 1024  # a search returns at most this many results per query; at or beyond it the exact model answers
_EMPTY_SCORE = -np.finfo(np.float32).max


def _first_unfiltered(ids, scores, drop, N):
    """Per row of ids / scores (rows x count, best first) the first N entries that `drop` (same shape, bool) does not
    mark; rows with fewer survivors end in (-1, -FLT_MAX)."""
    drop = drop | (ids < 0)
    order = np.argsort(drop, axis=1, kind="stable")[:, :N]
    out_ids = np.take_along_axis(ids, order, axis=1)
    out_scores = np.take_along_axis(scores, order, axis=1)
    gone = np.take_along_axis(drop, order, axis=1)
    out_ids[gone], out_scores[gone] = -1, _EMPTY_SCORE
    if out_ids.shape[1] < N:
        pad = N - out_ids.shape[1]
        out_ids = np.pad(out_ids, ((0, 0), (0, pad)), constant_values=-1)
        out_scores = np.pad(out_scores, ((0, 0), (0, pad)), constant_values=_EMPTY_SCORE)
    return out_ids, out_scores


class IVFModel(RecommenderBase):
    """Parameters
    ----------
    model : a fitted-or-not matrix-factorisation model of this package (item_factors / user_factors on the device)
    approximate_similar_items, approximate_recommend : build and use the index for that call; otherwise the exact model
    nlist : lists of the index (clamped to the item count, with a ParameterWarning)
    nprobe : lists scanned per query; above nlist it means nlist, but min(nprobe, nlist) > 1024 makes every search raise
        ValueError (IVFIndex.search probes at most 1024 lists)
    iterations : k-means rounds of the index build
    random_state : seed of the numpy Generator that draws the initial centroids (None: unseeded)

    Attributes
    ----------
    recommend_index, similar_items_index : implicit_amd.gpu.IVFIndex, inner product over the item factors / over the
        row-normalised item factors
    """

    def __init__(self, model, approximate_similar_items=True, approximate_recommend=True, nlist=400, nprobe=20,
                 iterations=10, random_state=None):
        self.model = model
        self.approximate_similar_items = approximate_similar_items
        self.approximate_recommend = approximate_recommend
        self.nlist = nlist
        self.nprobe = nprobe
        self.iterations = iterations
        self.random_state = random_state
        self.recommend_index = None
        self.similar_items_index = None
        self.factors = None

    def fit(self, user_items, show_progress=True, callback=None):
        self.model.fit(user_items, show_progress, callback=callback)
        self.build_indexes()

    def build_indexes(self):
        """(Re)build the indexes from the inner model's current item factors."""
        item_factors = self.model.item_factors
        items, self.factors = item_factors.shape
        nlist = int(self.nlist)
        if nlist > items:
            warnings.warn(f"nlist={nlist} exceeds the {items} items of the model: using {items} lists", ParameterWarning)
            nlist = items
        rng = np.random.default_rng(self.random_state)
        if self.approximate_recommend:
            log.debug("Building the IVF recommendation index")
            self.recommend_index = gpu.IVFIndex.build(item_factors, nlist, self.iterations,
                                                      init_rows=rng.choice(items, size=nlist, replace=False))
        if self.approximate_similar_items:
            log.debug("Building the IVF similar-items index")
            host = item_factors.to_numpy().astype(np.float32)
            norms = np.linalg.norm(host, axis=1)
            norms[norms == 0] = 1e-10
            self.similar_items_index = gpu.IVFIndex.build((host / norms[:, None]).astype(np.float32), nlist, self.iterations,
                                                          init_rows=rng.choice(items, size=nlist, replace=False))

    def recommend(self, userid, user_items, N=10, filter_already_liked_items=True, filter_items=None,
                  recalculate_user=False, items=None):
        scalar = np.isscalar(userid)
        if filter_already_liked_items or recalculate_user:
            if not isinstance(user_items, csr_matrix):
                raise ValueError("user_items needs to be a CSR sparse matrix")
            if user_items.shape[0] != (1 if scalar else len(userid)):
                raise ValueError("user_items must contain 1 row for every user in userids")
        if items is not None and self.approximate_recommend:
            raise NotImplementedError("using an 'items' list with the approximate search isn't supported")

        exact = dict(N=N, filter_already_liked_items=filter_already_liked_items, filter_items=filter_items,
                     recalculate_user=recalculate_user, items=items)
        if not self.approximate_recommend:
            return self.model.recommend(userid, user_items, **exact)

        # over-fetch by everything the filters could remove; one search serves the whole batch, sized by its largest row
        count = N
        if filter_items is not None:
            filter_items = np.asarray(filter_items).reshape(-1)
            count += len(filter_items)
        if filter_already_liked_items:
            liked = np.diff(user_items.indptr)
            count += int(liked.max()) if len(liked) else 0
        if count >= MAX_RESULTS:
            return self.model.recommend(userid, user_items, **exact)

        query = self.model.recalculate_user(userid, user_items) if recalculate_user else self.model._user_query(userid)
        ids, scores = self.recommend_index.search(query, count, self.nprobe)

        drop = np.zeros(ids.shape, dtype=bool)
        if filter_items is not None and len(filter_items):
            drop |= np.isin(ids, filter_items)
        if filter_already_liked_items and user_items.nnz:
            n_items = self.recommend_index.shape[0]
            rows = np.repeat(np.arange(user_items.shape[0], dtype=np.int64), np.diff(user_items.indptr))
            liked_keys = rows * n_items + user_items.indices
            keys = np.arange(ids.shape[0], dtype=np.int64)[:, None] * n_items + ids
            drop |= np.isin(keys, liked_keys) & (ids >= 0)
        ids, scores = _first_unfiltered(ids, scores, drop, N)
        return (ids[0], scores[0]) if scalar else (ids, scores)

    def similar_items(self, itemid, N=10, recalculate_item=False, item_users=None, filter_items=None, items=None):
        if items is not None and self.approximate_similar_items:
            raise NotImplementedError("using an 'items' filter isn't supported with the approximate search")
        count = N
        if filter_items is not None:
            filter_items = np.asarray(filter_items).reshape(-1)
            count += len(filter_items)
        if not self.approximate_similar_items or count >= MAX_RESULTS:
            return self.model.similar_items(itemid, N, recalculate_item=recalculate_item, item_users=item_users,
                                            filter_items=filter_items, items=items)

        scalar = np.isscalar(itemid)
        factors = self.model.recalculate_item(itemid, item_users) if recalculate_item else self.model.item_factors[itemid]
        factors = factors.to_numpy().astype(np.float32).reshape(-1, self.factors)
        norms = np.linalg.norm(factors, axis=1)
        norms[norms == 0] = 1e-10
        ids, scores = self.similar_items_index.search(factors / norms[:, None], count, self.nprobe)
        drop = np.zeros(ids.shape, dtype=bool)
        if filter_items is not None and len(filter_items):
            drop |= np.isin(ids, filter_items)
        ids, scores = _first_unfiltered(ids, scores, drop, N)
        return (ids[0], scores[0]) if scalar else (ids, scores)

    def explain(self, userid, user_items, itemid, user_weights=None, N=10):
        """Exact: explanations do not search the index; forwarded to the wrapped model (ALS only)."""
        return self.model.explain(userid, user_items, itemid, user_weights=user_weights, N=N)

    def explain_batch(self, userids, user_items, itemids, N=10, user_weights=None):
        return self.model.explain_batch(userids, user_items, itemids, N=N, user_weights=user_weights)

    def rank_items(self, userid, user_items, selected_items, N=None, filter_already_liked_items=False,
                   recalculate_user=False):
        """Exact: ranking given candidates does not search the index; forwarded to the wrapped model."""
        return self.model.rank_items(userid, user_items, selected_items, N=N,
                                     filter_already_liked_items=filter_already_liked_items, recalculate_user=recalculate_user)

    def score_items(self, userid, selected_items, user_items=None, recalculate_user=False):
        return self.model.score_items(userid, selected_items, user_items=user_items, recalculate_user=recalculate_user)

    def similar_users(self, userid, N=10, filter_users=None, users=None):
        raise NotImplementedError("similar_users isn't implemented with the approximate index "
                                  "(self.model.similar_users gives the exact result)")

    def save(self, file):
        raise NotImplementedError(".save isn't implemented for the approximate index")

    @classmethod
    def load(cls, file):
        raise NotImplementedError(".load isn't implemented for the approximate index")
