"""WARP-loss factorization over user and item features on MI355X: the hybrid model of Kula, "Metadata Embeddings for User
and Item Cold-start Recommendations" (CBRecSys 2015), known from LightFM.  No reference counterpart.

A user is the weighted sum of the embeddings of its features, an item likewise, plus a bias per item feature.  Training runs
one imp_hybrid_warp_update call per epoch (hybrid_warp_epoch, csrc/hybrid_warp.hip, which states the update) on the two
embedding matrices; after the last epoch user_factors = user_features @ user_embeddings (with the 1.0 bias column) and
item_factors = item_features @ item_embeddings are materialised with implicit_amd.gpu.spmm, so recommend / similar_* /
rank_items / score_items, implicit_amd.evaluation and implicit_amd.ann.IVFModel work through MatrixFactorizationBase as for
any factor model.  represent_items / represent_users give factor rows for feature rows the model never saw: the cold-start
path.  Embeddings are float32 only.
"""
import logging
import time
import types

import numpy as np
from scipy.sparse import identity

import implicit_amd.gpu as gpu

from ..utils import check_csr, check_random_state
from .als import _progress
from .matrix_factorization_base import MatrixFactorizationBase
from .pairwise import initial_bias_factors

log = logging.getLogger("implicit_amd")


def _features(features, rows, what):
    """A feature matrix as float32 CSR with `rows` rows; None: the identity (every row its own single feature)."""
    if features is None:
        return identity(rows, dtype=np.float32, format="csr")
    features = check_csr(features)
    if features.dtype != np.float32:
        features = features.astype(np.float32)
    if features.shape[0] != rows:
        raise ValueError(f"{what} must have one row per {what.split('_')[0]}: {features.shape[0]} rows for {rows}")
    return features


class HybridWARP(MatrixFactorizationBase):
    """Hybrid matrix factorization under the WARP ranking loss.

    factors, learning_rate, regularization, iterations, max_sampled, random_state: as WARPMatrixFactorization.  fit's
    `callback(epoch, elapsed, satisfied, trials)`.  user_embeddings (user features x factors + 1) and item_embeddings (item
    features x factors + 1) are the trained parameters; the last column of item_embeddings holds the item feature biases,
    the last column of user_embeddings is never read or trained (a user's bias coordinate is 1.0 by definition).
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
        self.user_embeddings = None
        self.item_embeddings = None

    def fit(self, user_items, user_features=None, item_features=None, show_progress=True, callback=None):
        """Trains on a (users x items) CSR matrix of positives (values ignored) with (users x UF) and (items x IF) feature
        matrices; None is the identity, and with both None the model is WARPMatrixFactorization's."""
        rs = check_random_state(self.random_state)
        user_items = check_csr(user_items)
        if user_items.dtype != np.float32:
            user_items = user_items.astype(np.float32)
        if not user_items.has_sorted_indices:
            user_items = user_items.copy()  # the caller's matrix stays as it was
            user_items.sort_indices()
        users, items = user_items.shape
        user_features = _features(user_features, users, "user_features")
        item_features = _features(item_features, items, "item_features")
        indptr = np.ascontiguousarray(user_items.indptr, dtype=np.int32)
        itemids = np.ascontiguousarray(user_items.indices, dtype=np.int32)
        userids = np.repeat(np.arange(users, dtype=np.int32), np.ediff1d(indptr))

        # PairwiseSGDBase's initial factors over the feature axes: item features before user features, zero rows for features
        # no row carries
        init = types.SimpleNamespace(factors=self.factors, item_factors=self.item_embeddings, user_factors=self.user_embeddings)
        axes = types.SimpleNamespace(shape=(user_features.shape[1], item_features.shape[1]), indices=item_features.indices)
        initial_bias_factors(init, rs, axes, np.bincount(user_features.indices, minlength=user_features.shape[1]))
        self.user_embeddings, self.item_embeddings = init.user_factors, init.item_factors
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None

        d_ids = gpu.IntVector(userids), gpu.IntVector(itemids), gpu.IntVector(indptr)
        d_uf, d_if = gpu.CSRMatrix(user_features), gpu.CSRMatrix(item_features)
        total = len(itemids)
        log.debug("Running %i hybrid WARP training epochs", self.iterations)
        progress = _progress(self.iterations, show_progress)
        for epoch in range(self.iterations):
            t0 = time.time()
            satisfied, trials = gpu.hybrid_warp_epoch(*d_ids, d_uf, d_if, self.user_embeddings, self.item_embeddings,
                                                      self.learning_rate, self.regularization, rs.integers(2**31), self.max_sampled)
            progress.update(None)
            if progress.bar is not None and total:
                progress.bar.set_postfix({"satisfied": f"{100.0 * satisfied / total:0.2f}%", "trials": f"{trials / total:0.2f}"})
            if callback:
                callback(epoch, time.time() - t0, satisfied, trials)
        progress.close()
        self.user_factors = self._represent(d_uf, self.user_embeddings, user_bias=True)
        self.item_factors = self._represent(d_if, self.item_embeddings, user_bias=False)
        self._check_fit_errors()

    @staticmethod
    def _represent(features, embeddings, user_bias):
        out = gpu.spmm(features, embeddings)
        if user_bias:  # a user's last coordinate is 1.0 by definition, whatever its features sum to
            host = out.to_numpy()
            host[:, -1] = 1.0
            out = gpu.Matrix(host)
        return out

    def represent_items(self, item_features):
        """Factor rows (a device Matrix, rows x factors + 1) for the rows of an (any x IF) item feature matrix -- items the
        model never saw included; they score against user_factors like rows of item_factors."""
        return self._represent_rows(item_features, self.item_embeddings, "item_features", False)

    def represent_users(self, user_features):
        """The same for the rows of an (any x UF) user feature matrix, against item_factors."""
        return self._represent_rows(user_features, self.user_embeddings, "user_features", True)

    def _represent_rows(self, features, embeddings, what, user_bias):
        if embeddings is None:
            raise ValueError("the model is not fitted")
        features = _features(features, features.shape[0], what)
        if features.shape[1] != embeddings.shape[0]:
            raise ValueError(f"{what} has {features.shape[1]} columns, the model has {embeddings.shape[0]} features")
        return self._represent(gpu.CSRMatrix(features), embeddings, user_bias)

    @property
    def user_feature_biases(self):
        """The last column of user_embeddings (host array): part of the layout only, never read or trained."""
        return self.user_embeddings.to_numpy()[:, -1]

    @property
    def item_feature_biases(self):
        """The bias of every item feature (host array): an item's bias is the weighted sum over its features."""
        return self.item_embeddings.to_numpy()[:, -1]

    # ---- persistence: the factor models' .npz plus the two embedding matrices ---------------------------------------------
    _npz_keys = ("regularization", "factors", "learning_rate", "max_sampled", "iterations", "dtype", "random_state")
    _npz_stale = ("dtype",)
    _npz_dtype = np.float32
    _embedding_names = ("user_embeddings", "item_embeddings")

    def save(self, fileobj_or_path):
        """user_factors / item_factors and the hyper-parameters as the other factor models store them, plus user_embeddings
        and item_embeddings."""
        args = {"user_factors": self.user_factors, "item_factors": self.item_factors,
                "user_embeddings": self.user_embeddings, "item_embeddings": self.item_embeddings}
        args = {k: v.to_numpy() for k, v in args.items() if v is not None}
        for key in self._npz_keys:
            args[key] = getattr(self, key, None)
        args["dtype"] = "float32"
        if not isinstance(self.random_state, (int, np.integer)):
            args["random_state"] = None
        np.savez(fileobj_or_path, **{k: v for k, v in args.items() if v is not None})

    @classmethod
    def load(cls, fileobj_or_path):
        model = super().load(fileobj_or_path)
        for name in cls._embedding_names:
            if isinstance(getattr(model, name, None), np.ndarray):
                setattr(model, name, gpu.Matrix(np.ascontiguousarray(getattr(model, name), dtype=np.float32)))
        return model

    def __getstate__(self):
        state = super().__getstate__()
        for name in self._embedding_names:
            state[name] = None if state[name] is None else state[name].to_numpy()
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        for name in self._embedding_names:
            if getattr(self, name) is not None:
                setattr(self, name, gpu.Matrix(getattr(self, name)))
