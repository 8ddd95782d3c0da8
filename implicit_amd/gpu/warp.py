"""WARP-loss matrix factorization on MI355X.

No reference counterpart: the loss is Weston, Bengio and Usunier, "WSABIE: Scaling Up To Large Vocabulary Image
Annotation" (IJCAI 2011).  Training runs one imp_warp_update call per epoch (warp_epoch, csrc/warp.hip, which states the
update); fit and the initial factors -- those of BayesianPersonalizedRanking bit for bit -- come from PairwiseSGDBase
(pairwise.py), recommend / similar_* / rank_items / save / load / pickling from MatrixFactorizationBase.  Factors are
float32 only.
"""
import numpy as np

import implicit_amd.gpu as gpu

from .pairwise import PairwiseSGDBase


class WARPMatrixFactorization(PairwiseSGDBase):
    """Matrix factorization under the WARP ranking loss.

    For every positive (user, item), up to `max_sampled` (1 .. 4096) items are drawn uniformly until one the user has not
    liked scores within a margin of 1 of the positive; the SGD step is weighted by a rank estimate taken from the number of
    draws that took, so mistakes near the top of the list weigh most.  factors, learning_rate, regularization, iterations:
    as BayesianPersonalizedRanking.  random_state: int, numpy RandomState / Generator or None -- seeds the initial factors
    and the per-epoch sample streams.  fit's `callback(epoch, elapsed, satisfied, trials)`: the samples that found no
    violating negative and the draws consumed.
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

    _log_name = "WARP"

    def _epoch(self, userids, itemids, indptr, seed):
        return gpu.warp_epoch(userids, itemids, indptr, self.user_factors, self.item_factors, self.learning_rate,
                              self.regularization, seed, self.max_sampled)

    def _postfix(self, total, satisfied, trials):
        return {"satisfied": f"{100.0 * satisfied / total:0.2f}%", "trials": f"{trials / total:0.2f}"} if total else None

    # the .npz keys of BayesianPersonalizedRanking, max_sampled in place of verify_negative_samples
    _npz_keys = ("regularization", "factors", "learning_rate", "max_sampled", "iterations", "dtype", "random_state")
    _npz_stale = ("dtype",)
    _npz_dtype = np.float32
