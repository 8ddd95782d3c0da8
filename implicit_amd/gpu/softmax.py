"""Sampled-softmax matrix factorization on MI355X.

No reference counterpart: the listwise loss of Wu et al., "On the Effectiveness of Sampled Softmax Loss for Item
Recommendation" (2022), with uniform negatives shared by a mini-batch.  Training runs one imp_softmax_update call per epoch
(softmax_epoch, csrc/softmax_mf.hip, which states the update); fit and the initial factors -- those of
BayesianPersonalizedRanking bit for bit -- come from PairwiseSGDBase (pairwise.py), recommend / similar_* / rank_items /
save / load / pickling from MatrixFactorizationBase.  Factors are float32 only.
"""
import numpy as np

import implicit_amd.gpu as gpu

from .pairwise import PairwiseSGDBase


class SampledSoftmaxMatrixFactorization(PairwiseSGDBase):
    """Matrix factorization under the sampled softmax loss.

    The positives of an epoch are taken in mini-batches of 64; every batch draws `negatives` items uniformly (a multiple of
    32 in 32 .. 256) and each of its rows takes one softmax step over its positive and those of the shared negatives its
    user has not liked.  factors, learning_rate, regularization, iterations: as BayesianPersonalizedRanking; the defaults
    of learning_rate and regularization are placeholders, not tuned on real data.  random_state: int, numpy RandomState /
    Generator or None -- seeds the initial factors and the per-epoch sample streams.  fit's `callback(epoch, elapsed,
    correct, masked)`: the rows whose positive outscored every unmasked negative, and the (row, negative) pairs left out
    because the user had liked the negative.
    """

    def __init__(self, factors=100, learning_rate=0.05, regularization=0.01, iterations=30, negatives=128, random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        if not 32 <= int(negatives) <= 256 or int(negatives) % 32:
            raise ValueError("negatives must be a multiple of 32 in 32 .. 256")
        self.factors = factors
        self.learning_rate = learning_rate
        self.iterations = iterations
        self.regularization = regularization
        self.negatives = int(negatives)
        self.random_state = random_state

    _log_name = "sampled softmax"

    def _epoch(self, userids, itemids, indptr, seed):
        return gpu.softmax_epoch(userids, itemids, indptr, self.user_factors, self.item_factors, self.learning_rate,
                                 self.regularization, seed, self.negatives)

    def _postfix(self, total, correct, masked):
        if not total:
            return None
        return {"correct": f"{100.0 * correct / total:0.2f}%", "masked": f"{100.0 * masked / (total * self.negatives):0.2f}%"}

    # the .npz keys of BayesianPersonalizedRanking, negatives in place of verify_negative_samples
    _npz_keys = ("regularization", "factors", "learning_rate", "negatives", "iterations", "dtype", "random_state")
    _npz_stale = ("dtype",)
    _npz_dtype = np.float32
