"""BayesianPersonalizedRanking on MI355X.

Public surface of implicit/gpu/bpr.py:15-160 (constructor, fit, to_cpu) plus save / load with the .npz keys of
implicit/cpu/bpr.pyx:228-244 (without num_threads).  Training runs one imp_bpr_update call per epoch (bpr_epoch,
csrc/bpr.hip) with the numerics of the reference's CPU update; fit and the initial factors come from PairwiseSGDBase
(pairwise.py), recommend / similar_* / save / load / pickling from MatrixFactorizationBase.  Factors are float32 only (the
reference's GPU class ignores `dtype` as well).
"""
import numpy as np

import implicit_amd.gpu as gpu

from .pairwise import PairwiseSGDBase


class BayesianPersonalizedRanking(PairwiseSGDBase):
    """Bayesian Personalized Ranking (Rendle et al., "BPR: Bayesian Personalized Ranking from Implicit Feedback").

    factors, learning_rate, regularization, iterations: as the reference.  verify_negative_samples: skip a sampled negative
    the user has liked (costs a search of the user's row per sample).  random_state: int, numpy RandomState / Generator or
    None -- seeds the initial factors and the per-epoch sample streams.  fit's `callback(epoch, elapsed, correct, skipped)`.
    """

    def __init__(self, factors=100, learning_rate=0.01, regularization=0.01, dtype=np.float32, iterations=100,
                 verify_negative_samples=True, random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        self.factors = factors
        self.learning_rate = learning_rate
        self.iterations = iterations
        self.regularization = regularization
        self.verify_negative_samples = verify_negative_samples
        self.random_state = random_state

    _log_name = "BPR"

    def _needs_sorted_indices(self):
        return self.verify_negative_samples

    def _epoch(self, userids, itemids, indptr, seed):
        return gpu.bpr_epoch(userids, itemids, indptr, self.user_factors, self.item_factors, self.learning_rate,
                             self.regularization, seed, self.verify_negative_samples)

    def _postfix(self, total, correct, skipped):
        if total and total != skipped:
            return {"train_auc": f"{100.0 * correct / (total - skipped):0.2f}%", "skipped": f"{100.0 * skipped / total:0.2f}%"}
        return None

    def to_cpu(self):
        """implicit/gpu/bpr.py:147-160: the same model as the reference's CPU class."""
        return self._cpu_twin("bpr", "BayesianPersonalizedRanking", factors=self.factors, learning_rate=self.learning_rate,
                              regularization=self.regularization, iterations=self.iterations,
                              verify_negative_samples=self.verify_negative_samples, random_state=self.random_state)

    # the .npz keys of implicit/cpu/bpr.pyx:228-244, without num_threads; `dtype` is written for the file's readers
    _npz_keys = ("regularization", "factors", "learning_rate", "verify_negative_samples", "iterations", "dtype", "random_state")
    _npz_stale = ("num_threads", "dtype")
    _npz_dtype = np.float32
