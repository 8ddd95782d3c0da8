"""Factory with the signature of implicit/bpr.py:8-72.  Only the GPU branch exists in this package: the reference's CPU
model is not part of the product."""
import numpy as np

import implicit_amd.gpu


def BayesianPersonalizedRanking(factors=100, learning_rate=0.01, regularization=0.01, dtype=np.float32, iterations=100,
                                use_gpu=implicit_amd.gpu.HAS_CUDA, num_threads=0, verify_negative_samples=True,
                                random_state=None):
    """`dtype` and `num_threads` belong to the reference's CPU model and are ignored here (factors are float32)."""
    if not use_gpu:
        raise ValueError("implicit_amd only ships the MI355X (use_gpu=True) path; "
                         "use benfred/implicit for the CPU model")
    import implicit_amd.gpu.bpr

    return implicit_amd.gpu.bpr.BayesianPersonalizedRanking(
        factors, learning_rate, regularization, iterations=iterations, verify_negative_samples=verify_negative_samples,
        random_state=random_state)
