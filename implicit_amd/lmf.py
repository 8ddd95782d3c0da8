"""Factory with the signature of implicit/lmf.py.  Only the GPU branch exists in this package (the reference has only the
CPU one): its CPU model is not part of the product."""
import numpy as np

import implicit_amd.gpu


def LogisticMatrixFactorization(factors=30, learning_rate=1.00, regularization=0.6, dtype=np.float32, iterations=30,
                                neg_prop=30, use_gpu=implicit_amd.gpu.HAS_CUDA, num_threads=0, random_state=None):
    """`dtype` and `num_threads` belong to the reference's CPU model and are ignored here (factors are float32)."""
    if not use_gpu:
        raise ValueError("implicit_amd only ships the MI355X (use_gpu=True) path; "
                         "use benfred/implicit for the CPU model")
    import implicit_amd.gpu.lmf

    return implicit_amd.gpu.lmf.LogisticMatrixFactorization(
        factors, learning_rate, regularization, iterations=iterations, neg_prop=neg_prop, random_state=random_state)
