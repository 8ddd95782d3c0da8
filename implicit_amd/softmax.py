"""Factory for sampled-softmax matrix factorization, in the manner of implicit_amd/warp.py.  Only the GPU branch exists in
this package (and the reference has no such model at all)."""
import implicit_amd.gpu


def SampledSoftmaxMatrixFactorization(factors=100, learning_rate=0.05, regularization=0.01, iterations=30, negatives=128,
                                      use_gpu=implicit_amd.gpu.HAS_CUDA, random_state=None):
    if not use_gpu:
        raise ValueError("implicit_amd only ships the MI355X (use_gpu=True) path; there is no CPU sampled-softmax model")
    import implicit_amd.gpu.softmax

    return implicit_amd.gpu.softmax.SampledSoftmaxMatrixFactorization(
        factors, learning_rate, regularization, iterations=iterations, negatives=negatives, random_state=random_state)
