"""Factory for WARP-loss matrix factorization, in the manner of implicit_amd/bpr.py.  Only the GPU branch exists in this
package (and the reference has no such model at all)."""
import implicit_amd.gpu


def WARPMatrixFactorization(factors=100, learning_rate=0.02, regularization=0.01, iterations=30, max_sampled=10,
                            use_gpu=implicit_amd.gpu.HAS_CUDA, random_state=None):
    if not use_gpu:
        raise ValueError("implicit_amd only ships the MI355X (use_gpu=True) path; there is no CPU WARP model")
    import implicit_amd.gpu.warp

    return implicit_amd.gpu.warp.WARPMatrixFactorization(
        factors, learning_rate, regularization, iterations=iterations, max_sampled=max_sampled, random_state=random_state)
