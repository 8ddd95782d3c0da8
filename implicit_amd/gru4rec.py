"""Factory for the GRU4Rec session model, in the manner of implicit_amd/dae.py.  Only the GPU branch exists in this package
(and the reference has no such model at all), so there is no to_cpu either."""
import implicit_amd.gpu


def GRU4Rec(hidden=128, loss="bpr-max", n_sample=2048, sample_alpha=0.75, bpreg=1.0, learning_rate=0.1, batch_size=64, iterations=10,
            steps_per_call=64, use_gpu=implicit_amd.gpu.HAS_CUDA, random_state=None):
    if not use_gpu:
        raise ValueError("implicit_amd only ships the MI355X (use_gpu=True) path; there is no CPU GRU4Rec model")
    import implicit_amd.gpu.gru4rec

    return implicit_amd.gpu.gru4rec.GRU4Rec(hidden, loss, n_sample, sample_alpha, bpreg, learning_rate, batch_size, iterations,
                                            steps_per_call, random_state=random_state)
