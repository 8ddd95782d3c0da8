"""Factory for the Mult-VAE autoencoder, in the manner of implicit_amd/dae.py.  Only the GPU branch exists in this package
(and the reference has no such model at all), so there is no to_cpu either."""
import implicit_amd.gpu


def MultVAE(hidden=256, latent=64, dropout=0.5, anneal_cap=0.2, anneal_steps=None, learning_rate=1e-3, regularization=0.0,
            batch_size=512, iterations=20, beta1=0.9, beta2=0.999, eps=1e-8, use_gpu=implicit_amd.gpu.HAS_CUDA, random_state=None):
    if not use_gpu:
        raise ValueError("implicit_amd only ships the MI355X (use_gpu=True) path; there is no CPU Mult-VAE model")
    if not 32 <= int(hidden) <= 512 or int(hidden) % 32:
        raise ValueError("hidden must be a multiple of 32 in 32 .. 512")
    if not 32 <= int(latent) <= 256 or int(latent) % 32:
        raise ValueError("latent must be a multiple of 32 in 32 .. 256")
    if int(batch_size) < 64 or int(batch_size) % 64:
        raise ValueError("batch_size must be a multiple of 64")
    if not anneal_cap >= 0 or (anneal_steps is not None and int(anneal_steps) < 1):
        raise ValueError("anneal_cap must not be negative and anneal_steps at least 1")
    import implicit_amd.gpu.vae

    return implicit_amd.gpu.vae.MultVAE(hidden, latent, dropout, anneal_cap, anneal_steps, learning_rate, regularization, batch_size,
                                        iterations, beta1, beta2, eps, random_state=random_state)
