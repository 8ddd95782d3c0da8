"""Mult-VAE without a device: the restatement's gradients against central finite differences of its own NLL + beta KL, and
the factory's argument checks."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import vae_reference as ref


def test_restatement_gradients_are_the_derivatives_of_its_loss():
    rng = np.random.default_rng(0)
    m = csr_matrix((rng.random((6, 9)) < 0.4).astype(np.float32))
    rows = np.array([0, 1, 2, 3, 4, 5, -1, -1])
    H, L, beta = 4, 3, 0.2
    shapes = [(9, H), (1, H), (H, 2 * L), (1, 2 * L), (L, H), (1, H), (9, H + 1)]
    params = [rng.standard_normal(s) * 0.5 for s in shapes]
    eps = rng.standard_normal((len(rows), L))

    def loss(p):
        out = ref.gradients(m, rows, p, 0.5, 3, beta, eps)
        return out["nll"] + beta * out["kl"]

    got = ref.gradients(m, rows, params, 0.5, 3, beta, eps)
    for i, name in enumerate(ref.NAMES):
        numeric = np.zeros_like(params[i])
        for at in np.ndindex(*params[i].shape):
            moved = [[p.copy() for p in params] for _ in range(2)]
            moved[0][i][at] += 1e-6
            moved[1][i][at] -= 1e-6
            numeric[at] = (loss(moved[0]) - loss(moved[1])) / 2e-6
        np.testing.assert_allclose(got[name], numeric, rtol=1e-6, atol=1e-8, err_msg=name)


def test_serving_inputs_have_no_near_tie_at_the_cut():
    assert min(gap for _, _, gap, _ in ref.serving_case()[1]) >= 1e-4


@pytest.mark.parametrize("kw", [dict(hidden=48), dict(hidden=544), dict(latent=16), dict(latent=288), dict(latent=80),
                                dict(batch_size=96), dict(anneal_cap=-0.1), dict(anneal_steps=0), dict(use_gpu=False)])
def test_factory_argument_errors(kw):
    from implicit_amd.vae import MultVAE

    with pytest.raises(ValueError):
        MultVAE(**kw)
