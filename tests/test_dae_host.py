"""Mult-DAE without a device: the restatement's gradients against central finite differences of its own loss, and the
factory's argument checks."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import dae_reference as ref


def test_restatement_gradients_are_the_derivatives_of_its_loss():
    rng = np.random.default_rng(0)
    m = csr_matrix((rng.random((6, 9)) < 0.4).astype(np.float32))
    rows = np.array([0, 1, 2, 3, 4, 5, -1, -1])
    params = [rng.standard_normal((9, 4)) * 0.5, rng.standard_normal((1, 4)) * 0.5, rng.standard_normal((9, 5)) * 0.5]
    got = ref.gradients(m, rows, *params, 0.5, 3)
    assert not ref.keep_mask(m, 3, 0.5).all() and ref.keep_mask(m, 3, 0.5).any()
    for i, name in enumerate(("dW_in", "db_in", "dW_out")):
        numeric = np.zeros_like(params[i])
        for at in np.ndindex(*params[i].shape):
            loss = []
            for eps in (1e-6, -1e-6):
                moved = [p.copy() for p in params]
                moved[i][at] += eps
                loss.append(ref.gradients(m, rows, *moved, 0.5, 3)["loss"])
            numeric[at] = (loss[0] - loss[1]) / 2e-6
        np.testing.assert_allclose(got[name], numeric, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("kw", [dict(hidden=48), dict(hidden=544), dict(hidden=0), dict(batch_size=96), dict(batch_size=0),
                                dict(use_gpu=False)])
def test_factory_argument_errors(kw):
    from implicit_amd.dae import MultDAE

    with pytest.raises(ValueError):
        MultDAE(**kw)
