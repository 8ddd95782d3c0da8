"""Loading a model file in the reference's CPU format (MatrixFactorizationBase.load): the keys a GPU model does not have
(num_threads, use_native, dtype) are dropped, the hyper-parameters and the factors arrive, and save() of the loaded model
writes the documented key set."""
import io

import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

FACTORS = 4
SGD = dict(regularization=0.02, factors=FACTORS, learning_rate=0.03, iterations=7, dtype="float32", random_state=11)
# model: (module, class, extra factor columns, hyper-parameters on file, stale keys on file and their values, stored dtype)
CASES = {
    "als": ("als", "AlternatingLeastSquares", 0,
            dict(regularization=0.02, factors=FACTORS, iterations=7, use_cg=True, cg_steps=4, calculate_training_loss=True,
                 dtype="float32", random_state=11, alpha=2.5), dict(num_threads=8, use_native=True), np.float32),
    "bpr": ("bpr", "BayesianPersonalizedRanking", 1, dict(SGD, verify_negative_samples=False), dict(num_threads=8), np.float64),
    "warp": ("warp", "WARPMatrixFactorization", 1, dict(SGD, max_sampled=5), {}, np.float64),
    "lmf": ("lmf", "LogisticMatrixFactorization", 2, dict(SGD, neg_prop=9), dict(num_threads=8), np.float64),
}
# attributes load() must not leave behind: the stale keys on file, and `dtype` where it is no attribute of the model
GONE = {"als": ("num_threads", "use_native"), "bpr": ("num_threads", "dtype"), "warp": ("dtype",), "lmf": ("num_threads", "dtype")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_load_of_a_cpu_format_file_drops_stale_keys(name):
    import importlib

    import implicit_amd.gpu as gpu

    module, cls_name, extra, params, stale, dtype = CASES[name]
    cls = getattr(importlib.import_module(f"implicit_amd.gpu.{module}"), cls_name)
    rng = np.random.default_rng(3)
    user_factors = rng.standard_normal((5, FACTORS + extra)).astype(dtype)
    item_factors = rng.standard_normal((6, FACTORS + extra)).astype(dtype)
    f = io.BytesIO()
    np.savez(f, user_factors=user_factors, item_factors=item_factors, **params, **stale)
    f.seek(0)

    model = cls.load(f)
    for key in GONE[name]:
        assert not hasattr(model, key), key
    for key, value in params.items():
        if key != "dtype":
            assert getattr(model, key) == value and type(getattr(model, key)) is type(value), key
    if name == "als":
        assert model.dtype == np.dtype("float32")
    for got, want in ((model.user_factors, user_factors), (model.item_factors, item_factors)):
        assert isinstance(got, gpu.Matrix) and got.to_numpy().dtype == np.float32 and got.shape == want.shape
        assert_array_equal(got.to_numpy(), want.astype(np.float32))

    out = io.BytesIO()
    model.save(out)
    out.seek(0)
    with np.load(out, allow_pickle=False) as data:
        assert set(data.files) == {"user_factors", "item_factors"} | set(params)
        for key, value in params.items():
            assert data[key].item() == value, key
        assert data["user_factors"].dtype == np.float32
        assert_array_equal(data["user_factors"], user_factors.astype(np.float32))
        assert_array_equal(data["item_factors"], item_factors.astype(np.float32))
