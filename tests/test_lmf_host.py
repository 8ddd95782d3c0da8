"""CPU-side checks of the LMF feature: the Philox negative positions and K formula the GPU tests predict with, the float64
restatement against the reference's own lmf_update (tests/golden/lmf_golden.npz), the factory's surface, and an import
without a device."""
import inspect
import os
import warnings

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import lmf_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lmf_golden.npz")


def _golden_csr(g, name):
    return csr_matrix((g[name + "_data"], g[name + "_indices"], g[name + "_indptr"]), shape=tuple(g[name + "_shape"]))


def test_negative_positions_in_range_and_uniform():
    rows = np.repeat(np.arange(2000), 100)
    ks = np.tile(np.arange(100), 2000)
    pos = ref.negative_positions(12345, 1000, rows, ks)
    assert pos.min() >= 0 and pos.max() < 1000
    counts = np.bincount(pos, minlength=1000)
    assert counts.min() > 120 and counts.max() < 290  # 200 per position
    assert not np.array_equal(pos, ref.negative_positions(12346, 1000, rows, ks))
    # words 0..3 of one Philox block serve negatives 4q .. 4q + 3 of a row: neighbouring negatives differ
    assert (pos[:-1] != pos[1:]).mean() > 0.99


def test_negative_positions_use_tag_3():
    from bpr_reference import philox4x32_10

    r = philox4x32_10(1, 7, 0, 3, 99, 0)
    want = [(int(w) * 5000) >> 32 for w in r]
    assert ref.negative_positions(99, 5000, [7] * 4, [4, 5, 6, 7]).tolist() == want


def test_negative_count_formula():
    n = np.array([0, 1, 5, 20])
    assert ref.negative_count(n, 7, 1).tolist() == [0, 1, 5, 7]
    assert ref.negative_count(n, 7, 2).tolist() == [0, 2, 7, 7]
    assert ref.negative_count(n, 7, 30).tolist() == [0, 7, 7, 7]
    assert ref.negative_count(n, 7, 0).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["np0_c5", "np0_c32", "np0_c66"])
def test_restatement_matches_reference_neg_prop_0(name):
    g = np.load(GOLDEN)
    m = _golden_csr(g, name)
    X, Y = g[name + "_X0"], g[name + "_Y"]
    G = np.zeros_like(X)
    empty = np.diff(m.indptr) == 0
    assert empty.any() and not np.all(m.data == 1)
    for step in (1, 2):  # the second call starts from the reference's fp32 output of the first
        X1, G1, bX, bG = ref.half_sweep64(m, X, Y, G, float(g[name + "_lr"]), float(g[name + "_reg"]), 0, 0)
        ok, worst = ref.within(g[f"{name}_X{step}"], X1, bX)
        assert ok, (step, worst)
        ok, worst = ref.within(g[f"{name}_G{step}"], G1, bG)
        assert ok, (step, worst)
        X, G = g[f"{name}_X{step}"], g[f"{name}_G{step}"]
        assert np.array_equal(X[empty], g[name + "_X0"][empty]) and not G[empty].any()


@pytest.mark.parametrize("neg_prop", [1, 2, 30])
def test_restatement_matches_reference_negative_count(neg_prop):
    g = np.load(GOLDEN)
    m = _golden_csr(g, "kprobe")
    C = int(g["kprobe_C"])
    X, Y, G = np.zeros((3, C), np.float32), np.ones((30, C), np.float32), np.zeros((3, C), np.float32)
    _, G1, _, _ = ref.half_sweep64(m, X, Y, G, 1.0, 0.0, neg_prop, 5)
    K = ref.negative_count(np.diff(m.indptr), C, neg_prop)
    np.testing.assert_array_equal(g[f"kprobe_G_np{neg_prop}"], np.repeat((K / 2.0) ** 2, C).reshape(3, C))
    np.testing.assert_allclose(G1, g[f"kprobe_G_np{neg_prop}"], rtol=1e-12)


def test_init_factors_follow_reference_layout():
    m = csr_matrix(np.array([[1, 0, 1], [0, 0, 0], [0, 0, 1]], dtype=np.float32))
    X, Y, _ = ref.init_factors(m, 4, 3)
    assert X.shape == (3, 6) and Y.shape == (3, 6) and X.dtype == Y.dtype == np.float32
    assert (X[[0, 2], -2] == 1).all() and not X[1].any()
    assert (Y[[0, 2], -1] == 1).all() and not Y[1].any()
    rs = np.random.default_rng(3)
    assert np.array_equal(Y[0, :-1], rs.standard_normal(size=(3, 6), dtype=np.float32)[0, :-1])


def test_factory_signature_matches_reference():
    import implicit_amd.lmf

    params = inspect.signature(implicit_amd.lmf.LogisticMatrixFactorization).parameters
    names = ["factors", "learning_rate", "regularization", "dtype", "iterations", "neg_prop", "use_gpu", "num_threads",
             "random_state"]
    assert list(params) == names
    defaults = {"factors": 30, "learning_rate": 1.0, "regularization": 0.6, "dtype": np.float32, "iterations": 30,
                "neg_prop": 30, "num_threads": 0, "random_state": None}
    for name, value in defaults.items():
        assert params[name].default == value, name


def test_model_constructor_signature_matches_reference():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu.lmf

    params = inspect.signature(implicit_amd.gpu.lmf.LogisticMatrixFactorization).parameters
    assert list(params) == ["factors", "learning_rate", "regularization", "dtype", "iterations", "neg_prop", "random_state"]
    assert [params[n].default for n in params] == [30, 1.0, 0.6, np.float32, 30, 30, None]


def test_factory_cpu_branch_raises():
    import implicit_amd.lmf

    with pytest.raises(ValueError):
        implicit_amd.lmf.LogisticMatrixFactorization(use_gpu=False)


def test_gpu_lmf_module_imports_without_device():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as g
        import implicit_amd.gpu.lmf as lm
        import implicit_amd.lmf  # noqa: F401

    assert callable(g.lmf_update) and issubclass(lm.LogisticMatrixFactorization, lm.MatrixFactorizationBase)
