"""CPU-side checks of the WARP feature: the host restatement's streams and weight (what the GPU tests predict samples
with), the factory's surface, and an import without a device."""
import inspect
import math
import warnings

import numpy as np
import pytest

import bpr_reference
import warp_reference as ref


def test_positions_in_range_and_spread():
    lp = ref.positions(12345, 1000, 200_000)
    assert lp.min() >= 0 and lp.max() < 1000
    counts = np.bincount(lp, minlength=1000)
    assert counts.min() > 100 and counts.max() < 300  # uniform: 200 per position
    assert not np.array_equal(lp[:1000], ref.positions(12346, 1000, 1000))
    # a later window of the same call continues the stream
    assert np.array_equal(ref.positions(12345, 1000, 50, first=100), lp[100:150])


def test_candidates_in_range_and_spread():
    items = 37
    c = np.concatenate([ref.candidates(99, s, items, 10) for s in range(4000)])
    assert c.min() >= 0 and c.max() < items
    counts = np.bincount(c, minlength=items)
    assert counts.min() > 0.8 * len(c) / items and counts.max() < 1.2 * len(c) / items  # uniform over the items
    # a shorter chain is a prefix of a longer one; the second Philox block (trials 5 ..) is not a repeat of the first
    long = ref.candidates(99, 5, 10**6, 12)
    assert np.array_equal(ref.candidates(99, 5, 10**6, 6), long[:6])
    assert not np.array_equal(long[:4], long[4:8]) and not np.array_equal(long[4:8], long[8:12])
    assert not np.array_equal(ref.candidates(99, 6, 10**6, 12), long)
    assert not np.array_equal(ref.candidates(98, 5, 10**6, 12), long)


def test_stream_differs_from_bpr():
    lp_bpr, _ = bpr_reference.sample_positions(777, 10**6, 1000)
    lp = ref.positions(777, 10**6, 1000)
    assert (lp != lp_bpr).mean() > 0.99


def test_positives_are_nonzeros():
    from scipy.sparse import csr_matrix

    rng = np.random.default_rng(0)
    m = csr_matrix((rng.random((30, 20)) < 0.2).astype(np.float32))
    u, i = ref.positives(m, 5, 500)
    assert (np.asarray(m[u, i]).ravel() == 1.0).all()
    assert len(set(zip(u.tolist(), i.tolist()))) > 0.5 * m.nnz


def test_weight():
    assert ref.weight(200, 1) == math.log(199)
    assert ref.weight(200, 2) == math.log(99)
    assert ref.weight(200, 199) == 0.0 and ref.weight(200, 4096) == 0.0
    assert ref.weight(10**6, 1) == 10.0  # log(999999) = 13.8: the cap
    assert ref.weight(22027, 1) < 10.0 <= ref.weight(22028, 1)  # e^10 = 22026.47


def test_step64_counts_trials():
    X = np.array([[0.5, 1.0]])
    Y = np.array([[1.0, 0.0], [9.0, 0.0], [-9.0, 0.0], [0.9, 0.0]])
    # liked candidate, then a far-below one, then the violating one (0.45 > 0.5 - 1)
    Xc, Yc = X.copy(), Y.copy()
    t, trials, closest = ref.step64(Xc, Yc, {0, 1}, 0, 0, np.array([1, 2, 3, 2]), 0.1, 0.0)
    assert (t, trials) == (3, 3) and closest == pytest.approx(0.95)
    L = ref.weight(4, 3)
    assert L == 0.0 and np.array_equal(Xc, X) and np.array_equal(Yc, Y)  # reg 0, weight 0: an update that changes nothing
    t, trials, closest = ref.step64(Xc, Yc, {0, 1}, 0, 0, np.array([1, 2, 2]), 0.1, 0.0)
    assert (t, trials) == (None, 3) and closest == pytest.approx(4.0)
    t, trials, closest = ref.step64(Xc, Yc, {0, 1}, 0, 0, np.array([1, 1]), 0.1, 0.0)
    assert (t, trials, closest) == (None, 2, math.inf)
    # a first-trial violation on a larger catalogue moves the three rows and the two biases
    Y2 = np.vstack([Y, np.zeros((96, 2))])
    t, trials, _ = ref.step64(Xc, Y2, {0}, 0, 0, np.array([3]), 0.1, 0.0)
    L = math.log(99)
    assert (t, trials) == (1, 1)
    assert Xc[0, 0] == pytest.approx(0.5 + 0.1 * L * (1.0 - 0.9)) and Xc[0, 1] == 1.0
    assert Y2[0].tolist() == pytest.approx([1.0 + 0.1 * L * 0.5, 0.1 * L])
    assert Y2[3].tolist() == pytest.approx([0.9 - 0.1 * L * 0.5, -0.1 * L])


def test_factory_signature():
    import implicit_amd.warp

    params = inspect.signature(implicit_amd.warp.WARPMatrixFactorization).parameters
    assert list(params) == ["factors", "learning_rate", "regularization", "iterations", "max_sampled", "use_gpu", "random_state"]
    defaults = {"factors": 100, "learning_rate": 0.02, "regularization": 0.01, "iterations": 30, "max_sampled": 10,
                "random_state": None}
    for name, value in defaults.items():
        assert params[name].default == value, name


def test_model_constructor_signature():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu.warp

    params = inspect.signature(implicit_amd.gpu.warp.WARPMatrixFactorization).parameters
    assert list(params) == ["factors", "learning_rate", "regularization", "iterations", "max_sampled", "random_state"]
    assert [params[n].default for n in params] == [100, 0.02, 0.01, 30, 10, None]


def test_factory_cpu_branch_raises():
    import implicit_amd.warp

    with pytest.raises(ValueError):
        implicit_amd.warp.WARPMatrixFactorization(use_gpu=False)


def test_gpu_warp_module_imports_without_device():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.warp  # noqa: F401
        import implicit_amd.gpu as g
        import implicit_amd.gpu.warp as w
        from implicit_amd.gpu.matrix_factorization_base import MatrixFactorizationBase

    assert callable(g.warp_epoch) and issubclass(w.WARPMatrixFactorization, MatrixFactorizationBase)
    assert not hasattr(w.WARPMatrixFactorization, "to_cpu")  # no CPU counterpart to return
    assert w.WARPMatrixFactorization.recalculate_user is MatrixFactorizationBase.recalculate_user  # the base's: it raises