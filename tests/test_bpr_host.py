"""CPU-side checks of the BPR feature: the host Philox restatement the GPU tests predict samples with, the factory's surface,
and an import without a device."""
import inspect
import warnings

import numpy as np
import pytest

from bpr_reference import philox4x32_10, predicted_skipped, sample_positions


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = philox4x32_10(*counter, *key)
    assert tuple(int(v) for v in got) == want


def test_sample_positions_in_range_and_spread():
    lp, dp = sample_positions(12345, 1000, 200_000)
    assert lp.min() >= 0 and lp.max() < 1000 and dp.min() >= 0 and dp.max() < 1000
    counts = np.bincount(lp, minlength=1000)
    assert counts.min() > 100 and counts.max() < 300  # uniform: 200 per position
    assert not np.array_equal(lp, dp)
    lp2, _ = sample_positions(12346, 1000, 1000)
    assert not np.array_equal(lp[:1000], lp2)


def test_predicted_skipped_counts_liked_negatives():
    from scipy.sparse import csr_matrix

    full = csr_matrix(np.ones((4, 3), dtype=np.float32))  # every negative is liked
    assert predicted_skipped(full, 7, True) == full.nnz
    assert predicted_skipped(full, 7, False) == 0


def test_factory_signature_matches_reference():
    import implicit_amd.bpr

    params = inspect.signature(implicit_amd.bpr.BayesianPersonalizedRanking).parameters
    names = ["factors", "learning_rate", "regularization", "dtype", "iterations", "use_gpu", "num_threads",
             "verify_negative_samples", "random_state"]
    assert list(params) == names
    defaults = {"factors": 100, "learning_rate": 0.01, "regularization": 0.01, "dtype": np.float32, "iterations": 100,
                "num_threads": 0, "verify_negative_samples": True, "random_state": None}
    for name, value in defaults.items():
        assert params[name].default == value, name


def test_model_constructor_signature_matches_reference():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu.bpr

    params = inspect.signature(implicit_amd.gpu.bpr.BayesianPersonalizedRanking).parameters
    assert list(params) == ["factors", "learning_rate", "regularization", "dtype", "iterations", "verify_negative_samples",
                            "random_state"]
    assert [params[n].default for n in params] == [100, 0.01, 0.01, np.float32, 100, True, None]


def test_factory_cpu_branch_raises():
    import implicit_amd.bpr

    with pytest.raises(ValueError):
        implicit_amd.bpr.BayesianPersonalizedRanking(use_gpu=False)


def test_gpu_bpr_module_imports_without_device():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.bpr  # noqa: F401
        import implicit_amd.gpu as g
        import implicit_amd.gpu.bpr as b
        from implicit_amd.gpu.matrix_factorization_base import MatrixFactorizationBase

    assert callable(g.bpr_epoch) and issubclass(b.BayesianPersonalizedRanking, MatrixFactorizationBase)
