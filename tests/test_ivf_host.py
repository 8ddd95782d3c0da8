"""CPU-side checks of the IVF-Flat feature: the float64 restatement the GPU tests compare against is itself right (full probe
equals brute force, the lists are a partition), and the model-layer modules import on a box without a device."""
import warnings

import numpy as np

import ivf_reference as ref


def _case(n=600, f=16, nlist=12, seed=3):
    rng = np.random.default_rng(seed)
    vectors = rng.standard_normal((n, f)).astype(np.float32)
    init = rng.choice(n, size=nlist, replace=False)
    cent, assign = ref.kmeans(vectors, init, 4)
    offsets, ids = ref.build_lists(assign, nlist)
    return vectors, cent, assign, offsets, ids, rng


def test_reference_full_probe_equals_brute_force():
    vectors, cent, _, offsets, ids, rng = _case()
    queries = rng.standard_normal((40, 16)).astype(np.float32)
    probes, got_ids, got_scores = ref.search(cent, offsets, ids, vectors, queries, 25, len(cent))
    want_ids, want_scores = ref.brute_force(vectors, queries, 25)
    assert probes.shape == (40, len(cent))
    assert (np.sort(probes, axis=1) == np.arange(len(cent))).all()
    np.testing.assert_array_equal(got_ids, want_ids)
    np.testing.assert_array_equal(got_scores, want_scores)
    # best first under (score desc, id desc)
    assert (np.diff(got_scores, axis=1) <= 0).all()


def test_reference_lists_are_a_partition():
    vectors, cent, assign, offsets, ids, _ = _case()
    assert offsets[0] == 0 and offsets[-1] == len(vectors) and (np.diff(offsets) >= 0).all()
    np.testing.assert_array_equal(np.sort(ids), np.arange(len(vectors)))
    for l in range(len(cent)):
        members = ids[offsets[l]:offsets[l + 1]]
        assert (np.diff(members) > 0).all()
        assert (assign[members] == l).all()
    norms = np.linalg.norm(cent, axis=1)
    assert np.allclose(norms[norms > 0], 1.0)


def test_reference_tie_rules():
    # ties go to the larger id, in the assignment and in the search
    scores = np.array([[1.0, 3.0, 3.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(ref.argmax_rows(scores), [2, 3])
    np.testing.assert_array_equal(ref.order_desc([2.0, 5.0, 5.0, 1.0]), [2, 1, 0, 3])
    got_ids, got_scores = ref.topk_candidates([1.0, 1.0], [7, 9], 4)
    np.testing.assert_array_equal(got_ids, [9, 7, -1, -1])
    assert got_scores[2] == -np.finfo(np.float32).max
    # a zero initial row stays zero until its list gives it a mean; the zero vector ties and goes to the larger list
    vectors = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [1.0, 0.0]])
    cent, assign = ref.kmeans(vectors, [2, 0], 0)
    np.testing.assert_array_equal(cent, [[0.0, 0.0], [1.0, 0.0]])
    np.testing.assert_array_equal(assign, [1, 0, 1, 1])
    cent, assign = ref.kmeans(vectors, [2, 0], 2)
    np.testing.assert_array_equal(cent, [[-1.0, 0.0], [1.0, 0.0]])
    np.testing.assert_array_equal(assign, [1, 0, 1, 1])
    # an empty list keeps its centroid (both start equal, every vector ties and goes to list 1)
    cent, assign = ref.kmeans(np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]]), [2, 2], 3)
    np.testing.assert_array_equal(cent, [[0.0, 1.0], [0.0, 1.0]])
    np.testing.assert_array_equal(assign, [1, 1, 1])
    # a zero mean keeps its centroid
    cent, assign = ref.kmeans(np.array([[1.0, 0.0], [-1.0, 0.0]]), [0], 3)
    np.testing.assert_array_equal(cent, [[1.0, 0.0]])
    assert not np.isnan(cent).any()


def test_ann_modules_import_without_a_device():
    """The import contract tests/test_abi.py pins for the package: importing succeeds, constructing a model raises."""
    import pytest

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as g
        import implicit_amd.ann as ann
        import implicit_amd.approximate_als as approximate_als
    assert ann.IVFModel is not None
    assert approximate_als.FaissAlternatingLeastSquares is approximate_als.IVFAlternatingLeastSquares
    assert not hasattr(approximate_als, "AnnoyAlternatingLeastSquares")
    assert not hasattr(approximate_als, "NMSLibAlternatingLeastSquares")
    with pytest.raises(ValueError):
        approximate_als.IVFAlternatingLeastSquares(factors=8, use_gpu=False)
    if not g.HAS_CUDA:
        with pytest.raises(ValueError):
            approximate_als.IVFAlternatingLeastSquares(factors=8)
