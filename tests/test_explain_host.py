"""explain / explain_batch without a GPU: the float64 restatement (tests/explain_reference.py) reproduces what the reference's
CPU model recorded in tests/golden/explain_golden.npz, obeys the identities that make the feature checkable, and its float32
twin says how much of the GPU tests' 1e-4 bar plain single precision uses up on the very inputs those tests run."""
import json
import os

import numpy as np
import pytest

import explain_cases as cases
import explain_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explain_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def golden_row(g, case):
    k, u = case["model"], case["user"]
    lo, hi = g[f"m{k}_indptr"][u], g[f"m{k}_indptr"][u + 1]
    reg, alpha = g[f"m{k}_params"]
    return g[f"m{k}_Y"], g[f"m{k}_indices"][lo:hi], g[f"m{k}_data"][lo:hi].astype(np.float64) * alpha, reg


def test_restatement_reproduces_the_reference(golden):
    assert len(golden["cases"]) >= 10
    for i, text in enumerate(golden["cases"]):
        case = json.loads(str(text))
        Y, indices, data, reg = golden_row(golden, case)
        total, ids, scores, _ = ref.explain(Y, indices, data, case["item"], reg)
        want_ids, want_scores = golden[f"c{i}_ids"], golden[f"c{i}_scores"]
        n = len(want_ids)
        assert n == min(case["N"], int((data > 0).sum())), case
        np.testing.assert_array_equal(ids[:n], want_ids, err_msg=str(case))
        np.testing.assert_allclose(scores[:n], want_scores, rtol=0, atol=1e-6, err_msg=str(case))
        assert abs(total - float(golden[f"c{i}_total"])) <= 1e-6, case


def test_total_is_the_recalculated_users_score(golden):
    """total = y_i . x_u with x_u from a float64 solve of the normal equations, and = the sum of the contributions."""
    for text in golden["cases"]:
        case = json.loads(str(text))
        Y, indices, data, reg = golden_row(golden, case)
        A = ref.normal_matrix(Y, indices, data, reg)
        b = (Y[indices].astype(np.float64) * np.maximum(data, 0)[:, None]).sum(axis=0)
        x = np.linalg.solve(A, b)
        total, _, scores, _ = ref.explain(Y, indices, data, case["item"], reg)
        assert abs(total - Y[case["item"]].astype(np.float64) @ x) <= 1e-12 * max(1.0, np.abs(scores).sum()), case
        assert abs(total - scores.sum()) <= 1e-12 * max(1.0, np.abs(scores).sum()), case


def test_negative_confidences_are_absent_from_the_list_but_present_in_A():
    Y = cases.factors(16)
    indices, data = np.array([3, 9, 77, 120]), np.array([2.0, -3.0, 4.0, -1.5])
    total, ids, scores, L = ref.explain(Y, indices, data, 5, cases.REG)
    assert sorted(ids.tolist()) == [3, 77]
    np.testing.assert_allclose(L @ L.T, ref.normal_matrix(Y, indices, np.abs(data), cases.REG), rtol=0, atol=1e-12)
    _, _, without, _ = ref.explain(Y, indices[[0, 2]], data[[0, 2]], 5, cases.REG)  # dropping them from A changes the scores
    assert np.abs(np.sort(scores) - np.sort(without)).max() > 1e-6 * np.abs(scores).max()
    total, ids, scores, _ = ref.explain(Y, indices, -np.abs(data), 5, cases.REG)
    assert total == 0 and len(ids) == 0 and len(scores) == 0


def test_tie_rule():
    """Equal scores: the larger id first (the order of the reference's (score, itemid) heap)."""
    Y = cases.factors(16, cases.EDGE_ITEMS)
    lo, hi = cases.TIE
    np.testing.assert_array_equal(Y[lo], Y[hi])
    _, ids, scores, _ = ref.explain(Y, np.array([2, lo, 400, hi, 1999]), np.array([1.5, 3.0, 2.0, 3.0, 4.5]), 7, cases.REG)
    at = ids.tolist().index(hi)
    assert ids[at + 1] == lo and scores[at] == scores[at + 1]
    np.testing.assert_array_equal(ref.order([4, 9, 1, 9], [0.5, 0.25, 0.5, 0.75]), [3, 0, 2, 1])


@pytest.mark.parametrize("f,alpha", cases.ACCURACY)
def test_float32_twin_leaves_a_4x_margin(f, alpha):
    """Plain float32 arithmetic on the GPU tests' inputs stays within 2.5e-5 under both of their measures (their bar is 1e-4)
    and changes no top-10 id position.  Measured with numpy (LAPACK float32 factor and solves) over the seven settings:
    worst contribution error 1.7e-5 of max |s| (f = 256), worst total error 1.8e-5 of sum |s| (f = 256), 0 of 19 614 top-10
    id positions differ."""
    r64, r32 = cases.accuracy_reference(f, alpha), cases.accuracy_reference(f, alpha, np.float32)
    got = ref.compare(r32[0], r32[1], r32[2], r64[0], r64[1], r64[2], r64[3])
    print(f, alpha, got)
    assert got["contribution"] <= 2.5e-5 and got["total"] <= 2.5e-5
    assert got["differing"] == 0 and got["positions"] > 2500


def test_float32_twin_on_the_edge_batch():
    for f in (16, 256):
        r64, r32 = cases.edge_reference(f, 10, 10), cases.edge_reference(f, 10, 10, np.float32)
        got = ref.compare(r32[0], r32[1], r32[2], r64[0], r64[1], r64[2], r64[3])
        print(f, got)
        assert got["contribution"] <= 2.5e-5 and got["total"] <= 2.5e-5 and got["differing"] == 0


def test_edge_batch_holds_what_it_says():
    m, names = cases.edge_matrix()
    lengths = np.diff(m.indptr)
    for n in cases.EDGE_LENGTHS:
        assert lengths[names.index(f"len{n}")] == n
    assert (m.data[m.indptr[names.index("all_negative")]:m.indptr[names.index("all_negative") + 1]] < 0).all()
    ids = cases.edge_items(10)
    liked = m.indices[m.indptr[names.index("likes_40")]:m.indptr[names.index("likes_40") + 1]].tolist()
    assert ids[names.index("likes_40"), 0] in liked and ids[names.index("likes_40"), 1] not in liked
    assert cases.EDGE_ITEMS - 1 in liked and ids[names.index("likes_40_again"), 1] == cases.EDGE_ITEMS - 1
    assert ids[names.index("len1"), 0] == cases.EDGE_ITEMS - 1


def test_model_modules_import_without_a_device():
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.ann.ivf as ivf
        import implicit_amd.gpu.als as als
        import implicit_amd.gpu.bpr as bpr
        import implicit_amd.gpu.lmf as lmf
    for cls in (als.AlternatingLeastSquares, ivf.IVFModel):
        assert callable(getattr(cls, "explain")) and callable(getattr(cls, "explain_batch"))
    for cls in (bpr.BayesianPersonalizedRanking, lmf.LogisticMatrixFactorization):  # ALS only, as the reference
        assert not hasattr(cls, "explain") and not hasattr(cls, "explain_batch")
