"""CPU checks of the EASE restatement (tests/ease_reference.py) against facts that do not depend on it, and of the inputs the
GPU suite (tests/test_gpu_ease.py) runs: the exact Gram cases stay exact in float32, and the LAPACK-fp32 yardstick of the
inverse is sound on every SPD case."""
import numpy as np
import pytest

import ease_reference as ref


@pytest.fixture(scope="module")
def gold():
    return ref.golden()


def test_golden_weights_are_the_closed_form(gold):
    X, reg, B = gold["X"], float(gold["regularization"]), gold["B"]
    assert X.shape == (60, 40) and X.dtype == np.float32 and B.dtype == np.float64
    assert len(np.unique(X[X != 0])) > 3  # weighted values
    np.testing.assert_allclose(ref.ease64(X, reg), B, rtol=0, atol=1e-13)
    assert np.all(np.diag(B) == 0.0)


def test_stationarity_of_every_column(gold):
    """G B[:, j] = G[:, j] - e_j / P[j, j]: the normal equations of column j's ridge regression with B[j, j] forced to 0."""
    X, reg, B = gold["X"], float(gold["regularization"]), gold["B"]
    G = ref.gram64(X, reg)
    P = np.linalg.inv(G)
    rhs = G - np.diag(1.0 / np.diag(P))
    np.testing.assert_allclose(G @ B, rhs, rtol=0, atol=1e-9 * np.abs(G).max())


@pytest.mark.parametrize("j", [0, 7, 39])
def test_column_is_the_ridge_regression_on_the_other_items(gold, j):
    X, reg, B = gold["X"].astype(np.float64), float(gold["regularization"]), gold["B"]
    others = np.delete(np.arange(X.shape[1]), j)
    A = np.vstack([X[:, others], np.sqrt(reg) * np.eye(len(others))])  # the lambda-augmented system
    y = np.concatenate([X[:, j], np.zeros(len(others))])
    w = np.linalg.lstsq(A, y, rcond=None)[0]
    np.testing.assert_allclose(B[others, j], w, rtol=0, atol=1e-10)
    assert B[j, j] == 0.0


def test_scores32_agrees_with_the_golden_scores(gold):
    X, B = gold["X"], gold["B"]
    B32 = B.astype(np.float32)
    for r, u in enumerate(gold["users"]):
        cols = np.flatnonzero(X[u])
        s = ref.scores32(B32, cols, X[u, cols])
        s64 = X[u].astype(np.float64) @ B
        bound = (len(cols) + 2) * 2.0**-23 * (np.abs(X[u].astype(np.float64)) @ np.abs(B))
        assert np.all(np.abs(s - s64) <= bound + 1e-30)
        s[cols] = -ref.FLT_MAX
        ids, top = ref.topk_order(s, 5)
        np.testing.assert_array_equal(ids, gold["top_ids"][r])
        np.testing.assert_allclose(top, gold["top_scores"][r], rtol=0, atol=float(bound.max()))


def test_weights32_is_one_division():
    P = ref.lapack32_inverse(ref.spd_case(31)[0])
    B = ref.weights32(P)
    assert B.dtype == np.float32 and np.all(np.diag(B) == 0)
    i, j = 4, 9
    assert B[i, j] == -(np.float32(P[i, j]) / np.float32(P[j, j]))
    np.testing.assert_allclose(B, ref.weights64(P.astype(np.float64)), rtol=2.0**-23, atol=0)


def test_topk_order_rules():
    s = np.array([1.0, -0.0, 0.0, 1.0, -3.0], dtype=np.float32)
    ids, top = ref.topk_order(s, 7)
    np.testing.assert_array_equal(ids, [3, 0, 2, 1, 4, -1, -1])  # ties by id descending, -0.0 ranks as +0.0
    assert not np.signbit(top[2]) and not np.signbit(top[3])
    assert top[5] == -ref.FLT_MAX and top[6] == -ref.FLT_MAX


@pytest.mark.parametrize("items", ref.GRAM_EXACT_ITEMS)
def test_exact_gram_cases_stay_below_2_24(items):
    X = ref.gram_exact_case(items)
    assert X.shape[1] == items and X.shape[0] >= 4 * items
    assert ref.max_partial_sum(X) < 2.0**24
    assert np.all(X.data == np.rint(X.data)) and X.data.min() >= 1 and X.data.max() <= 3
    lens = np.diff(X.indptr)
    assert lens[1] == 0  # an empty user row
    held = np.bincount(X.indices, minlength=items)
    assert held[0] == (lens > 0).sum() or items == 1  # one item held by every (non-empty) user
    if 2 < items < 257:
        assert held[items - 2] == 0  # an item nobody has
    if items == 257:
        assert lens.max() > 256


@pytest.mark.parametrize("n", ref.SPD_SIZES)
def test_lapack_fp32_is_a_sound_yardstick(n):
    G32, P64 = ref.spd_case(n)
    cond = np.linalg.cond(G32.astype(np.float64))
    d_ref = ref.rel_distance(ref.lapack32_inverse(G32), P64)
    assert np.isfinite(cond) and np.isfinite(d_ref)
    assert d_ref < 1e-5
