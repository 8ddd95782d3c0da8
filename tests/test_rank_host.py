"""Host side of rank_items / score_items: the normaliser of selected_items, the float64 restatement against a brute-force
loop, and the tie rule on the planted duplicates.  No device."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import rank_cases as cases
import rank_reference as ref
from implicit_amd.utils import candidate_form, candidate_lists


# ---- the normaliser -----------------------------------------------------------------------------------------------------
def test_shared_list_is_repeated_for_every_user():
    for shared in ([5, 3, 9], np.array([5, 3, 9]), np.array([5, 3, 9], dtype=np.int64), (5, 3, 9)):
        assert candidate_form(shared) == "shared"
        offsets, cand = candidate_lists(shared, 3)
        assert offsets.dtype == np.int64 and cand.dtype == np.int32
        assert_array_equal(offsets, [0, 3, 6, 9])
        assert_array_equal(cand, [5, 3, 9] * 3)
    offsets, cand = candidate_lists([], 2)
    assert_array_equal(offsets, [0, 0, 0])
    assert len(cand) == 0
    offsets, cand = candidate_lists([4], 0)
    assert_array_equal(offsets, [0])
    assert len(cand) == 0


def test_padded_array_skips_negative_entries():
    sel = np.array([[-1, 7, -5, 2], [-1, -1, -1, -1], [3, 3, -2, 0]])
    assert candidate_form(sel) == "padded"
    offsets, cand = candidate_lists(sel, 3)
    assert_array_equal(offsets, [0, 2, 2, 5])
    assert_array_equal(cand, [7, 2, 3, 3, 0])
    assert offsets.dtype == np.int64 and cand.dtype == np.int32


def test_ragged_lists_keep_their_order():
    sel = [np.array([9, 1]), [], np.array([4], dtype=np.int16), [2, 2, 2]]
    assert candidate_form(sel) == "ragged"
    offsets, cand = candidate_lists(sel, 4)
    assert_array_equal(offsets, [0, 2, 2, 3, 6])
    assert_array_equal(cand, [9, 1, 4, 2, 2, 2])
    # equal lengths stay ragged (no padding rule) as long as it is not a 2-d ndarray
    offsets, cand = candidate_lists([[1, 2], [3, 4]], 2)
    assert_array_equal(offsets, [0, 2, 4])
    assert_array_equal(cand, [1, 2, 3, 4])
    obj = np.empty(2, dtype=object)
    obj[0], obj[1] = np.array([1]), np.array([2, 3])
    assert candidate_form(obj) == "ragged"
    assert_array_equal(candidate_lists(obj, 2)[0], [0, 1, 3])


def test_the_case_inputs_agree_in_both_forms():
    users = cases.ALL
    ragged = candidate_lists(cases.lists_of(users), len(users))
    pad = candidate_lists(cases.padded(users), len(users))
    assert_array_equal(ragged[0], pad[0])
    assert_array_equal(ragged[1], pad[1])
    assert_array_equal(np.diff(ragged[0]), [cases.length_of(u) for u in users])
    assert set(cases.LENGTHS) == {cases.length_of(u) for u in users}


@pytest.mark.parametrize("sel, batch, error", [
    (np.array([[1, 2], [3, 4]]), 3, ValueError),        # rows != users
    ([[1], [2]], 3, ValueError),                        # lists != users
    (np.zeros((2, 2, 2), dtype=np.int32), 2, ValueError),
    (np.array([1.0, 2.0]), 1, ValueError),              # not integers
    (np.array([[1.5, 2.0]]), 1, ValueError),
    ([[1.5], [2]], 2, ValueError),
    ([np.array([[1, 2]]), [3]], 2, ValueError),         # a list that is not 1-d
    (5, 1, ValueError),
    (np.array([2**40]), 1, IndexError),                 # beyond int32: no such item
], ids=repr)
def test_normaliser_rejections(sel, batch, error):
    with pytest.raises(error):
        candidate_lists(sel, batch)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_scores_against_a_python_loop():
    X, Y = cases.factors("bpr33")
    users = [4, 20, cases.LIKES_ALL, cases.LIKES_NONE]  # lists of 64, 63, 6000, 5000
    lists = [l[:80] for l in cases.lists_of(users)]
    liked = cases.rows_of(cases.liked(), users)
    got, mags = ref.scores(X, Y, users, lists, liked)
    plain, _ = ref.scores(X, Y, users, lists)
    filtered = 0
    for r, u in enumerate(users):
        row = set(liked.indices[liked.indptr[r]:liked.indptr[r + 1]].tolist())
        for j, i in enumerate(lists[r]):
            s = sum(float(X[u, k]) * float(Y[i, k]) for k in range(X.shape[1]))
            m = sum(abs(float(X[u, k])) * abs(float(Y[i, k])) for k in range(X.shape[1]))
            assert abs(plain[r][j] - s) <= 1e-15 and abs(mags[r][j] - m) <= 1e-15
            assert got[r][j] == (-float(ref.FLT_MAX) if int(i) in row else plain[r][j])
            filtered += int(i) in row
    assert filtered >= 80 and (got[2] == -float(ref.FLT_MAX)).all() and (got[3] == plain[3]).all()


def test_rank_against_a_python_sort():
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 50, 200)
    s = rng.integers(-3, 4, 200).astype(np.float32) * np.float32(0.5)
    s[s == 0] = np.where(rng.random((s == 0).sum()) < 0.5, np.float32(-0.0), np.float32(0.0))
    want = sorted(zip(s.tolist(), ids.tolist()), key=lambda p: (-p[0], -p[1]))  # python: -0.0 == 0.0
    for N in (1, 7, 200, 230):
        got_ids, got_scores = ref.rank(s, ids, N)
        assert got_ids.dtype == np.int32 and got_scores.dtype == np.float32 and len(got_ids) == len(got_scores) == N
        n = min(N, 200)
        assert_array_equal(got_ids[:n], [p[1] for p in want[:n]])
        assert_array_equal(got_scores[:n], np.array([p[0] for p in want[:n]], dtype=np.float32))
        assert (got_ids[n:] == -1).all() and (got_scores[n:] == -ref.FLT_MAX).all()
    empty = ref.rank(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32), 3)
    assert_array_equal(empty[0], [-1, -1, -1])
    assert (empty[1] == -ref.FLT_MAX).all()


def test_planted_duplicates_tie_larger_id_first():
    X, Y = cases.factors("als32")
    for u in (7, 12, 16):  # lists of 256, 4095, 6000: every planted item is in them
        ids = cases.lists()[u]
        s64, _ = ref.scores(X, Y, [u], [ids])
        got_ids, got_scores = ref.rank(s64[0].astype(np.float32), ids, len(ids))
        pos = {int(i): int(np.flatnonzero(got_ids == i)[0]) for g in cases.DUP_ITEMS for i in g}
        for group in cases.DUP_ITEMS:
            where = [pos[i] for i in sorted(group, reverse=True)]
            assert where == list(range(where[0], where[0] + len(group)))  # adjacent, larger id first
    zero = cases.lists()[cases.ZERO_USER]
    s64, _ = ref.scores(X, Y, [cases.ZERO_USER], [zero])
    assert (s64[0] == 0).all()
    assert_array_equal(ref.rank(s64[0].astype(np.float32), zero, len(zero))[0], np.sort(zero)[::-1])


def test_repeated_ids_are_in_the_lists():
    for u in range(cases.USERS):
        ids = cases.lists()[u]
        counts = np.bincount(ids, minlength=cases.ITEMS)
        assert counts.max() == (3 if cases.length_of(u) in cases.REPEAT_LENGTHS else min(1, len(ids)))
        if len(ids) > 2:
            assert (np.diff(ids) < 0).any() and (np.diff(ids) > 0).any()  # unsorted
    assert_array_equal(np.sort(cases.lists()[16]), np.arange(cases.ITEMS))  # every item
