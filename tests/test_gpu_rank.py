"""rank_items / score_items of the GPU models (csrc/rank.hip) on the inputs of tests/rank_cases.py.

Scores are checked against float64 on the stored factors with the derived bound |s - s64| <= w 2^-23 sum_k |x_k| |y_k| (twice
gamma_w of an fp32 dot product in any summation order).  The ORDER is checked exactly, with no near-tie allowance: rank_items
must equal the sort (rank_reference.rank) of the scores score_items returns for the same arguments, and a pair's score has the
same bits wherever it is computed.

The mixed batch holds lists of 4097, 5000 and 6000 candidates, which are ranked for N <= 1024 only (a ValueError otherwise,
test_rejections): N in {1, 2, 10, 1024} runs on the whole mixed batch, N in {None, longest + 5, 1025} on its 42 users whose
lists have at most 4096 entries (still every length from 0 to 4096)."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import rank_cases as cases
import rank_reference as ref

pytestmark = pytest.mark.gpu

NAMES = sorted(cases.MODELS)
_models, _scores = {}, {}


def new_model(gpu, name):
    """A model of rank_cases.MODELS with its factors assigned (no fit)."""
    kind, width, dtype, _ = cases.MODELS[name]
    if kind == "als":
        from implicit_amd.gpu.als import AlternatingLeastSquares

        model = AlternatingLeastSquares(factors=width, dtype=dtype, regularization=cases.REG)
    elif kind == "bpr":
        from implicit_amd.gpu.bpr import BayesianPersonalizedRanking

        model = BayesianPersonalizedRanking(factors=width - 1)
    else:
        from implicit_amd.gpu.lmf import LogisticMatrixFactorization

        model = LogisticMatrixFactorization(factors=width - 2)
    X, Y = cases.factors(name)
    model.user_factors, model.item_factors = gpu.Matrix(X.copy()), gpu.Matrix(Y.copy())
    return model


def shared_model(gpu, name):
    if name not in _models:
        _models[name] = new_model(gpu, name)
    return _models[name]


def mixed_scores(gpu, name):
    """score_items of the mixed batch (every user against its own list), computed once per model and left unchanged."""
    if name not in _scores:
        got = shared_model(gpu, name).score_items(cases.ALL, cases.lists_of(cases.ALL))
        for s in got:
            s.setflags(write=False)
        _scores[name] = got
    return _scores[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expected_rank(score_lists, lists, N):
    rows = [ref.rank(s, ids, N) for s, ids in zip(score_lists, lists)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def assert_ranked(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])


# ---- 1. scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_scores_against_float64(gpu, name):
    X, Y = cases.factors(name)
    w = cases.MODELS[name][1]
    lists = cases.lists_of(cases.ALL)
    got = mixed_scores(gpu, name)
    assert isinstance(got, list) and [len(s) for s in got] == [len(l) for l in lists]
    s64, mags = ref.scores(X, Y, cases.ALL, lists)
    worst = 0.0
    for s, want, m in zip(got, s64, mags):
        assert s.dtype == np.float32
        bound = w * 2.0 ** -23 * m
        err = np.abs(s.astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if len(s) else 0.0)
        assert (err <= bound).all()
    print(f"{name}: largest |s - s64| / bound = {worst:.3f}")
    # the 2-d form: the same bits at the entries, -FLT_MAX at the padding
    pad = cases.padded(cases.ALL)
    got2 = shared_model(gpu, name).score_items(cases.ALL, pad)
    assert got2.shape == pad.shape and got2.dtype == np.float32
    assert (got2[pad < 0] == -ref.FLT_MAX).all()
    assert_array_equal(bits(got2[pad >= 0]), bits(np.concatenate(got)))


@pytest.mark.parametrize("name", ["als32", "als64h", "bpr33"])
def test_filtered_scores_are_exactly_flt_max(gpu, name):
    """Score mode with the liked pattern (KnnQuery.rank, n = 0): a liked candidate is -FLT_MAX, every other keeps its bits."""
    from implicit_amd.utils import candidate_lists

    model = shared_model(gpu, name)
    lists = cases.lists_of(cases.ALL)
    offsets, cand = candidate_lists(lists, cases.USERS)
    liked = cases.liked().sorted_indices()
    got = model.knn.rank(model.item_factors, model.user_factors, offsets, cand, 0, liked)
    plain = np.concatenate(mixed_scores(gpu, name))
    hit = np.concatenate([np.isin(ids, liked.indices[liked.indptr[u]:liked.indptr[u + 1]]) for u, ids in enumerate(lists)])
    assert hit.sum() > 1000 and (~hit).sum() > 1000
    assert_array_equal(bits(got), bits(np.where(hit, -ref.FLT_MAX, plain)))


# ---- 2. order, exactly ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 10, 1024])
@pytest.mark.parametrize("name", NAMES)
def test_order_of_the_mixed_batch(gpu, name, N):
    lists = cases.lists_of(cases.ALL)
    got = shared_model(gpu, name).rank_items(cases.ALL, None, lists, N=N)
    assert got[0].shape == got[1].shape == (cases.USERS, N)
    assert_ranked(got, expected_rank(mixed_scores(gpu, name), lists, N))
    assert_ranked(shared_model(gpu, name).rank_items(cases.ALL, None, cases.padded(cases.ALL), N=N), got)


@pytest.mark.parametrize("N", [None, 4096 + 5, 1025])
@pytest.mark.parametrize("name", NAMES)
def test_order_of_the_lists_up_to_4096(gpu, name, N):
    users = cases.SHORT_USERS
    lists = cases.lists_of(users)
    assert max(len(l) for l in lists) == 4096
    got = shared_model(gpu, name).rank_items(users, None, lists, N=N)
    width = 4096 if N is None else N
    assert got[0].shape == (len(users), width)
    assert_ranked(got, expected_rank([mixed_scores(gpu, name)[u] for u in users], lists, width))


@pytest.mark.parametrize("userid", [7, np.int64(14), cases.VIEW, [int(u) for u in cases.VIEW], cases.UNSORTED, cases.REPEATED],
                         ids=["int", "int64-scalar", "view", "view-as-list", "unsorted", "repeated"])
@pytest.mark.parametrize("name", ["als32", "als64h", "lmf34"])
def test_order_for_every_userid_form(gpu, name, userid):
    model = shared_model(gpu, name)
    scalar = np.isscalar(userid)
    lists = cases.lists_of(userid)
    selected = lists[0] if scalar else lists
    got = model.rank_items(userid, None, selected, N=10)
    assert got[0].shape == got[1].shape == ((10,) if scalar else (len(userid), 10))
    scores = model.score_items(userid, selected)
    want = expected_rank([scores] if scalar else scores, lists, 10)
    assert_ranked(got, (want[0][0], want[1][0]) if scalar else want)
    for r, u in enumerate(np.atleast_1d(userid)):  # the same user against the same list: the bits of the mixed batch
        assert_array_equal(bits(scores if scalar else scores[r]), bits(mixed_scores(gpu, name)[int(u)]))


def test_shared_list_forms(gpu):
    model = shared_model(gpu, "als32")
    shared = cases.lists()[5]  # 65
    scores = model.score_items(cases.VIEW, shared)
    assert scores.shape == (len(cases.VIEW), 65)
    ids, ranked = model.rank_items(cases.VIEW, None, [int(i) for i in shared])
    assert ids.shape == (len(cases.VIEW), 65)
    assert_ranked((ids, ranked), expected_rank(scores, [shared] * len(cases.VIEW), 65))
    one = model.score_items(9, shared)
    assert one.shape == (65,)
    assert_array_equal(bits(one), bits(scores[9 - cases.VIEW[0]]))
    empty = model.rank_items(cases.VIEW, None, [])
    assert empty[0].shape == empty[1].shape == (len(cases.VIEW), 0)
    padded_row = model.rank_items(cases.VIEW[:3], None, [[], [4], []], N=2)
    assert_array_equal(padded_row[0], [[-1, -1], [4, -1], [-1, -1]])
    assert (padded_row[1][[0, 2]] == -ref.FLT_MAX).all() and padded_row[1][1, 1] == -ref.FLT_MAX


# ---- 3. pair determinism, bitwise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_pair_scores_the_same_bits_everywhere(gpu, name):
    model = shared_model(gpu, name)
    X, Y = cases.factors(name)
    u = 9
    s64 = Y.astype(np.float64) @ X[u].astype(np.float64)
    s64[list(cases.PLANTED_ITEMS)] = -np.inf
    i = int(np.argmax(s64))  # the user's best item: inside every top-N below
    one = model.score_items(u, [i])
    assert one.shape == (1,)
    want = bits(one)[0]
    for base, N in ((cases.lists()[13], 4096), (cases.lists()[16], 1024)):  # lists of 4096 (LDS sort) and 6000 (radix select)
        ids = base.copy()
        ids[0] = ids[-1] = i
        in_list = bits(model.score_items(u, ids))
        assert in_list[0] == want and in_list[-1] == want
        rid, rscore = model.rank_items(u, None, ids, N=N)
        where = np.flatnonzero(rid == i)
        assert len(where) == int((ids == i).sum()) >= 2 and (bits(rscore)[where] == want).all()
    view = model.score_items(np.arange(8, 11), [i])
    gathered = model.score_items([8, 9, 10], [i])
    batch = model.score_items(np.array([40, 9, 2, 9]), [[i, 3], [5, i], [], [i]])
    assert bits(view)[1, 0] == want and bits(gathered)[1, 0] == want
    assert bits(batch[0])[0] != want and bits(batch[1])[1] == want and bits(batch[3])[0] == want


def test_dtype_pairs_give_the_same_bits(gpu):
    """fp16 is widened exactly: the same values stored as fp16 or fp32, on either side, score the same bits."""
    from implicit_amd.utils import candidate_lists

    X, Y = cases.factors("als64h")
    users = np.array([1, 5, 13, 14])  # lists of 1, 65, 4096, 4097
    offsets, cand = candidate_lists(cases.lists_of(users), len(users))
    knn, got = gpu.KnnQuery(), []
    for tq in (np.float16, np.float32):
        for ti in (np.float16, np.float32):
            items, query = gpu.Matrix(Y.astype(ti)), gpu.Matrix(X[users].astype(tq))
            got.append((knn.rank(items, query, offsets, cand), knn.rank(items, query, offsets, cand, 100)))
    for scores, (ids, ranked) in got[1:]:
        assert_array_equal(bits(scores), bits(got[0][0]))
        assert_array_equal(ids, got[0][1][0])
        assert_array_equal(bits(ranked), bits(got[0][1][1]))
    assert_array_equal(bits(got[0][0]), bits(np.concatenate([mixed_scores(gpu, "als64h")[u] for u in users])))


@pytest.mark.parametrize("name", ["als32", "als64h", "als256", "bpr33"])
def test_chunk_boundaries_change_no_byte(gpu, name):
    model = new_model(gpu, name)
    model._knn = gpu.KnnQuery(max_temp_memory=150_000)  # the 6000-list alone takes 104 KB at N = 1024: many chunks
    lists = cases.lists_of(cases.ALL)
    got = model.score_items(cases.ALL, lists)
    for s, want in zip(got, mixed_scores(gpu, name)):
        assert_array_equal(bits(s), bits(want))
    for kw in (dict(N=10), dict(N=1024, filter_already_liked_items=True)):
        chunked = model.rank_items(cases.ALL, cases.liked(), lists, **kw)
        whole = shared_model(gpu, name).rank_items(cases.ALL, cases.liked(), lists, **kw)
        assert_array_equal(chunked[0], whole[0])
        assert_array_equal(bits(chunked[1]), bits(whole[1]))


@pytest.mark.parametrize("name", ["als32", "als128", "lmf34"])
def test_planted_rows(gpu, name):
    model = shared_model(gpu, name)
    shared = cases.lists()[13]
    ids, scores = model.rank_items(np.array(cases.DUP_USERS), None, shared, N=50)
    assert_array_equal(ids[0], ids[1])
    assert_array_equal(bits(scores[0]), bits(scores[1]))
    for u in (7, 12, 16):  # lists of 256, 4095 and 6000 (N <= 1024 there): identical items tie, larger id first
        lst = cases.lists()[u]
        N = min(len(lst), 1024)
        ids, scores = model.rank_items(u, None, lst, N=N)
        for group in cases.DUP_ITEMS:
            where = [np.flatnonzero(ids == i) for i in sorted(group, reverse=True)]
            if all(len(p) for p in where):
                first = int(where[0][0])
                assert [int(p[0]) for p in where] == list(range(first, first + len(group)))
                assert len(set(bits(scores[first:first + len(group)]).tolist())) == 1
    for lst in (cases.lists()[cases.ZERO_USER], cases.lists()[12]):  # a zero user's list (4097, 4095) comes back by id alone
        N = 1024 if len(lst) > 4096 else len(lst)
        ids, scores = model.rank_items(cases.ZERO_USER, None, lst, N=N)
        assert_array_equal(ids, np.sort(lst)[::-1][:N])
        assert (scores == 0).all()


# ---- 4. filter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["als32", "als64h", "als100", "bpr33"])
def test_filter_against_the_restatement(gpu, name):
    model = shared_model(gpu, name)
    liked = cases.liked()
    assert not liked.has_sorted_indices

    def want(users, N):
        out = []
        for r, u in enumerate(users):
            ids = cases.lists()[int(u)]
            hit = np.isin(ids, liked.indices[liked.indptr[u]:liked.indptr[u + 1]])  # stored zeros included
            out.append(np.where(hit, -ref.FLT_MAX, mixed_scores(gpu, name)[int(u)]).astype(np.float32))
        return expected_rank(out, cases.lists_of(users), N)

    for N in (10, 1024):
        got = model.rank_items(cases.ALL, liked, cases.lists_of(cases.ALL), N=N, filter_already_liked_items=True)
        assert_ranked(got, want(cases.ALL, N))
        assert (got[1][cases.LIKES_ALL] == -ref.FLT_MAX).all()  # every candidate liked: all of them stay, by id
        assert_array_equal(got[0][cases.LIKES_ALL], np.arange(cases.ITEMS - 1, cases.ITEMS - 1 - N, -1))
    users = cases.SHORT_USERS
    got = model.rank_items(users, cases.rows_of(liked, users), cases.lists_of(users), filter_already_liked_items=True)
    assert_ranked(got, want(users, 4096))
    got = model.rank_items(cases.UNSORTED, cases.rows_of(liked, cases.UNSORTED), cases.padded(cases.UNSORTED), N=7,
                           filter_already_liked_items=True)
    assert_ranked(got, want(cases.UNSORTED, 7))
    one = model.rank_items(cases.LIKES_NONE, liked[cases.LIKES_NONE], cases.lists()[cases.LIKES_NONE], N=20,
                           filter_already_liked_items=True)
    plain = model.rank_items(cases.LIKES_NONE, None, cases.lists()[cases.LIKES_NONE], N=20)
    assert_ranked(one, plain)


# ---- 5. recalculate_user ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["als32", "als64h"])
def test_recalculated_users_rank_bitwise(gpu, name):
    from implicit_amd.utils import candidate_lists

    model = shared_model(gpu, name)
    users = np.array([7, cases.LIKES_ALL, cases.LIKES_NONE, 12, 14])
    rows = cases.rows_of(cases.liked(), users)
    lists = cases.lists_of(users)
    offsets, cand = candidate_lists(lists, len(users))
    query = model.recalculate_user(users, rows)
    assert not np.array_equal(query.to_numpy(), cases.factors(name)[0][users])
    got = model.rank_items(users, rows, lists, N=10, recalculate_user=True)
    want = model.knn.rank(model.item_factors, query, offsets, cand, 10)
    assert_array_equal(got[0], want[0])
    assert_array_equal(bits(got[1]), bits(want[1]))
    got = model.rank_items(users, rows, lists, N=10, recalculate_user=True, filter_already_liked_items=True)
    want = model.knn.rank(model.item_factors, query, offsets, cand, 10, rows.sorted_indices())
    assert_array_equal(got[0], want[0])
    assert_array_equal(bits(got[1]), bits(want[1]))
    scores = model.score_items(users, lists, user_items=rows, recalculate_user=True)
    assert_array_equal(bits(np.concatenate(scores)), bits(model.knn.rank(model.item_factors, query, offsets, cand)))
    one = model.rank_items(7, rows[0], lists[0], N=10, recalculate_user=True)
    want = model.knn.rank(model.item_factors, model.recalculate_user(7, rows[0]), offsets[:2], cand[:offsets[1]], 10)
    assert_array_equal(one[0], want[0][0])
    assert_array_equal(bits(one[1]), bits(want[1][0]))


# ---- 6. rejections -------------------------------------------------------------------------------------------------------------
def test_rejections(gpu):
    model = shared_model(gpu, "als32")
    liked = cases.liked()
    long_list, short_list = cases.lists()[14], cases.lists()[13]  # 4097, 4096
    with pytest.raises(ValueError, match="1024"):
        model.rank_items(3, None, long_list, N=1025)
    with pytest.raises(ValueError):
        model.rank_items(np.array([3, 4]), None, [short_list, long_list])  # N=None: 4097
    model.rank_items(3, None, long_list, N=1024)
    model.rank_items(3, None, short_list, N=5000)
    for bad in ([0, cases.ITEMS], [-1, 4], np.array([[3, cases.ITEMS]])):
        with pytest.raises(IndexError, match="Some itemids are not in the model"):
            model.rank_items(3, None, bad)
        with pytest.raises(IndexError, match="Some itemids are not in the model"):
            model.score_items(3, bad)
    with pytest.raises(ValueError, match="user_items must contain 1 row for every user in userids"):
        model.rank_items(np.array([3, 4]), liked[[3, 4, 5]], short_list, filter_already_liked_items=True)
    with pytest.raises(ValueError, match="user_items needs to be a CSR sparse matrix"):
        model.rank_items(np.array([3, 4]), None, short_list, filter_already_liked_items=True)
    with pytest.raises(ValueError, match="user_items must contain 1 row for every user in userids"):
        model.score_items(3, short_list, user_items=liked[[3, 4]], recalculate_user=True)
    with pytest.raises(ValueError):
        model.rank_items(3, None, short_list, N=0)
    with pytest.raises(ValueError):
        model.rank_items(np.array([3, 4]), None, [short_list])
    model.rank_items(np.array([3, 4]), None, short_list, N=3)  # user_items is not read without a filter


def test_knn_rank_rejects_before_writing(gpu):
    from implicit_amd.gpu import _hip

    knn = gpu.KnnQuery()
    X, Y = cases.factors("als32")
    items, query = gpu.Matrix(Y.copy()), gpu.Matrix(X[:2].copy())
    offsets, cand = np.array([0, 2, 3], dtype=np.int64), np.array([5, 9, 7], dtype=np.int32)
    plain = knn.rank(items, query, offsets, cand)
    assert_ranked(knn.rank(items, query, offsets, cand, 2), expected_rank([plain[:2], plain[2:]], [cand[:2], cand[2:]], 2))
    with pytest.raises(ValueError, match="same number of columns"):
        knn.rank(items, gpu.Matrix(cases.factors("als64")[0][:2].copy()), offsets, cand, 2)
    with pytest.raises(ValueError):
        knn.rank(items, query, np.array([1, 2, 3], dtype=np.int64), np.array([5, 9, 7], dtype=np.int32), 2)
    with pytest.raises(ValueError):
        knn.rank(items, query, np.array([0, 3, 2], dtype=np.int64), np.array([5, 9], dtype=np.int32), 2)
    with pytest.raises(ValueError):
        knn.rank(items, query, offsets, np.array([5, cases.ITEMS, 7], dtype=np.int32), 2)
    with pytest.raises(ValueError):
        knn.rank(items, query, offsets, cand, -1)
    unsorted = cases.liked()[[4, 5]]
    assert not unsorted.has_sorted_indices
    with pytest.raises(ValueError, match="strictly increasing"):
        knn.rank(items, query, offsets, cand, 2, unsorted)
    with pytest.raises(ValueError, match="bytes"):
        gpu.KnnQuery(max_temp_memory=1000).rank(items, query, np.array([0, 3000, 3000], dtype=np.int64),
                                                np.zeros(3000, dtype=np.int32), 2)
    # at the C boundary: the caller's buffers keep their bytes when the call is refused
    out_ids, out_scores = np.full((2, 2), 12345, dtype=np.int32), np.full((2, 2), 0.5, dtype=np.float32)
    bad = np.array([5, -3, 7], dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    status = _hip.lib().imp_knn_rank(knn._h, items._h, query._h, vp(offsets), vp(bad), 2, None, None, vp(out_ids), vp(out_scores))
    assert status == _hip.IMP_INVALID_ARGUMENT
    assert (out_ids == 12345).all() and (out_scores == 0.5).all()


# ---- 7. forwarders --------------------------------------------------------------------------------------------------------------
def test_ivf_model_forwards(gpu):
    from implicit_amd.ann.ivf import IVFModel

    model = shared_model(gpu, "als32")
    wrapped = IVFModel(model)
    users, liked = cases.VIEW, cases.rows_of(cases.liked(), cases.VIEW)
    lists = cases.lists_of(users)
    got = wrapped.rank_items(users, liked, lists, N=10, filter_already_liked_items=True)
    want = model.rank_items(users, liked, lists, N=10, filter_already_liked_items=True)
    assert_array_equal(got[0], want[0])
    assert_array_equal(bits(got[1]), bits(want[1]))
    for a, b in zip(wrapped.score_items(users, lists), model.score_items(users, lists)):
        assert_array_equal(bits(a), bits(b))


class StubComm:
    def __init__(self, rank, nranks):
        self.rank, self.nranks = rank, nranks


@pytest.mark.parametrize("form", ["ragged", "padded", "shared"])
def test_sharded_rank_items_stacks_into_the_one_call_result(gpu, form):
    from implicit_amd.gpu import sharded

    model = shared_model(gpu, "als64")
    users = cases.SHORT_USERS
    liked = cases.rows_of(cases.liked(), users)
    selected = {"ragged": cases.lists_of(users), "padded": cases.padded(users), "shared": cases.lists()[8]}[form]
    for kw in (dict(), dict(N=10, filter_already_liked_items=True)):
        whole = model.rank_items(users, liked, selected, **kw)
        covered = 0
        for rank in range(3):
            lo, hi, ids, scores = sharded.rank_items(model, StubComm(rank, 3), users, liked, selected, **kw)
            assert lo == covered and hi > lo
            assert_array_equal(ids, whole[0][lo:hi])
            assert_array_equal(bits(scores), bits(whole[1][lo:hi]))
            covered = hi
        assert covered == len(users)
