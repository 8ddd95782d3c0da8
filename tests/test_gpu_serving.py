"""recommend / similar_items / similar_users of the GPU models against the float64 restatement tests/serving_reference.py
(pinned to the reference's own output by tests/test_serving_host.py).  Factors are assigned, not trained, so every expected
answer is a pure function of tests/serving_cases.py.

Comparison rule: ids exactly equal except audited near-ties (serving_reference.audit, the rule of smoke()), at most 1 % of a
case's positions -- tests/test_serving_host.py::test_margin_census proves the inputs themselves stay inside that cap;
scores rtol 1e-4, atol 1e-7 (fp16 storage: the restatement runs on the fp16-rounded factors, rtol 2e-3).  Tail positions
(filtered -FLT_MAX / -inf, unwritten 0.0) are compared like every other."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import serving_cases as cases
import serving_reference as ref

pytestmark = pytest.mark.gpu

_models = {}


def new_model(gpu, name, **kw):
    """A model of serving_cases.MODELS with its factors assigned (no fit)."""
    kind, width, dtype, _, _ = cases.MODELS[name]
    if kind == "als":
        from implicit_amd.gpu.als import AlternatingLeastSquares

        model = AlternatingLeastSquares(factors=width, dtype=dtype, regularization=cases.REG, **kw)
    elif kind == "bpr":
        from implicit_amd.gpu.bpr import BayesianPersonalizedRanking

        model = BayesianPersonalizedRanking(factors=width - 1)
    else:
        from implicit_amd.gpu.lmf import LogisticMatrixFactorization

        model = LogisticMatrixFactorization(factors=width - 2)
    X, Y = cases.factors(name)
    model.user_factors, model.item_factors = gpu.Matrix(X.copy()), gpu.Matrix(Y.copy())
    assert model.user_factors.shape == X.shape and model.item_factors.to_numpy().dtype == dtype
    return model


def shared_model(gpu, name):
    if name not in _models:
        _models[name] = new_model(gpu, name)
    return _models[name]


def rtol_of(name):
    return 2e-3 if cases.MODELS[name][2] == np.float16 else 1e-4


def compare(got, want, score_of, f, rtol):
    """The comparison rule of the module docstring; returns the number of audited near-ties."""
    (got_ids, got_scores), (want_ids, want_scores) = got, want
    got_ids, got_scores = np.atleast_2d(got_ids), np.atleast_2d(got_scores)
    want_ids, want_scores = np.atleast_2d(want_ids), np.atleast_2d(want_scores)
    assert got_ids.shape == want_ids.shape and got_scores.shape == want_scores.shape
    np.testing.assert_allclose(got_scores, want_scores, rtol=rtol, atol=1e-7)
    exceptions = ref.audit(got_ids, want_ids, want_scores, score_of, f)
    assert exceptions <= 0.01 * got_ids.size, f"{exceptions} near-ties in {got_ids.size} positions"
    return exceptions


def dot_scorer(Q, Y):
    Q, Y = np.atleast_2d(Q).astype(np.float64), Y.astype(np.float64)
    return lambda r, i: Q[r] @ Y[i]


def cosine_scorer(Q, F, qnorm):
    Q, F = np.atleast_2d(Q).astype(np.float64), F.astype(np.float64)
    norms, qnorm = ref.calculate_norms(F), np.atleast_1d(qnorm)
    return lambda r, i: Q[r] @ F[i] / norms[i] / qnorm[r]


def call(model, case):
    X, Y = cases.factors(case["model"])
    if case["call"] == "recommend":
        rows = cases.rows_of(cases.liked(len(Y)), case["userid"])
        got = model.recommend(case["userid"], rows, N=case["N"], filter_already_liked_items=case["filter_liked"],
                              filter_items=case["filter_items"], items=case["items"])
        return got, dot_scorer(X[np.atleast_1d(case["userid"])], Y)
    if case["call"] == "similar_items":
        got = model.similar_items(case["qid"], N=case["N"], filter_items=case["filter_ids"], items=case["subset"])
        F = Y
    else:
        got = model.similar_users(case["qid"], N=case["N"], filter_users=case["filter_ids"], users=case["subset"])
        F = X
    qids = np.atleast_1d(case["qid"])
    return got, cosine_scorer(F[qids], F, ref.calculate_norms(F)[qids])


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_serving_case(gpu, case):
    model = shared_model(gpu, case["model"])
    got, score_of = call(model, case)
    scalar = np.isscalar(case["userid"] if case["call"] == "recommend" else case["qid"])
    assert got[0].ndim == got[1].ndim == (1 if scalar else 2)
    exceptions = compare(got, cases.expected(case), score_of, cases.width(case), rtol_of(case["model"]))
    print(f"{cases.case_id(case)}: {exceptions} audited near-ties in {got[0].size} positions")


@pytest.mark.parametrize("name", sorted(cases.MODELS))
def test_view_and_gather_queries_agree_bitwise(gpu, name):
    """A consecutive run of user ids as an ndarray takes the row-range view of the factors, the same ids as a python list
    the gather: same bits.  The run starts off a 128-row block and crosses rows 128 and 256."""
    model = shared_model(gpu, name)
    rows = cases.rows_of(cases.liked(cases.MODELS[name][3]), cases.VIEW)
    for kw in (dict(N=10), dict(N=37, filter_already_liked_items=False), dict(N=5, filter_items=[3, 17])):
        view = model.recommend(cases.VIEW, rows, **kw)
        gather = model.recommend([int(u) for u in cases.VIEW], rows, **kw)
        assert_array_equal(view[0], gather[0])
        assert_array_equal(view[1].view(np.uint32), gather[1].view(np.uint32))


@pytest.mark.parametrize("name", sorted(cases.MODELS))
def test_batch_rows_equal_scalar_calls_bitwise(gpu, name):
    model = shared_model(gpu, name)
    items = cases.MODELS[name][3]
    users = np.concatenate([cases.REPEATED, np.arange(250, 262)])
    rows = cases.rows_of(cases.liked(items), users)
    sub = cases.SMALL_SUBSET if items == cases.SMALL_ITEMS else cases.SUBSET
    for kw in (dict(N=10), dict(N=37, filter_already_liked_items=False), dict(N=7, items=sub), dict(N=4, filter_items=[17, 3])):
        ids, scores = model.recommend(users, rows, **kw)
        for r, u in enumerate(users):
            one_ids, one_scores = model.recommend(int(u), rows[r], **kw)
            assert_array_equal(one_ids, ids[r], err_msg=f"user {u} {kw}")
            assert_array_equal(one_scores.view(np.uint32), scores[r].view(np.uint32), err_msg=f"user {u} {kw}")
    queries = cases.ITEM_BATCH[:12]
    ids, scores = model.similar_items(queries, N=9)
    for r, i in enumerate(queries):
        one_ids, one_scores = model.similar_items(int(i), N=9)
        assert_array_equal(one_ids, ids[r])
        assert_array_equal(one_scores.view(np.uint32), scores[r].view(np.uint32))


@pytest.mark.parametrize("name", sorted(cases.MODELS))
def test_duplicated_rows_tie_larger_id_first(gpu, name):
    model = shared_model(gpu, name)
    group = sorted(cases.DUP_ITEMS[0], reverse=True)
    ids, scores = model.recommend(cases.LEAD_USER, None, N=5, filter_already_liked_items=False)
    assert list(ids[:3]) == group and len(set(scores[:3].view(np.uint32).tolist())) == 1
    ids, scores = model.similar_items(group[1], N=5)
    assert list(ids[:3]) == group and len(set(scores[:3].view(np.uint32).tolist())) == 1
    np.testing.assert_allclose(scores[:3], 1.0, rtol=rtol_of(name))
    pair = sorted(cases.DUP_ITEMS[1], reverse=True)
    ids, scores = model.similar_items(np.array(pair), N=2)
    assert ids.tolist() == [pair, pair] and len(set(scores.view(np.uint32).ravel().tolist())) == 1
    # one place for three equal scores: the bounded heap of the contract keeps the first arrival, the smallest id
    ids, _ = model.recommend(cases.LEAD_USER, None, N=1, filter_already_liked_items=False)
    assert list(ids) == [group[-1]]


def test_own_id_first_with_score_one(gpu):
    model = shared_model(gpu, "als64")
    plain_items = np.array([i for i in cases.ITEM_BATCH if i not in cases.PLANTED_ITEMS])
    ids, scores = model.similar_items(plain_items, N=3)
    assert_array_equal(ids[:, 0], plain_items)
    np.testing.assert_allclose(scores[:, 0], 1.0, rtol=1e-4)
    plain_users = np.array([u for u in cases.USER_BATCH if u not in cases.PLANTED_USERS])
    ids, scores = model.similar_users(plain_users, N=3)
    assert_array_equal(ids[:, 0], plain_users)
    np.testing.assert_allclose(scores[:, 0], 1.0, rtol=1e-4)


def test_host_side_rejections(gpu):
    """Everything here is refused by the Python layer before any launch; no out-of-range id reaches a kernel."""
    model = shared_model(gpu, "als32")
    liked = cases.liked()
    with pytest.raises(ValueError):
        model.recommend(7, liked[7], items=[1, 2, 3], filter_items=[2])
    for bad in ([1, 2, cases.ITEMS], [-1, 2, 3]):
        with pytest.raises(IndexError):
            model.recommend(7, liked[7], items=bad)
        with pytest.raises(IndexError):
            model.similar_items(7, items=bad)
    for bad in (cases.USERS, np.int64(cases.USERS), -1):
        with pytest.raises((IndexError, ValueError)):
            model.recommend(bad, liked[7])
    for bad in (np.array([0, cases.USERS]), [3, -1], np.arange(cases.USERS - 3, cases.USERS + 1)):
        with pytest.raises(IndexError):
            model.recommend(bad, liked[:len(bad)])
    with pytest.raises(ValueError):
        model.recommend(7, liked[7].tocoo())
    with pytest.raises(ValueError):
        model.recommend(7, liked[7].toarray())
    with pytest.raises(ValueError):
        model.recommend(np.array([7, 8]), liked[7])
    with pytest.raises(ValueError):
        model.recommend(7, liked[[7, 8]], recalculate_user=True, filter_already_liked_items=False)


# ---- fold-in -----------------------------------------------------------------------------------------------------------
def rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b)


@pytest.mark.parametrize("alpha", [1.0, 2.0])
@pytest.mark.parametrize("name", ["als32", "als64h"])
def test_fold_in_users(gpu, oracle, name, alpha):
    """recalculate_user against the oracle's Cholesky solve of the alpha-scaled rows (1e-4 relative, fp16 storage 1e-3);
    recommend(recalculate_user=True) against the restatement on the rows recalculate_user returned."""
    model = new_model(gpu, name, alpha=alpha)
    X, Y = cases.factors(name)
    users = np.array([7, cases.LIKES_ALL, cases.LIKES_NONE, cases.LEAD_USER, 300, 301])
    rows = cases.rows_of(cases.liked(), users)
    got = model.recalculate_user(users, rows).to_numpy()
    want = np.zeros((len(users), X.shape[1]), dtype=np.float32)
    oracle.least_squares((alpha * rows).tocsr(), want, Y.astype(np.float32), cases.REG)
    err = rel(got, want)
    print(f"{name} alpha {alpha}: recalculate_user against the oracle {err:.2e}")
    assert err < (1e-3 if X.dtype == np.float16 else 1e-4)
    one = model.recalculate_user(7, rows[0]).to_numpy()
    assert rel(one, want[:1]) < (1e-3 if X.dtype == np.float16 else 1e-4)
    for kw in (dict(N=10), dict(N=10, filter_already_liked_items=False), dict(N=8, items=cases.SUBSET)):
        served = model.recommend(users, rows, recalculate_user=True, **kw)
        want_served = ref.recommend(got, Y, np.arange(len(users)), rows, **kw)
        compare(served, want_served, dot_scorer(got, Y), X.shape[1], rtol_of(name))
    served = model.recommend(7, rows[0], recalculate_user=True, N=10)
    compare(served, ref.recommend(one, Y, 0, rows[0], N=10), dot_scorer(one, Y), X.shape[1], rtol_of(name))


@pytest.mark.parametrize("alpha", [1.0, 2.0])
@pytest.mark.parametrize("name", ["als32", "als64h"])
def test_fold_in_items(gpu, oracle, name, alpha):
    """recalculate_item likewise; similar_items(recalculate_item=True) divides by the STORED norm of the item id (the
    reference's GPU model layer; its CPU layer takes the recalculated row's norm -- DESIGN.md, serving contract)."""
    model = new_model(gpu, name, alpha=alpha)
    X, Y = cases.factors(name)
    ids = np.array([8, 17, 5, cases.ZERO_ITEM, 640])
    rows = cases.rows_of(cases.likers(), ids)
    got = model.recalculate_item(ids, rows).to_numpy()
    want = np.zeros((len(ids), Y.shape[1]), dtype=np.float32)
    oracle.least_squares((alpha * rows).tocsr(), want, X.astype(np.float32), cases.REG)
    err = rel(got, want)
    print(f"{name} alpha {alpha}: recalculate_item against the oracle {err:.2e}")
    assert err < (1e-3 if Y.dtype == np.float16 else 1e-4)
    stored = ref.calculate_norms(Y)[ids]
    served = model.similar_items(ids, N=10, recalculate_item=True, item_users=rows)
    want_served = ref.similar(Y, ids, 10, query_factors=got)
    compare(served, want_served, cosine_scorer(got, Y, stored), Y.shape[1], rtol_of(name))
    other = ref.similar(Y, ids, 10, query_factors=got, recalculated_norm=True)[1]
    assert not np.allclose(served[1][0], other[0], rtol=1e-2)  # the pinned quirk is visible on these inputs
    one = model.similar_items(8, N=10, recalculate_item=True, item_users=rows[0])
    compare(one, ref.similar(Y, 8, 10, query_factors=got[0]), cosine_scorer(got[:1], Y, stored[:1]), Y.shape[1], rtol_of(name))


# ---- partial_fit_* drops the cached norms ------------------------------------------------------------------------------
def test_partial_fit_items_refreshes_the_norms(gpu):
    model = new_model(gpu, "als32")
    f = cases.width(dict(model="als32"))
    queries = np.array([3, 8, 17])
    before = model.similar_items(queries, N=10)  # fills the norm caches
    ids = np.array([3, cases.ITEMS + 1])          # one changed row, one new row behind a gap (row ITEMS stays zero)
    model.partial_fit_items(ids, cases.rows_of(cases.likers(), np.array([3, 9])))
    F = model.item_factors.to_numpy()
    assert F.shape[0] == cases.ITEMS + 2 and not F[cases.ITEMS].any() and F[cases.ITEMS + 1].any()
    queries = np.array([3, 8, 17, cases.ITEMS + 1, cases.ITEMS])
    after = model.similar_items(queries, N=10)
    qnorm = ref.calculate_norms(F)[queries]
    compare(after, ref.similar(F, queries, 10), cosine_scorer(F[queries], F, qnorm), f, 1e-4)
    assert after[0][0, 0] == 3 and abs(after[1][0, 0] - 1) < 1e-4
    assert not np.allclose(after[1][0], before[1][0], rtol=1e-3)
    # the liked filter and the id map over the grown catalogue
    rows = cases.rows_of(cases.liked(), cases.VIEW)
    rows.resize(len(cases.VIEW), cases.ITEMS + 2)
    X = cases.factors("als32")[0]
    compare(model.recommend(cases.VIEW, rows, N=10), ref.recommend(X, F, cases.VIEW, rows, 10), dot_scorer(X[cases.VIEW], F), f, 1e-4)


def test_partial_fit_users_refreshes_the_norms(gpu):
    model = new_model(gpu, "als32")
    f = cases.width(dict(model="als32"))
    queries = np.array([8, 40, 12])
    before = model.similar_users(queries, N=10)
    ids = np.array([8, cases.USERS + 2])
    model.partial_fit_users(ids, cases.rows_of(cases.liked(), np.array([8, 9])))
    F = model.user_factors.to_numpy()
    assert F.shape[0] == cases.USERS + 3 and not F[cases.USERS].any() and F[cases.USERS + 2].any()
    queries = np.array([8, 40, 12, cases.USERS + 2, cases.USERS + 1])
    after = model.similar_users(queries, N=10)
    qnorm = ref.calculate_norms(F)[queries]
    compare(after, ref.similar(F, queries, 10), cosine_scorer(F[queries], F, qnorm), f, 1e-4)
    assert after[0][0, 0] == 8 and abs(after[1][0, 0] - 1) < 1e-4
    assert not np.allclose(after[1][0], before[1][0], rtol=1e-3)
    Y = cases.factors("als32")[1]
    users = np.array([cases.USERS + 2, 8, 7])
    rows = cases.rows_of(cases.liked(), np.array([9, 8, 7]))
    compare(model.recommend(users, rows, N=10), ref.recommend(F, Y, users, rows, 10), dot_scorer(F[users], Y), f, 1e-4)
