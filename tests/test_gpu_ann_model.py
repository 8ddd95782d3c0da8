"""IVFModel / IVFAlternatingLeastSquares (implicit_amd.ann, implicit_amd.approximate_als) over a small ALS fit: with every
list probed the approximate calls equal the exact model's (ids audited by the near-tie rule of smoke(), scores within
rtol = 1e-4, atol = 1e-7); with few lists probed they stay inside the catalogue and honour the filters."""
import warnings

import numpy as np
import pytest

import ivf_reference as ref

pytestmark = pytest.mark.gpu

USERS, ITEMS, FACTORS, NLIST = 2000, 900, 32, 12


@pytest.fixture(scope="module")
def fitted(gpu):
    from implicit_amd.approximate_als import IVFAlternatingLeastSquares
    from implicit_amd.synthetic import synthetic_csr

    user_items = synthetic_csr(USERS, ITEMS, 60_000, seed=5)
    wrapped = IVFAlternatingLeastSquares(factors=FACTORS, iterations=3, random_state=7, nlist=NLIST, nprobe=NLIST, use_gpu=True)
    wrapped.fit(user_items, show_progress=False)
    return wrapped, user_items


def _same(model, queries, got, want, cosine=False):
    """got == want under the audit; `queries`: the float64 query rows the scores belong to."""
    got_ids, got_scores = (np.atleast_2d(x) for x in got)
    want_ids, want_scores = (np.atleast_2d(x) for x in want)
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    items = model.item_factors.to_numpy().astype(np.float64)
    if cosine:
        norms = np.linalg.norm(items, axis=1)
        norms[norms == 0] = 1e-10
        items = items / norms[:, None]
    ref.audit(got_ids, want_ids, want_scores.astype(np.float64), lambda r, i: items[i] @ queries[r], FACTORS)
    np.testing.assert_allclose(got_scores, want_scores, rtol=1e-4, atol=1e-7)


def _user_rows(model, userids):
    return model.user_factors.to_numpy().astype(np.float64)[np.atleast_1d(userids)]


@pytest.mark.parametrize("userids", [17, np.arange(300, 365)], ids=["scalar", "batch65"])
def test_recommend_matches_the_exact_model(gpu, fitted, userids):
    wrapped, user_items = fitted
    model = wrapped.model
    liked = user_items[userids]
    rows = _user_rows(model, userids)
    for kwargs in (dict(), dict(filter_already_liked_items=False), dict(filter_items=[3, 5, 8, 400, 899]),
                   dict(filter_already_liked_items=False, filter_items=[0, 1, 2])):
        _same(model, rows, wrapped.recommend(userids, liked, N=10, **kwargs), model.recommend(userids, liked, N=10, **kwargs))
    got = wrapped.recommend(userids, liked, N=10, recalculate_user=True)
    want = model.recommend(userids, liked, N=10, recalculate_user=True)
    _same(model, model.recalculate_user(userids, liked).to_numpy().astype(np.float64), got, want)


@pytest.mark.parametrize("itemids", [41, np.arange(100, 165)], ids=["scalar", "batch65"])
def test_similar_items_matches_the_exact_model(gpu, fitted, itemids):
    wrapped, _ = fitted
    model = wrapped.model
    items = model.item_factors.to_numpy().astype(np.float64)
    norms = np.linalg.norm(items, axis=1)
    norms[norms == 0] = 1e-10
    queries = (items / norms[:, None])[np.atleast_1d(itemids)]
    _same(model, queries, wrapped.similar_items(itemids, N=10), model.similar_items(itemids, N=10), cosine=True)
    _same(model, queries, wrapped.similar_items(itemids, N=5, filter_items=[41, 100, 7]),
          model.similar_items(itemids, N=5, filter_items=[41, 100, 7]), cosine=True)


def test_few_probes_stay_in_the_catalogue(gpu, fitted):
    wrapped, user_items = fitted
    userids = np.arange(65)
    wrapped.nprobe = 3
    try:
        ids, scores = wrapped.recommend(userids, user_items[userids], N=10, filter_items=[1, 2, 3])
        one_ids, one_scores = wrapped.recommend(5, user_items[5], N=10, filter_items=[1, 2, 3])
    finally:
        wrapped.nprobe = NLIST
    assert ids.shape == (65, 10) and scores.shape == (65, 10)
    assert ((ids >= -1) & (ids < ITEMS)).all()
    np.testing.assert_array_equal(one_ids, ids[5])
    np.testing.assert_array_equal(one_scores, scores[5])
    for r, u in enumerate(userids):
        found = ids[r][ids[r] >= 0]
        assert len(found) == len(set(found)) and len(found) >= 1
        assert not set(found) & set(user_items[u].indices) and not set(found) & {1, 2, 3}
        assert (np.diff(scores[r][ids[r] >= 0]) <= 0).all()


def test_fallback_to_the_exact_model(gpu, fitted):
    wrapped, user_items = fitted
    model = wrapped.model
    filter_items = list(range(500, 1600))  # 1100 ids, count >= 1024: more than a search returns (400 of them are in the catalogue)
    wrapped.nprobe = 1  # the approximate path could not give the exact answer
    try:
        got = wrapped.recommend(9, user_items[9], N=10, filter_items=filter_items)
        got_items = wrapped.similar_items(9, N=10, filter_items=filter_items)
    finally:
        wrapped.nprobe = NLIST
    want = model.recommend(9, user_items[9], N=10, filter_items=filter_items)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    want_items = model.similar_items(9, N=10, filter_items=filter_items)
    np.testing.assert_array_equal(got_items[0], want_items[0])


def test_exceptions_and_aliases(gpu, fitted):
    from implicit_amd import approximate_als
    from implicit_amd.ann import IVFModel
    from implicit_amd.utils import ParameterWarning

    wrapped, user_items = fitted
    assert isinstance(wrapped, IVFModel)
    assert approximate_als.FaissAlternatingLeastSquares is approximate_als.IVFAlternatingLeastSquares
    assert "native" in approximate_als.FaissAlternatingLeastSquares.__doc__
    with pytest.raises(NotImplementedError):
        wrapped.recommend(3, user_items[3], items=[1, 2, 3])
    with pytest.raises(NotImplementedError):
        wrapped.similar_items(3, items=[1, 2, 3])
    with pytest.raises(NotImplementedError):
        wrapped.similar_users(3)
    with pytest.raises(NotImplementedError):
        wrapped.save("model.npz")
    with pytest.raises(NotImplementedError):
        IVFModel.load("model.npz")
    with pytest.raises(ValueError):
        approximate_als.FaissAlternatingLeastSquares(factors=8, use_gpu=False)
    big = IVFModel(wrapped.model, nlist=5000, nprobe=5000, iterations=2, random_state=1)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        big.build_indexes()
    assert any(issubclass(w.category, ParameterWarning) for w in caught)
    assert big.recommend_index.nlist == ITEMS and big.similar_items_index.nlist == ITEMS
    want_ids, want_scores = wrapped.model.recommend(4, user_items[4], N=5)
    rows = _user_rows(wrapped.model, 4)
    _same(wrapped.model, rows, big.recommend(4, user_items[4], N=5), (want_ids, want_scores))
