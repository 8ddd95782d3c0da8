"""Host-only checks of the serving contract (no GPU): the float64 restatement tests/serving_reference.py reproduces what
the reference's own model layer returned (tests/golden/serving_golden.npz, written by tests/golden/make_serving_golden.py),
and the inputs of tests/test_gpu_serving.py hold few enough near-ties for its 1 % cap on audited exceptions."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import serving_cases as cases
import serving_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "serving_golden.npz")
U = 2.0 ** -24  # float32 unit roundoff


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    users, items = len(g["X"]), len(g["Y"])
    g["liked"] = sp.csr_matrix((g["liked_data"], g["liked_indices"], g["liked_indptr"]), shape=(users, items))
    return g


def _restate(g, i, opt):
    """The restatement's answer for golden case i and the scale of its float32 rounding per position."""
    X, Y = g["X"], g["Y"]
    if opt["call"] == "recommend":
        userid = opt["userid"]
        rows = cases.rows_of(g["liked"], userid)
        Q = X[np.atleast_1d(userid)].astype(np.float64)
        if opt["recalculate"]:  # the fold-in itself is the solver's business: restate serving on the reference's own rows
            Q = np.atleast_2d(g[f"c{i}_query"]).astype(np.float64)
        q = 0 if np.isscalar(userid) else np.arange(len(Q))
        ids, scores = ref.recommend(Q, Y, q, rows, opt["N"], opt["filter_liked"], opt["filter_items"], opt["items"])
        ynorm = np.sqrt((Y.astype(np.float64) ** 2).sum(axis=1))
        scale = np.sqrt((Q * Q).sum(axis=1))[:, None] * ynorm[np.atleast_2d(ids)]
        return ids, scores, scale
    F = Y if opt["call"] == "similar_items" else X
    query = g[f"c{i}_query"] if opt["recalculate"] else None
    ids, scores = ref.similar(F, opt["qid"], opt["N"], opt["subset"], opt["filter_ids"], query_factors=query,
                              recalculated_norm=True)
    return ids, scores, np.ones(np.atleast_2d(ids).shape)  # |cosine| <= 1


def test_restatement_equals_the_golden_file(golden):
    """Every recorded case: ids exactly equal (the duplicated rows, the all-filtered and the unwritten tails included),
    -FLT_MAX / -inf / unwritten 0.0 positions exactly equal, every other score within the rounding of the reference's
    float32 arithmetic.  That bound is a priori: an f-term float32 dot product is within f u |q| |y| of the exact one
    (u = 2^-24), and the cosine adds three divisions and two rounded norms, so (f + 5) u |q| |y| covers both calls
    (|q| |y| = 1 for a cosine).  Measured here (printed below) on the golden file, f = 8: recommend 1.92 u, similar_items
    4.0 u, similar_users 4.0 u against the bound of 13 u."""
    g = golden
    f = g["X"].shape[1]
    bound = (f + 5) * U
    worst = {}
    for i, text in enumerate(g["cases"]):
        opt = json.loads(str(text))
        ids, scores, scale = (np.atleast_2d(a) for a in _restate(g, i, opt))
        got_ids, got_scores = np.atleast_2d(g[f"c{i}_ids"]), np.atleast_2d(g[f"c{i}_scores"]).astype(np.float64)
        assert got_ids.shape == ids.shape, (i, opt)
        np.testing.assert_array_equal(got_ids, ids, err_msg=f"case {i}: {opt}")
        exact = ~(scores > -1e30) | (scores == 0)  # filtered and unwritten positions, a zero row's exact 0.0
        np.testing.assert_allclose(got_scores[exact], scores[exact], rtol=1e-6, atol=0, err_msg=f"case {i}: {opt}")
        err = np.abs(got_scores[~exact] - scores[~exact]) / np.maximum(scale[~exact], 1e-300)
        if err.size:
            worst[opt["call"]] = max(worst.get(opt["call"], 0.0), float(err.max()))
            assert err.max() <= bound, (i, opt, err.max() / U)
    print("reference float32 against float64, worst error in units of u |q| |y|:",
          {k: round(v / U, 2) for k, v in worst.items()}, f"bound {bound / U:.0f} u")
    assert set(worst) == {"recommend", "similar_items", "similar_users"}


def test_stored_zero_and_recalculated_norm_quirks(golden):
    """What the golden file decides: a stored zero in user_items filters in a plain recommend() and does not under items=;
    the reference's CPU layer divides a recalculated item's scores by the norm of the recalculated row."""
    g = golden
    liked7 = g["liked"][7]
    zeros = set(liked7.indices[liked7.data == 0].tolist())
    zero = min(zeros)
    seen = set()
    for i, text in enumerate(g["cases"]):
        opt = json.loads(str(text))
        if opt["call"] == "recommend" and opt["userid"] == 7 and opt["filter_liked"] and not opt["recalculate"] \
                and opt["filter_items"] is None:
            ids, scores = g[f"c{i}_ids"], g[f"c{i}_scores"]
            live = set(ids[scores > -1e30].tolist())
            if opt["items"] is None and opt["N"] == len(g["Y"]):
                assert zero not in live
                seen.add("plain")
            if opt["items"] is not None and set(opt["items"]) == set(liked7.indices.tolist()):
                assert live and live <= zeros  # a subset made only of liked items: the stored zeros are all that is left
                seen.add("items")
        if opt["call"] == "similar_items" and opt["recalculate"] and opt["qid"] == 20:
            stored = ref.similar(g["Y"], 20, opt["N"], query_factors=g[f"c{i}_query"])[1]
            assert not np.allclose(stored, g[f"c{i}_scores"], rtol=1e-3)
            seen.add("norm")
    assert seen == {"plain", "items", "norm"}


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_margin_census(case):
    """Near-ties (float64 gap to the next score below 4 f 2^-23 relative) among the positions the GPU test compares: at most
    1 %, so the reference alone stays inside the cap on audited exceptions used there."""
    close, compared = cases.census(case)
    print(f"{cases.case_id(case)}: {close} near-ties in {compared} positions")
    assert compared > 0 and close <= 0.01 * compared


def test_case_ids_are_unique():
    names = [cases.case_id(c) for c in cases.CASES]
    assert len(names) == len(set(names))


def test_planted_duplicates_lead_every_model():
    """The tie-order tests of the GPU file rely on it: for LEAD_USER the three identical item rows come first."""
    group = sorted(cases.DUP_ITEMS[0], reverse=True)
    for name in cases.MODELS:
        X, Y = cases.factors(name)
        ids, scores = ref.recommend(X, Y, cases.LEAD_USER, None, 5, False)
        assert list(ids[:3]) == group and scores[0] == scores[2] > scores[3]
        ids, scores = ref.similar(Y, group[1], 5)
        assert list(ids[:3]) == group and scores[0] == scores[2] > scores[3]
        assert list(ref.recommend(X, Y, cases.LEAD_USER, None, 1, False)[0]) == [group[-1]]


def test_liked_pattern_reindexed_onto_a_subset():
    """The model's host-side re-indexing of the liked pattern under items= (no device involved): positions inside the sorted
    subset, entries outside it and stored zeros dropped -- what the golden file shows the reference to do."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from implicit_amd.gpu.matrix_factorization_base import _filter_items_from_sparse_matrix
    items = np.sort(np.array(cases.SUBSET))
    rows = cases.rows_of(cases.liked(), cases.VIEW)
    got = _filter_items_from_sparse_matrix(items, rows)
    assert got.shape == (len(cases.VIEW), len(items))
    kept = 0
    for r in range(rows.shape[0]):
        cols, data = rows[r].indices, rows[r].data
        want = sorted(np.searchsorted(items, c) for c, d in zip(cols, data) if d != 0 and c in set(items.tolist()))
        assert sorted(got[r].indices.tolist()) == want, r
        kept += len(want)
    assert 0 < kept < rows.nnz and (rows.data == 0).any()
