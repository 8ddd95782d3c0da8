"""AlternatingLeastSquares.explain / explain_batch on the device (csrc/explain.hip) against the float64 restatement
(tests/explain_reference.py) on the same inputs (tests/explain_cases.py).

Accuracy measures (the project's 1e-4, stated for this quantity): every contribution within 1e-4 x max |s| of its pair, every
total within 1e-4 x sum |s|; ids identical, a differing position excused only as a near-tie (the two items' float64
contributions within 2e-4 x max |s|), and at most 0.5 % of all compared positions excused.  The float32 twin of the restatement
stays within 1.8e-5 under both measures on these inputs and excuses nothing (tests/test_explain_host.py)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import explain_cases as cases
import explain_reference as ref

pytestmark = pytest.mark.gpu

BAR, EXCUSED = 1e-4, 0.005
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explain_golden.npz")


def model_for(gpu, Y, alpha=1.0, reg=cases.REG, dtype=np.float32):
    from implicit_amd.gpu.als import AlternatingLeastSquares

    model = AlternatingLeastSquares(factors=Y.shape[1], regularization=reg, alpha=alpha, dtype=dtype)
    model.item_factors = gpu.Matrix(np.ascontiguousarray(Y.astype(dtype)))
    return model


def check(got, want, label):
    total, ids, scores = got[:3]
    assert total.dtype == np.float32 and ids.dtype == np.int32 and scores.dtype == np.float32
    assert total.shape == want[0].shape and ids.shape == want[1].shape and scores.shape == want[2].shape
    m = ref.compare(total, ids, scores, want[0], want[1], want[2], want[3])
    print(label, m)
    assert m["contribution"] <= BAR, (label, m)
    assert m["total"] <= BAR, (label, m)
    assert m["unexcused"] == 0, (label, m)
    assert m["differing"] <= EXCUSED * m["positions"], (label, m)
    return m


@pytest.mark.parametrize("f,alpha", cases.ACCURACY)
def test_accuracy_at_every_factor_count(gpu, f, alpha):
    model = model_for(gpu, cases.factors(f), alpha)
    got = model.explain_batch(np.arange(300), cases.accuracy_matrix(), cases.accuracy_items(), N=10)
    check(got, cases.accuracy_reference(f, alpha), f"f={f} alpha={alpha}")


@pytest.mark.parametrize("f", [16, 100, 256])
@pytest.mark.parametrize("M,N", [(1, 1), (10, 10), (1, 300), (10, 300)])
def test_row_lengths_in_one_batch(gpu, f, M, N):
    user_items, names = cases.edge_matrix()
    model = model_for(gpu, cases.factors(f, cases.EDGE_ITEMS))
    got = model.explain_batch(np.arange(len(names)), user_items, cases.edge_items(M), N=N)
    check(got, cases.edge_reference(f, M, N), f"edges f={f} M={M} N={N}")
    total, ids, scores, _ = got
    neg = names.index("all_negative")
    assert (total[neg] == 0).all() and (ids[neg] == -1).all() and (scores[neg] == np.float32(-ref.FLT_MAX)).all()
    empty = names.index("len0")
    assert (total[empty] == 0).all() and (ids[empty] == -1).all()
    a, b = names.index("likes_40"), names.index("likes_40_again")  # the same user twice: column 0 explains the same item
    np.testing.assert_array_equal(ids[a, 0], ids[b, 0])
    np.testing.assert_array_equal(scores[a, 0], scores[b, 0])
    assert total[a, 0] == total[b, 0]
    if N >= 2:  # the tie: bit-equal scores, larger id first
        row = ids[names.index("tie"), 0].tolist()
        lo, hi = cases.TIE
        at = row.index(hi)
        assert row[at + 1] == lo
        assert scores[names.index("tie"), 0, at] == scores[names.index("tie"), 0, at + 1]


def test_factors_beyond_256_raise(gpu):
    Y = np.random.default_rng(1).uniform(-0.05, 0.05, size=(50, 260)).astype(np.float32)
    model = model_for(gpu, Y)
    user_items = cases.accuracy_matrix()[:4, :50]
    with pytest.raises(ValueError, match="256"):
        model.explain_batch(np.arange(4), user_items, [1, 2, 3, 4])
    # the library itself refuses too, before any launch
    solver = gpu.LeastSquaresSolver()
    with pytest.raises(ValueError, match="256"):
        solver.explain_factor(gpu.CSRMatrix(user_items), gpu.Matrix.zeros(260, 260), model.item_factors, 0.01,
                              gpu.Matrix.zeros(4 * 260, 260))
    with pytest.raises(ValueError, match="256"):
        solver.explain(gpu.CSRMatrix(user_items), model.item_factors, gpu.Matrix.zeros(4 * 260, 260),
                       gpu.IntVector(np.arange(4, dtype=np.int32)), 1, 10)


def test_same_call_twice_is_bit_identical(gpu):
    user_items, names = cases.edge_matrix()
    model = model_for(gpu, cases.factors(100, cases.EDGE_ITEMS))
    first = model.explain_batch(np.arange(len(names)), user_items, cases.edge_items(10), N=300)
    second = model.explain_batch(np.arange(len(names)), user_items, cases.edge_items(10), N=300)
    for a, b in zip(first[:3], second[:3]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(first[3].to_numpy(), second[3].to_numpy())


@pytest.mark.parametrize("f", [16, 128, 256])
def test_reused_weights(gpu, f):
    user_items, names = cases.edge_matrix()
    Y = cases.factors(f, cases.EDGE_ITEMS)
    model = model_for(gpu, Y)
    fresh = model.explain_batch(np.arange(len(names)), user_items, cases.edge_items(10), N=10)
    W = fresh[3]
    assert isinstance(W, gpu.Matrix) and W.shape == (len(names) * f, f)
    again = model.explain_batch(np.arange(len(names)), user_items, cases.edge_items(10), N=10, user_weights=W)
    assert again[3] is W
    for a, b in zip(fresh[:3], again[:3]):
        np.testing.assert_array_equal(a, b)
    L = W.to_numpy().astype(np.float64).reshape(len(names), f, f)
    for b in range(len(names)):
        assert (np.triu(L[b], 1) == 0).all(), names[b]
        lo, hi = user_items.indptr[b], user_items.indptr[b + 1]
        A = ref.normal_matrix(Y, user_items.indices[lo:hi], user_items.data[lo:hi], cases.REG)
        assert np.linalg.norm(L[b] @ L[b].T - A) <= 1e-5 * np.linalg.norm(A), names[b]


# ---- model level -----------------------------------------------------------------------------------------------------------------
def fit_model():
    from implicit_amd.gpu.als import AlternatingLeastSquares

    user_items = cases.accuracy_matrix()
    model = AlternatingLeastSquares(factors=16, regularization=0.05, alpha=2.0, iterations=5, use_cg=False, random_state=3)
    model.fit(user_items, show_progress=False)
    return model, user_items


@pytest.fixture(scope="module")
def fitted(gpu):
    return fit_model()


def test_explain_total_is_the_recalculated_recommendation(gpu, fitted):
    model, user_items = fitted
    for user in (0, 7, 123):
        ids, scores = model.recommend(user, user_items[user], N=3, recalculate_user=True)
        total, top, W = model.explain(user, user_items, int(ids[0]))
        assert abs(total - float(scores[0])) <= 1e-4
        assert abs(sum(s for _, s in top) - total) <= 1e-4 or len(top) == 10
        assert [s for _, s in top] == sorted((s for _, s in top), reverse=True)
        assert isinstance(W, gpu.Matrix) and W.shape == (16, 16)
        liked = user_items[user]
        positive = set(liked.indices[liked.data > 0].tolist())
        assert all(isinstance(i, int) and i in positive for i, _ in top) and len(top) == min(10, len(positive))
        again = model.explain(user, user_items, int(ids[0]), user_weights=W)
        assert again[0] == total and again[1] == top


def test_explain_is_row_0_of_explain_batch_and_honours_alpha(gpu, fitted):
    model, user_items = fitted
    user, item = 42, 17
    total, top, _ = model.explain(user, user_items, item, N=5)
    bt, bi, bs, _ = model.explain_batch([user], user_items[user], [item], N=5)
    assert bt.shape == (1, 1) and bi.shape == (1, 1, 5)
    assert total == float(bt[0, 0])
    assert top == [(int(i), float(s)) for i, s in zip(bi[0, 0], bs[0, 0]) if i >= 0]
    Y = model.item_factors.to_numpy()
    want = ref.explain_batch(Y, user_items[user], [[item]], model.regularization, 5, alpha=model.alpha)
    check((bt, bi, bs), want, "fitted, alpha=2")
    wrong = ref.explain_batch(Y, user_items[user], [[item]], model.regularization, 5, alpha=1.0)
    assert abs(float(wrong[0][0, 0]) - total) > 1e-3 * abs(total)  # alpha = 1 would be a different answer


def test_float16_model(gpu):
    Y16 = cases.factors(64).astype(np.float16)
    model = model_for(gpu, Y16, dtype=np.float16)
    assert model.item_factors.dtype == np.float16
    got = model.explain_batch(np.arange(300), cases.accuracy_matrix(), cases.accuracy_items(), N=10)
    want = ref.explain_batch(Y16.astype(np.float64), cases.accuracy_matrix(), cases.accuracy_items(), cases.REG, 10)
    check(got, want, "float16 storage")


def test_explanation_follows_partial_fit_items(gpu):
    model, user_items = fit_model()  # a model of its own: it is changed in place
    user, item = 5, 9
    before = model.explain(user, user_items, item)
    changed = sorted({int(before[1][0][0]), item})  # the best contributor and the explained item
    item_users = user_items.T.tocsr()
    model.partial_fit_items(changed, item_users[changed] * 3.0)
    after = model.explain(user, user_items, item)
    assert after[0] != before[0]
    want = ref.explain_batch(model.item_factors.to_numpy(), user_items[user], [[item]], model.regularization, 10, alpha=model.alpha)
    bt, bi, bs, _ = model.explain_batch([user], user_items[user], [item])
    check((bt, bi, bs), want, "after partial_fit_items")
    assert after[0] == float(bt[0, 0])


def test_ivf_model_forwards(gpu, fitted):
    from implicit_amd.ann.ivf import IVFModel

    model, user_items = fitted
    wrapped = IVFModel(model, nlist=8, nprobe=8)
    a, b = wrapped.explain(3, user_items, 11), model.explain(3, user_items, 11)
    assert a[0] == b[0] and a[1] == b[1]
    users = np.array([3, 9, 9])
    x = wrapped.explain_batch(users, user_items[users], [[11, 2], [5, 6], [5, 7]], N=4)
    y = model.explain_batch(users, user_items[users], [[11, 2], [5, 6], [5, 7]], N=4)
    for p, q in zip(x[:3], y[:3]):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(x[1][1, 0], x[1][2, 0])  # the same user and item twice in a batch


def test_golden_pairs_from_the_recorded_factors(gpu):
    g = np.load(GOLDEN)
    for i, text in enumerate(g["cases"]):
        case = json.loads(str(text))
        k, u = case["model"], case["user"]
        reg, alpha = g[f"m{k}_params"]
        user_items = sp.csr_matrix((g[f"m{k}_data"], g[f"m{k}_indices"], g[f"m{k}_indptr"]),
                                   shape=(len(g[f"m{k}_indptr"]) - 1, g[f"m{k}_Y"].shape[0]))
        model = model_for(gpu, g[f"m{k}_Y"], alpha=float(alpha), reg=float(reg))
        total, top, _ = model.explain(u, user_items, case["item"], N=case["N"])
        want_ids, want_scores = g[f"c{i}_ids"], g[f"c{i}_scores"]
        full = ref.explain_batch(g[f"m{k}_Y"], user_items[u], [[case["item"]]], reg, case["N"], alpha=alpha)[3]
        smax, ssum = np.abs(full[0][0][1]).max(), np.abs(full[0][0][1]).sum()
        assert abs(total - float(g[f"c{i}_total"])) <= BAR * ssum, case
        assert [t[0] for t in top] == want_ids.tolist(), case  # no near-ties among the recorded pairs
        assert np.abs(np.array([t[1] for t in top]) - want_scores).max() <= BAR * smax, case


# ---- error paths -----------------------------------------------------------------------------------------------------------------
def test_non_positive_pivot_names_the_user(gpu):
    model = model_for(gpu, cases.factors(16), reg=-1000.0)
    users = np.array([250, 251, 252])
    with pytest.raises(ValueError, match="user 250"):
        model.explain_batch(users, cases.accuracy_matrix()[users], [1, 2, 3])
    with pytest.raises(ValueError, match="user 7"):
        model.explain(7, cases.accuracy_matrix(), 3)


def test_argument_errors(gpu):
    model = model_for(gpu, cases.factors(16))
    user_items = cases.accuracy_matrix()[:3]
    with pytest.raises(ValueError, match="item id"):
        model.explain_batch([0, 1, 2], user_items, [1, cases.ITEMS, 3])
    with pytest.raises(ValueError, match="item id"):
        model.explain_batch([0, 1, 2], user_items, [1, -1, 3])
    with pytest.raises(ValueError):
        model.explain_batch([0, 1, 2], user_items, [1, 2, 3], N=0)
    with pytest.raises(ValueError, match="user_weights"):
        model.explain_batch([0, 1, 2], user_items, [1, 2, 3], user_weights=gpu.Matrix.zeros(16, 16))
    with pytest.raises(ValueError):
        model.explain_batch([0, 1], user_items, [1, 2])
    # the same through the C-ABI, which validates before it launches
    solver, C, Y = gpu.LeastSquaresSolver(), gpu.CSRMatrix(user_items), model.item_factors
    W = gpu.Matrix.zeros(3 * 16, 16)
    solver.explain_factor(C, model._YtY_unreg, Y, cases.REG, W)
    ids = gpu.IntVector(np.array([1, 2, 3], dtype=np.int32))
    with pytest.raises(ValueError, match="item id"):
        solver.explain(C, Y, W, gpu.IntVector(np.array([1, cases.ITEMS, 3], dtype=np.int32)), 1, 10)
    with pytest.raises(ValueError):
        solver.explain(C, Y, W, ids, 1, 0)
    with pytest.raises(ValueError, match="weights"):
        solver.explain(C, Y, gpu.Matrix.zeros(16, 16), ids, 1, 10)
    with pytest.raises(ValueError, match="itemids"):
        solver.explain(C, Y, W, ids, 2, 10)
    with pytest.raises(ValueError, match="weights"):
        solver.explain_factor(C, model._YtY_unreg, Y, cases.REG, gpu.Matrix.zeros(16, 16))
