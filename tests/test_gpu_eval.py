"""Ranking metrics on the device (csrc/evaluation.hip, implicit_amd.evaluation): the kernel against the host function that
shares its per-row arithmetic (imp_host_ranking_metrics), the accumulator's bookkeeping, and ranking_metrics_at_k end to end
against the numpy restatement (tests/evaluation_reference.py) driven by the same model's recommend().

Bars: integer-valued sums and per-row hits exactly.  Per-row doubles, device against host: both sides add at most K correctly
rounded terms in the same order, so at most K 2^-52 relative; measured on the MI355X they are bit-identical (the two sides run
the same accumulator code under -ffp-contract=off), and equality is what is asserted.  Totals against a differently ordered
sum of the same non-negative terms: 1e-12 relative (at most 2 n 2^-53, n <= 3000 here)."""
import numpy as np
import pytest
import scipy.sparse as sp

import evaluation_reference as er

pytestmark = pytest.mark.gpu

RTOL = 1e-12
USERS, ITEMS = 400, 300
DOUBLES = ("sum_ap", "sum_ndcg", "sum_auc")
INTEGERS = ("relevant", "pr_div", "total")


def check_sums(got, want):
    for name in INTEGERS:
        assert got[name] == want[name], (name, got[name], want[name])
    for name in DOUBLES:
        assert abs(got[name] - want[name]) <= RTOL * abs(want[name]), (name, got[name], want[name])


@pytest.fixture(scope="module")
def held_out():
    """400 x 300 held-out pattern: a quarter of the users holds nothing out, the others 1 .. 150 items."""
    rng = np.random.default_rng(9)
    lengths = np.where(np.arange(USERS) % 4 == 1, 0, rng.integers(1, 151, USERS))
    lengths[:4] = (1, 0, 150, 64)
    indices = np.concatenate([np.sort(rng.choice(ITEMS, size=n, replace=False)) for n in lengths]).astype(np.int32)
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(USERS, ITEMS))


def rows_for(K, n, seed):
    """n recommendation rows: user ids with gaps, repeats and no order (users without held-out items among them), ids with
    hits, misses and, in a third of the rows, a tail of -1 padding."""
    rng = np.random.default_rng(seed)
    userids = rng.integers(0, USERS, n).astype(np.int32)
    ids = np.stack([rng.permutation(ITEMS)[:K] for _ in range(n)]).astype(np.int32)
    for r in range(0, n, 3):
        ids[r, rng.integers(0, K):] = -1
    return ids, userids


@pytest.mark.parametrize("K", [1, 3, 10, 63, 64, 65, 100])
def test_kernel_equals_the_host_function(gpu, held_out, K):
    for n in (1, 63, 64, 65, 1000):
        ids, userids = rows_for(K, n, 1000 * K + n)
        want, want_rows = gpu.host_ranking_metrics(held_out, K, ids, userids, per_row=True)
        acc = gpu.RankingMetrics(held_out, K)
        rows = acc.add(ids, userids, per_row=True)
        got = acc.sums()
        worst = np.max(np.abs(rows - want_rows) / np.maximum(np.abs(want_rows), 1e-300))
        print(f"K={K} n={n}: worst per-row relative difference {worst:.3g}, sums {got}")
        assert np.array_equal(rows[:, 0], want_rows[:, 0])
        np.testing.assert_allclose(rows, want_rows, rtol=K * 2.0**-52, atol=0)
        assert np.array_equal(rows, want_rows)  # the stronger statement that holds: same code, same bits
        check_sums(got, want)
        assert got["total"] == (np.diff(held_out.indptr)[userids] > 0).sum()
        # a device Matrix of int32 bit patterns, as KnnQuery.topk_device hands it over, and an IntVector
        acc.reset()
        acc.add(gpu.Matrix(ids.view(np.float32)), gpu.IntVector(userids))
        assert acc.sums() == got


def test_accumulation_over_batches(gpu, held_out):
    K, n = 10, 200
    ids, userids = rows_for(K, n, 77)
    want = gpu.host_ranking_metrics(held_out, K, ids, userids)
    results = []
    for step in (1, 7, n):
        acc = gpu.RankingMetrics(held_out, K)
        for s in range(0, n, step):
            acc.add(ids[s:s + step], userids[s:s + step])
        results.append(acc.sums())
        check_sums(results[-1], want)
    for other in results[1:]:
        for name in INTEGERS:
            assert other[name] == results[0][name]
    # the same calls give the same bits; reset returns the handle to zero
    acc = gpu.RankingMetrics(held_out, K)
    for _ in range(2):
        for s in range(0, n, 7):
            acc.add(ids[s:s + 7], userids[s:s + 7])
        assert acc.sums() == results[1]
        acc.reset()
        assert acc.sums() == dict.fromkeys(INTEGERS + DOUBLES, 0.0)


def test_add_rejects_mismatched_arguments(gpu, held_out):
    acc = gpu.RankingMetrics(held_out, 5)
    with pytest.raises(ValueError):
        acc.add(np.zeros((3, 4), np.int32), np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        acc.add(np.zeros((3, 5), np.int32), np.zeros(2, np.int32))
    with pytest.raises(ValueError):
        gpu.RankingMetrics(held_out, 0)
    unsorted = held_out.copy()
    assert np.diff(held_out.indptr)[2] > 1
    unsorted.indices[held_out.indptr[2]:held_out.indptr[2] + 2] = held_out.indices[held_out.indptr[2]:held_out.indptr[2] + 2][::-1]
    with pytest.raises(ValueError):
        gpu.RankingMetrics(unsorted, 5)
    assert acc.sums()["total"] == 0.0


@pytest.fixture(scope="module")
def split():
    from implicit_amd.evaluation import train_test_split
    from implicit_amd.synthetic import synthetic_csr

    C = synthetic_csr(3000, 1200, 150_000, seed=4)
    train, test = train_test_split(C, train_percentage=0.8, random_state=7)
    return train.astype(np.float32), test.astype(np.float32)


def fitted(kind, train):
    if kind == "als":
        from implicit_amd.gpu.als import AlternatingLeastSquares

        model = AlternatingLeastSquares(factors=64, regularization=0.05, iterations=3, random_state=11)
    elif kind == "bpr":
        from implicit_amd.gpu.bpr import BayesianPersonalizedRanking

        model = BayesianPersonalizedRanking(factors=31, iterations=5, random_state=11)
    else:
        from implicit_amd.nearest_neighbours import CosineRecommender

        model = CosineRecommender(K=20)
    model.fit(train, show_progress=False)
    return model


@pytest.mark.parametrize("kind", ["als", "bpr", "cosine"])
def test_ranking_metrics_end_to_end(gpu, split, kind):
    from implicit_amd import evaluation as ev

    train, test = split
    model = fitted(kind, train.astype(np.float64) if kind == "cosine" else train)
    K = 10
    want = er.ranking_metrics_at_k(model, train, test, K, batch_size=1000)
    got = ev.ranking_metrics_at_k(model, train, test, K=K, show_progress=False)
    print(kind, "device", got, "restatement", want)
    assert set(got) == {"precision", "map", "ndcg", "auc"}
    assert got["precision"] == want["precision"] > 0
    for key in ("map", "ndcg", "auc"):
        assert abs(got[key] - want[key]) <= RTOL * abs(want[key]), (key, got[key], want[key])
    for batch_size in (256, 100_000):
        other = ev.ranking_metrics_at_k(model, train, test, K=K, show_progress=False, batch_size=batch_size)
        assert other["precision"] == got["precision"]
        for key in ("map", "ndcg", "auc"):
            assert abs(other[key] - got[key]) <= RTOL * abs(got[key]), (key, batch_size, other[key], got[key])
    if kind == "als":
        assert ev.precision_at_k(model, train, test, K=K, show_progress=False) == got["precision"]
        assert ev.mean_average_precision_at_k(model, train, test, K=K, show_progress=False) == got["map"]
        assert ev.ndcg_at_k(model, train, test, K=K, show_progress=False) == got["ndcg"]
        assert ev.AUC_at_k(model, train, test, K=K, show_progress=False) == got["auc"]
        # an unsorted test matrix means the same
        order = np.arange(test.nnz)
        for u in range(0, test.shape[0], 2):
            order[test.indptr[u]:test.indptr[u + 1]] = order[test.indptr[u]:test.indptr[u + 1]][::-1]
        messy = sp.csr_matrix((test.data[order], test.indices[order], test.indptr), shape=test.shape)
        assert not messy.has_sorted_indices
        assert ev.ranking_metrics_at_k(model, train, messy, K=K, show_progress=False) == got
        for bad in (0, test.shape[1] + 1):
            with pytest.raises(ValueError):
                ev.ranking_metrics_at_k(model, train, test, K=bad, show_progress=False)
