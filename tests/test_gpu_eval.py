"""Ranking metrics on the device (csrc/evaluation.hip, implicit_amd.evaluation): the kernel against the host function that
shares its per-row arithmetic (imp_host_ranking_metrics), the accumulator's bookkeeping, and ranking_metrics_at_k end to end
against the numpy restatement (tests/evaluation_reference.py) driven by the same model's recommend().

Bars: integer-valued sums and per-row hits exactly.  Per-row doubles, device against host: both sides add at most K correctly
rounded terms in the same order, so at most K 2^-52 relative; measured on the MI355X they are bit-identical (the two sides run
the same accumulator code under -ffp-contract=off), and equality is what is asserted.  Totals against a differently ordered
sum of the same non-negative terms: 1e-12 relative (at most 2 n 2^-53, n <= 3000 here); the tests with more rows use
2 n 2^-53 itself (6e-11 at n = 262 147).  Per-row doubles against the numpy restatement, which adds the same terms in
another order: K 2^-52 as well."""
import numpy as np
import pytest
import scipy.sparse as sp

import evaluation_reference as er
import sgd_cases as sc

pytestmark = pytest.mark.gpu

RTOL = 1e-12
USERS, ITEMS = 400, 300
WIDE_ITEMS = ITEMS + 260  # the pattern for K > 100
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


@pytest.fixture(scope="module")
def held_out_wide():
    """The same with 560 items, for K up to 200: the users hold out 1 .. 280 items."""
    rng = np.random.default_rng(10)
    lengths = np.where(np.arange(USERS) % 4 == 1, 0, rng.integers(1, 281, USERS))
    lengths[:4] = (1, 0, 280, 200)
    indices = np.concatenate([np.sort(rng.choice(WIDE_ITEMS, size=n, replace=False)) for n in lengths]).astype(np.int32)
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(USERS, WIDE_ITEMS))


KS = [1, 3, 10, 63, 64, 65, 100] + sc.EVAL_NEW_K  # G = 1, 4, 16, 64 lanes per row; the new ones 2, 8, 8, 32, 32, 64, 64, 64


def pattern_for(K, held_out, held_out_wide):
    return held_out if K <= 100 else held_out_wide


def rows_for(K, n, seed, items=ITEMS):
    """n recommendation rows: user ids with gaps, repeats and no order (users without held-out items among them), ids with
    hits, misses and, in a third of the rows, a tail of -1 padding."""
    rng = np.random.default_rng(seed)
    userids = rng.integers(0, USERS, n).astype(np.int32)
    ids = np.stack([rng.permutation(items)[:K] for _ in range(n)]).astype(np.int32)
    for r in range(0, n, 3):
        ids[r, rng.integers(0, K):] = -1
    return ids, userids


def many_rows_for(K, n, seed, items=ITEMS):
    """rows_for for tens of thousands of rows: ids drawn with repeats from -1 .. items + 2 (a negative id and one past the
    catalogue are misses); the rows of the last two tiles belong to users who hold something out."""
    rng = np.random.default_rng(seed)
    userids = rng.integers(0, USERS, n).astype(np.int32)
    userids[-512:] = 4 * rng.integers(0, USERS // 4, 512)  # users 0, 4, 8, ...: never the empty ones (1 mod 4)
    ids = rng.integers(-1, items + 3, (n, K)).astype(np.int32)
    return ids, userids


@pytest.mark.parametrize("K", KS)
def test_kernel_equals_the_host_function(gpu, held_out, held_out_wide, K):
    held_out = pattern_for(K, held_out, held_out_wide)
    assert held_out.shape[1] >= K
    for n in (1, 63, 64, 65, 1000):
        ids, userids = rows_for(K, n, 1000 * K + n, held_out.shape[1])
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


@pytest.mark.parametrize("K", KS)
def test_kernel_equals_numpy(gpu, held_out, held_out_wide, K):
    """The device against the numpy restatement directly, not through the host function that shares its accumulator."""
    held_out = pattern_for(K, held_out, held_out_wide)
    for n in (1, 65, 1000):
        ids, userids = rows_for(K, n, 2000 * K + n, held_out.shape[1])
        want, want_rows = er.metrics(held_out, ids, userids, K)
        acc = gpu.RankingMetrics(held_out, K)
        rows = acc.add(ids, userids, per_row=True)
        worst = np.max(np.abs(rows - want_rows) / np.maximum(np.abs(want_rows), 1e-300))
        print(f"K={K} n={n}: worst per-row relative difference to numpy {worst:.3g} (bound {K * 2.0**-52:.3g})")
        assert np.array_equal(rows[:, 0], want_rows[:, 0])
        np.testing.assert_allclose(rows, want_rows, rtol=K * 2.0**-52, atol=0)
        check_sums(acc.sums(), want)


def check_many(got, want, n):
    """Integer sums exactly; double sums of non-negative terms in two orders: 2 n 2^-53 relative."""
    for name in INTEGERS:
        assert got[name] == want[name], (name, got[name], want[name])
    for name in DOUBLES:
        assert abs(got[name] - want[name]) <= 2 * n * 2.0**-53 * abs(want[name]), (name, got[name], want[name])


@pytest.mark.parametrize("n, K", sc.EVAL_ROUND_SHAPES)
def test_second_tile_round_and_long_fold(gpu, held_out, n, K):
    """More workgroups than eval_fold_kernel has threads (258 slots: its `j += 256` takes a second step), and more tiles than
    the grid has workgroups (1025 or 1026 on 1024: `tile += gridDim.x` takes a second step and the register sum is carried
    over), at 64, 16 and 1 lanes per row and at one and three chunks per row.  sgd_cases.EVAL_ROUND_SHAPES lists the counts."""
    G, tiles, slots = sc.eval_launch(n, K)
    assert slots > 256  # which steps each shape takes: tests/test_sgd_cases_host.py
    ids, userids = many_rows_for(K, n, 31 * n + K)
    want, want_rows = gpu.host_ranking_metrics(held_out, K, ids, userids, per_row=True)
    acc = gpu.RankingMetrics(held_out, K)
    rows = acc.add(ids, userids, per_row=True)
    got = acc.sums()
    print(f"n={n} K={K}: G {G}, {tiles} tiles, {slots} slots, sums {got}")
    assert np.array_equal(rows, want_rows)
    check_many(got, want, n)
    live = np.diff(held_out.indptr)[userids] > 0
    assert got["total"] == live.sum() and live[-2 * (256 // G):].all()  # the rows of the last two tiles count
    # without them the total falls by exactly their number: they were in it
    cut = n - 2 * (256 // G)
    acc.reset()
    acc.add(ids[:cut], userids[:cut])
    assert acc.sums()["total"] == got["total"] - 2 * (256 // G)


def test_slots_are_not_read_past_the_grid(gpu, held_out):
    """4101 rows fill all 1024 slots of the handle's workspace; the next add of 3 rows writes one slot and must fold one."""
    K = 64
    ids, userids = many_rows_for(K, 4104, 5)
    want = gpu.host_ranking_metrics(held_out, K, ids, userids)
    acc = gpu.RankingMetrics(held_out, K)
    acc.add(ids[:4101], userids[:4101])
    acc.add(ids[4101:], userids[4101:])
    check_many(acc.sums(), want, 4104)
    assert want["total"] > 3000 and want["relevant"] > 0


def test_ids_outside_the_matrices_add_nothing(gpu, held_out):
    """User ids -1 and `rows` give a zero record and add nothing; item ids >= cols and negative ids other than -1 are misses."""
    K, n = 10, 300
    rng = np.random.default_rng(12)
    ids, userids = rows_for(K, n, 99)
    ids[rng.random(ids.shape) < 0.1] = ITEMS
    ids[rng.random(ids.shape) < 0.1] = ITEMS + 7
    ids[rng.random(ids.shape) < 0.1] = -2
    ids[rng.random(ids.shape) < 0.05] = np.iinfo(np.int32).min
    ids[rng.random(ids.shape) < 0.05] = np.iinfo(np.int32).max
    outside = np.zeros(n, dtype=bool)
    outside[[0, 5, 17, 64, 65, 255, 256, n - 1]] = True
    userids[outside] = np.where(np.arange(outside.sum()) % 2 == 0, -1, USERS)
    want, want_rows = er.metrics(held_out, ids[~outside], userids[~outside], K)
    acc = gpu.RankingMetrics(held_out, K)
    rows = acc.add(ids, userids, per_row=True)
    got = acc.sums()
    assert not rows[outside].any()
    assert np.array_equal(rows[~outside][:, 0], want_rows[:, 0])
    np.testing.assert_allclose(rows[~outside], want_rows, rtol=K * 2.0**-52, atol=0)
    check_sums(got, want)
    assert got["total"] == (np.diff(held_out.indptr)[userids[~outside]] > 0).sum() > 0
    # rows of users outside the matrix alone leave the sums as they are
    acc.add(ids[outside], userids[outside])
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
