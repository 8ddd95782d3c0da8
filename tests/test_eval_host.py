"""Host-only checks of implicit_amd.evaluation: the shared per-row arithmetic through imp_host_ranking_metrics (plain host
code in libimplicit_hip.so, no device) against the reference's recorded results (tests/golden/eval_golden.npz) and the numpy
restatement (tests/evaluation_reference.py); the canonical form of the held-out pattern; the two splitters.

Bars: integer-valued sums and per-row hits exactly; totals against a differently ordered sum of the same non-negative terms
1e-12 relative (two orders differ by at most 2 n 2^-53 relative, n <= 2000 here)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import evaluation_reference as er

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "eval_golden.npz")
RTOL = 1e-12
KS = (1, 3, 10, 64, 65, 100)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def host():
    from implicit_amd import _build
    from implicit_amd.gpu import _cuda, _hip

    if not os.path.exists(_hip.LIB_PATH):
        _build.build(verbose=False)
    return _cuda.host_ranking_metrics


def pattern(g, name):
    n = len(g[name + "_indices"])
    return sp.csr_matrix((np.ones(n), g[name + "_indices"], g[name + "_indptr"]), shape=tuple(g[name + "_shape"]))


def check_sums(got, want):
    for name in ("relevant", "pr_div", "total"):
        assert got[name] == want[name], name
    for name in ("sum_ap", "sum_ndcg", "sum_auc"):
        assert abs(got[name] - want[name]) <= RTOL * abs(want[name]), (name, got[name], want[name])


def test_golden_cases_cover_the_issue(golden):
    assert tuple(int(golden[n + "_K"]) for n in golden["names"]) == KS
    for name in golden["names"]:
        K, ids = int(golden[name + "_K"]), golden[name + "_ids"]
        test = pattern(golden, name)
        users, items = test.shape
        assert (users, items) == (150, 257) and ids.shape == (users, K) and ids.dtype == np.int32
        lengths = np.diff(test.indptr)
        assert (lengths == 0).sum() == users // 3
        assert {1, max(K - 1, 1), K, K + 1, 200} <= set(lengths.tolist())
        hits = np.array([np.isin(ids[u], test[u].indices).sum() for u in range(users)])
        assert hits[0] == K and hits[1] == 0 and lengths[1] > 0
        likes3 = test[3].indices
        assert likes3[-1] == items - 1 and ids[3, -1] == items - 1 and (K == 1 or ids[3, 0] == likes3[0])
        assert (ids[4, 1:] == -1).all() and (ids == -1).any(axis=1).sum() > 1


@pytest.mark.parametrize("K", KS)
def test_host_metrics_equal_the_reference(golden, host, K):
    name = f"K{K}"
    test, ids = pattern(golden, name), golden[name + "_ids"]
    users = np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)
    sums, per_row = host(test, K, ids[users], users, per_row=True)
    got = er.finish(sums)
    want = dict(zip(("precision", "map", "ndcg", "auc"), golden[name + "_result"]))
    for key in want:
        assert abs(got[key] - want[key]) <= RTOL * abs(want[key]), (key, got[key], want[key])
    # every user at once, the empty ones included: they add nothing
    all_sums = host(test, K, ids, np.arange(test.shape[0], dtype=np.int32))
    assert all_sums == sums
    # and the numpy restatement, per row too
    ref_sums, ref_rows = er.metrics(test, ids[users], users, K)
    check_sums(sums, ref_sums)
    assert np.array_equal(per_row[:, 0], ref_rows[:, 0])
    np.testing.assert_allclose(per_row[:, 1:], ref_rows[:, 1:], rtol=RTOL, atol=0)


@pytest.mark.parametrize("K,wide", [(1, False), (7, True), (64, False), (65, True), (130, False),
                                    # the K the device tests compare the kernel with this function at (tests/test_gpu_eval.py)
                                    (2, False), (5, True), (8, False), (17, True), (32, False), (128, True), (129, False),
                                    (200, True)])
def test_host_metrics_equal_numpy_on_random_input(host, K, wide):
    rng = np.random.default_rng(100 + K)
    users, items, n = 300, 211, 700
    test = sp.random(users, items, density=0.08, random_state=np.random.RandomState(K), format="csr")
    test = sp.csr_matrix(sp.diags((np.arange(users) % 5 != 0).astype(float)) @ test)  # every fifth user holds nothing out
    test.eliminate_zeros()
    test.sort_indices()
    if wide:
        test.indptr = test.indptr.astype(np.int64)  # 64-bit offsets beside 32-bit column ids
        assert test.indptr.dtype == np.int64 and test.indices.dtype == np.int32
    userids = rng.integers(0, users, n).astype(np.int32)  # repeats, any order, empty rows among them
    ids = rng.integers(-1, items + 3, (n, K)).astype(np.int32)  # -1 and ids >= items are misses
    sums, per_row = host(test, K, ids, userids, per_row=True)
    ref_sums, ref_rows = er.metrics(test, ids, userids, K)
    check_sums(sums, ref_sums)
    assert np.array_equal(per_row[:, 0], ref_rows[:, 0])
    np.testing.assert_allclose(per_row[:, 1:], ref_rows[:, 1:], rtol=RTOL, atol=0)
    assert sums["total"] == (np.diff(test.indptr)[userids] > 0).sum() < n


def test_host_metrics_reject_bad_input(host):
    ids, users = np.zeros((1, 2), np.int32), np.zeros(1, np.int32)

    def csr(indices, indptr, cols=5):
        return sp.csr_matrix((np.ones(len(indices)), np.array(indices, np.int32), np.array(indptr, np.int32)), shape=(2, cols))

    with pytest.raises(ValueError, match="strictly increasing"):
        host(csr([3, 1], [0, 2, 2]), 2, ids, users)  # unsorted
    with pytest.raises(ValueError, match="strictly increasing"):
        host(csr([1, 1], [0, 2, 2]), 2, ids, users)  # duplicate
    bad = csr([1, 4], [0, 2, 2])
    bad.indices[1] = 5
    with pytest.raises(ValueError, match="out of range"):
        host(bad, 2, ids, users)
    with pytest.raises(ValueError):
        host(csr([1, 4], [0, 2, 2]), 0, np.zeros((1, 0), np.int32), users)
    good = csr([1, 4], [0, 2, 2])
    for u in (-1, 2):
        with pytest.raises(IndexError):
            host(good, 2, ids, np.array([u], np.int32))
    assert host(good, 2, ids, users)["total"] == 1.0


def test_canonical_pattern_has_the_reference_meaning(host):
    """Duplicates count once, the order of a row does not matter, an explicit zero is a like."""
    from implicit_amd.evaluation import _canonical_pattern

    indptr = np.array([0, 4, 4, 7], np.int32)
    indices = np.array([5, 2, 5, 0, 3, 1, 3], np.int32)
    data = np.array([1.0, 0.0, 2.0, 1.0, -1.0, 1.0, 1.0])  # item 2 of user 0 is an explicit zero; item 3 of user 2 sums to zero
    raw = sp.csr_matrix((data, indices, indptr), shape=(3, 6))
    canon = _canonical_pattern(raw)
    assert canon.indptr.tolist() == [0, 3, 3, 5] and canon.indices.tolist() == [0, 2, 5, 1, 3]
    assert raw.indices.tolist() == indices.tolist() and raw.nnz == 7  # the caller's matrix is untouched
    ids = np.array([[2, 4, 5], [3, 0, 1]], np.int32)
    users = np.array([0, 2], np.int32)
    sums, rows = host(canon, 3, ids, users, per_row=True)
    want, want_rows = er.metrics(raw, ids, users, 3)
    check_sums(sums, want)
    assert rows[:, 0].tolist() == [2.0, 2.0] and sums["pr_div"] == 5.0
    np.testing.assert_allclose(rows, want_rows, rtol=RTOL, atol=0)
    with pytest.raises(ValueError):
        host(raw, 3, ids, users)


def test_train_test_split_equals_the_reference(golden):
    from implicit_amd.evaluation import train_test_split

    def csr(prefix):
        return sp.csr_matrix((golden[prefix + "_data"], golden[prefix + "_indices"], golden[prefix + "_indptr"]),
                             shape=tuple(golden[prefix + "_shape"]))

    m = csr("split_in")
    assert (m.data < 0).any()
    train, test = train_test_split(m, 0.8, random_state=7)
    for got, want in ((train, csr("split_train")), (test, csr("split_test"))):
        assert isinstance(got, sp.csr_matrix) and got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert np.array_equal(got.data, want.data)
    assert (test.data > 0).all() and (train + test).nnz < m.nnz  # negative held-out values were dropped


@pytest.mark.parametrize("K,train_only", [(1, 0.0), (3, 0.0), (2, 0.4)])
def test_leave_k_out_split_properties(K, train_only):
    from implicit_amd.evaluation import leave_k_out_split

    m = sp.random(200, 60, density=0.1, random_state=np.random.RandomState(3), format="csr")
    m.data = np.ceil(m.data * 5)
    train, test = leave_k_out_split(m, K=K, train_only_size=train_only, random_state=11)
    assert isinstance(train, sp.csr_matrix) and isinstance(test, sp.csr_matrix)
    assert abs(train + test - m).nnz == 0 and train.nnz + test.nnz == m.nnz
    counts, held = np.diff(m.indptr), np.diff(test.indptr)
    assert set(held.tolist()) == {0, K}
    assert (counts[held > 0] > K + 1).all()
    eligible = (counts > K + 1).sum()
    if train_only == 0.0:
        assert (held > 0).sum() == eligible
    else:
        kept_out = eligible - (held > 0).sum()
        assert 0 < kept_out <= max(1, int((counts > 0).sum() * train_only))
    again = leave_k_out_split(m, K=K, train_only_size=train_only, random_state=11)
    assert abs(again[1] - test).nnz == 0 and abs(again[0] - train).nnz == 0
    other = leave_k_out_split(m, K=K, train_only_size=train_only, random_state=12)
    assert abs(other[1] - test).nnz > 0


def test_leave_k_out_split_rejects_bad_arguments():
    from implicit_amd.evaluation import leave_k_out_split

    m = sp.identity(4, format="csr")
    with pytest.raises(ValueError):
        leave_k_out_split(m, K=0)
    with pytest.raises(ValueError):
        leave_k_out_split(m, train_only_size=1.0)
