"""The native IVF-Flat index (csrc/ivf.hip, implicit_amd.gpu.IVFIndex) against the float64 restatement in ivf_reference.py.

Where ids are compared with a float64 result, a mismatch is accepted only as a near-tie by the rule of smoke(): the float64
score of the id that came back equals the expected score at that position within 4 f 2^-23 relative (ivf_reference.audit).
Scores are compared with rtol = 1e-4, atol = 1e-7.  Where a cap is stated, at most 1 % of the compared positions may be such
exceptions."""
import numpy as np
import pytest

import ivf_reference as ref

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
_cache = {}


def _lists(ix):
    return ix.centroids, ix.list_offsets, ix.list_ids


def _assign_of(offsets, ids):
    assign = np.empty(len(ids), dtype=np.int64)
    for l in range(len(offsets) - 1):
        assign[ids[offsets[l]:offsets[l + 1]]] = l
    return assign


def _check_scores(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-7)


def _check_search(vectors, queries, got_ids, got_scores, want_ids, want_scores, cap=None):
    """ids audited against the float64 result, scores within tolerance; returns the number of near-tie exceptions."""
    v64, q64 = np.asarray(vectors, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    f = v64.shape[1]
    assert got_ids.shape == want_ids.shape and got_scores.shape == want_scores.shape
    assert ((got_ids < 0) == (want_ids < 0)).all()
    exceptions = ref.audit(got_ids, want_ids, want_scores, lambda r, i: v64[i] @ q64[r], f)
    _check_scores(got_scores, want_scores)
    if cap is not None:
        assert exceptions <= cap * got_ids.size, f"{exceptions} near-tie exceptions among {got_ids.size} positions"
    return exceptions


def _check_probes(centroids, queries, probes, cap=None):
    c64, q64 = np.asarray(centroids, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    coarse = q64 @ c64.T
    want = np.stack([ref.order_desc(row)[:probes.shape[1]] for row in coarse])
    want_scores = np.take_along_axis(coarse, want, axis=1)
    exceptions = ref.audit(probes, want, want_scores, lambda r, l: coarse[r, l], c64.shape[1])
    if cap is not None:
        assert exceptions <= cap * probes.size
    return exceptions


def _random_index(gpu, n, f, nlist, seed, dtype=np.float32, iterations=10):
    key = (n, f, nlist, seed, np.dtype(dtype).name, iterations)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        vectors = rng.standard_normal((n, f)).astype(dtype)
        init = rng.choice(n, size=nlist, replace=False)
        _cache[key] = (vectors, init, gpu.IVFIndex.build(vectors, nlist, iterations, init_rows=init))
    return _cache[key]


# ---- 1. build invariants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f,nlist,dtype", [(5000, 30, 37, np.float32), (4096, 128, 64, np.float16)])
def test_build_invariants(gpu, n, f, nlist, dtype):
    vectors, _, ix = _random_index(gpu, n, f, nlist, seed=11, dtype=dtype)
    assert ix.shape == (n, f) and ix.nlist == nlist
    centroids, offsets, ids = _lists(ix)
    assert centroids.shape == (nlist, f) and not np.isnan(centroids).any()
    assert offsets[0] == 0 and offsets[-1] == n and (np.diff(offsets) >= 0).all()
    np.testing.assert_array_equal(np.sort(ids), np.arange(n))
    for l in range(nlist):
        assert (np.diff(ids[offsets[l]:offsets[l + 1]]) > 0).all()
    norms = np.linalg.norm(centroids.astype(np.float64), axis=1)
    zero = ~centroids.any(axis=1)
    assert (np.abs(norms[~zero] - 1.0) < 1e-5).all()
    # every vector sits in the list of its best final centroid (float64 argmax, audited)
    scores = vectors.astype(np.float64) @ centroids.astype(np.float64).T
    want = ref.argmax_rows(scores)
    got = _assign_of(offsets, ids)
    best = scores[np.arange(n), want]
    exceptions = ref.audit(got[:, None], want[:, None], best[:, None], lambda r, l: scores[r, l], f)
    assert exceptions <= 0.01 * n


# ---- 2. k-means against the reference ----------------------------------------------------------------------------------
def test_kmeans_matches_reference(gpu):
    n, f, nlist, iterations = 4096, 64, 16, 5
    rng = np.random.default_rng(5)
    directions = np.linalg.qr(rng.standard_normal((f, f)))[0][:nlist]  # 16 orthonormal directions
    planted = np.arange(n) % nlist
    vectors = (directions[planted] + 0.05 * rng.standard_normal((n, f))).astype(np.float32)
    init = np.arange(nlist)  # row c belongs to planted cluster c
    history = []
    want_cent, want_assign = ref.kmeans(vectors, init, iterations, history=history)
    assert len(history) == iterations + 1
    for _, margin in history:
        assert margin.min() > 1e-3  # no fp32 rounding can flip an assignment
    ix = gpu.IVFIndex.build(vectors, nlist, iterations, init_rows=init)
    centroids, offsets, ids = _lists(ix)
    np.testing.assert_array_equal(_assign_of(offsets, ids), want_assign)
    assert np.linalg.norm(centroids - want_cent) / np.linalg.norm(want_cent) < 1e-4


# ---- 3. the scan against the index's own lists -----------------------------------------------------------------------
@pytest.mark.parametrize("f", [64, 100])
@pytest.mark.parametrize("q", [1, 70])
@pytest.mark.parametrize("k", [10, 200])
def test_scan_against_own_lists(gpu, f, q, k):
    n, nlist, nprobe = 3000, 24, 5
    vectors, _, ix = _random_index(gpu, n, f, nlist, seed=21)
    queries = np.random.default_rng(100 + f).standard_normal((70, f)).astype(np.float32)[:q]
    ids, scores, probes = ix.search(queries, k, nprobe, return_probes=True)
    assert ids.shape == (q, k) and scores.shape == (q, k) and probes.shape == (q, nprobe)
    assert ids.dtype == np.int32 and scores.dtype == np.float32 and probes.dtype == np.int32
    centroids, offsets, list_ids = _lists(ix)
    _check_probes(centroids, queries, probes, cap=0.01)
    _, want_ids, want_scores = ref.search(centroids, offsets, list_ids, vectors, queries, k, nprobe, probes=probes)
    _check_search(vectors, queries, ids, scores, want_ids, want_scores, cap=0.01)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------
def test_duplicates_and_empty_lists(gpu):
    rng = np.random.default_rng(2)
    distinct = rng.standard_normal((5, 24)).astype(np.float32)
    vectors = distinct[np.arange(50) % 5]
    init = rng.choice(50, size=16, replace=False)
    ix = gpu.IVFIndex.build(vectors, 16, 10, init_rows=init)
    centroids, offsets, ids = _lists(ix)
    assert not np.isnan(centroids).any()
    assert (np.diff(offsets) == 0).any() and offsets[-1] == 50
    got_ids, got_scores = ix.search(distinct, 20, 16)
    want_ids, want_scores = ref.brute_force(vectors, distinct, 20)
    _check_search(vectors, distinct, got_ids, got_scores, want_ids, want_scores)
    bits = got_scores.view(np.uint32)
    for r in range(5):
        for a in range(20):
            for b in range(a + 1, 20):
                if got_ids[r, a] % 5 == got_ids[r, b] % 5:  # the same vector: the same bits, the larger id first
                    assert bits[r, a] == bits[r, b] and got_ids[r, a] > got_ids[r, b]


def test_zero_rows(gpu):
    rng = np.random.default_rng(8)
    vectors = rng.standard_normal((2000, 20)).astype(np.float32)
    zero_rows = rng.choice(2000, size=400, replace=False)
    vectors[zero_rows] = 0
    nlist = 10
    init = np.concatenate([zero_rows[:1], np.setdiff1d(np.arange(2000), zero_rows)[:nlist - 1]])
    ix = gpu.IVFIndex.build(vectors, nlist, 4, init_rows=init)
    centroids, offsets, ids = _lists(ix)
    assert not np.isnan(centroids).any()
    norms = np.linalg.norm(centroids.astype(np.float64), axis=1)
    assert ((np.abs(norms - 1) < 1e-5) | (norms == 0)).all()
    assign = _assign_of(offsets, ids)
    assert (assign[zero_rows] == nlist - 1).all()  # every score ties at zero: the larger list id
    got_ids, got_scores = ix.search(vectors[:64], 10, nlist)
    assert not np.isnan(got_scores).any()
    want_ids, want_scores = ref.brute_force(vectors, vectors[:64], 10)
    _check_search(vectors, vectors[:64], got_ids, got_scores, want_ids, want_scores)


def test_select_when_the_far_tail_does_not_fit_in_lds(gpu):
    """ivf_select_kernel with its radix select on the score segments themselves: every score is an integer in [1024, 1280),
    so all 3 000 keys share sign, exponent and the two top mantissa bits -- one bucket of the 11-bit histogram, more than the
    2 048 keys the LDS copy holds (a condition on the scores alone; nothing at run time reports it).  Scores are exact in fp32
    and full of ties: ids and scores equal the float64 brute force under (score desc, id desc), no near-tie exceptions."""
    rng = np.random.default_rng(17)
    n, f = 3000, 8
    vectors = rng.integers(-20, 21, size=(n, f)).astype(np.float32)
    vectors[:, 0] = rng.integers(1100, 1200, size=n)
    queries = np.zeros((3, f), dtype=np.float32)
    queries[:, 0] = 1
    queries[0, 1], queries[1, 2], queries[2, 3] = 1, -1, 2   # scores v0 + v1, v0 - v2, v0 + 2 v3: within [1060, 1240)
    scores = vectors.astype(np.float64) @ queries.astype(np.float64).T
    assert (scores == np.round(scores)).all() and scores.min() >= 1024 and scores.max() < 1280
    ix = gpu.IVFIndex.build(vectors, 4, 4, init_rows=np.array([0, 1, 2, 3]))
    got_ids, got_scores = ix.search(queries, 10, 4)
    want_ids, want_scores = ref.brute_force(vectors, queries, 10)
    np.testing.assert_array_equal(got_ids, want_ids)
    np.testing.assert_array_equal(got_scores, want_scores.astype(np.float32))
    assert any(len(set(row)) < len(row) for row in want_scores)  # (ties among the winners)


@pytest.fixture(scope="module")
def lopsided(gpu):
    """6000 vectors in 6 planted clusters: one of 3500, one of a single vector."""
    rng = np.random.default_rng(13)
    f = 32
    directions = np.linalg.qr(rng.standard_normal((f, f)))[0][:6]
    planted = np.concatenate([np.zeros(3500, dtype=int), np.full(1, 1), 2 + np.arange(2499) % 4])
    vectors = (directions[planted] + 0.05 * rng.standard_normal((6000, f))).astype(np.float32)
    init = np.array([np.flatnonzero(planted == c)[0] for c in range(6)])
    ix = gpu.IVFIndex.build(vectors, 6, 3, init_rows=init)
    return vectors, planted, ix


def test_long_and_single_vector_lists(gpu, lopsided):
    vectors, planted, ix = lopsided
    centroids, offsets, ids = _lists(ix)
    sizes = np.diff(offsets)
    assert sizes.max() > 3000 and (sizes == 1).any()
    queries = vectors[[0, 3500, 3501, 5999, 17, 4000]]
    got_ids, got_scores = ix.search(queries, 10, 6)
    want_ids, want_scores = ref.brute_force(vectors, queries, 10)
    _check_search(vectors, queries, got_ids, got_scores, want_ids, want_scores)
    got_ids, got_scores, probes = ix.search(queries, 50, 2, return_probes=True)
    _check_probes(centroids, queries, probes)
    _, want_ids, want_scores = ref.search(centroids, offsets, ids, vectors, queries, 50, 2, probes=probes)
    _check_search(vectors, queries, got_ids, got_scores, want_ids, want_scores)


def test_k_beyond_the_probed_lists(gpu, lopsided):
    vectors, planted, ix = lopsided
    single = int(np.flatnonzero(planted == 1)[0])
    got_ids, got_scores = ix.search(vectors[single:single + 1], 10, 1)
    assert got_ids[0, 0] == single
    assert (got_ids[0, 1:] == -1).all() and (got_scores[0, 1:] == -FLT_MAX).all()
    assert got_scores[0, 0] == pytest.approx(float(vectors[single].astype(np.float64) @ vectors[single]), rel=1e-4)


def test_nprobe_is_clamped_and_arguments_checked(gpu, lopsided):
    vectors, _, ix = lopsided
    queries = vectors[::500]
    a = ix.search(queries, 10, 1000, return_probes=True)
    b = ix.search(queries, 10, ix.nlist, return_probes=True)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    with pytest.raises(ValueError):
        ix.search(queries, 0, 2)
    with pytest.raises(ValueError):
        ix.search(queries, 10, 0)
    with pytest.raises(ValueError):
        ix.search(queries, 1025, 2)
    with pytest.raises(ValueError):
        ix.search(queries[:, :5], 10, 2)


def test_chunked_search_changes_nothing(gpu):
    n, f, nlist, nprobe, k, q = 3000, 64, 24, 5, 10, 70
    vectors, _, ix = _random_index(gpu, n, f, nlist, seed=21)
    queries = np.random.default_rng(77).standard_normal((q, f)).astype(np.float32)
    whole = ix.search(queries, k, nprobe, return_probes=True)
    # a query's share of the budget is at least 4 bytes for each vector of the nprobe longest lists, which hold at least
    # nprobe * n / nlist vectors: 64 KiB fit at most 26 queries, so the 70 take three chunks or more
    budget = 64 << 10
    assert budget // (4 * (nprobe * n // nlist)) < q // 2
    ix.set_temp_memory(budget)
    try:
        chunked = ix.search(queries, k, nprobe, return_probes=True)
    finally:
        ix.set_temp_memory(0)
    for x, y in zip(whole, chunked):
        assert x.tobytes() == y.tobytes()
    centroids, offsets, list_ids = _lists(ix)
    _, want_ids, want_scores = ref.search(centroids, offsets, list_ids, vectors, queries, k, nprobe, probes=chunked[2])
    _check_search(vectors, queries, chunked[0], chunked[1], want_ids, want_scores)


# ---- 5. / 6. exactness at full probe, monotone recall ------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_probe(gpu):
    n, f, nlist, q = 8000, 128, 32, 300
    vectors, _, ix = _random_index(gpu, n, f, nlist, seed=31)
    queries = np.random.default_rng(32).standard_normal((q, f)).astype(np.float32)
    want_ids, want_scores = ref.brute_force(vectors, queries, 10)
    return vectors, queries, ix, want_ids, want_scores


def test_full_probe_is_exact(gpu, full_probe):
    vectors, queries, ix, want_ids, want_scores = full_probe
    got_ids, got_scores = ix.search(queries, 10, 32)
    _check_search(vectors, queries, got_ids, got_scores, want_ids, want_scores, cap=0.01)
    knn_ids, knn_scores = gpu.KnnQuery().topk(gpu.Matrix(vectors), gpu.Matrix(queries), 10)
    v64, q64 = vectors.astype(np.float64), queries.astype(np.float64)
    knn_exact = np.einsum("qkf,qf->qk", v64[knn_ids], q64)
    exceptions = ref.audit(got_ids, knn_ids, knn_exact, lambda r, i: v64[i] @ q64[r], vectors.shape[1])
    assert exceptions <= 0.01 * got_ids.size
    _check_scores(got_scores, knn_scores)


def test_recall_is_monotone_in_nprobe(gpu, full_probe):
    vectors, queries, ix, want_ids, _ = full_probe
    centroids = ix.centroids
    full_ids, _, full_probes = ix.search(queries, 10, 32, return_probes=True)
    coarse = queries.astype(np.float64) @ centroids.astype(np.float64).T
    want_probes = np.stack([ref.order_desc(row) for row in coarse])
    ref.audit(full_probes, want_probes, np.take_along_axis(coarse, want_probes, axis=1), lambda r, l: coarse[r, l], vectors.shape[1])
    # queries whose probe order, or whose full-probe result, rests on an (audited) near-tie are left out
    excluded = (full_probes != want_probes).any(axis=1) | (full_ids != want_ids).any(axis=1)
    assert excluded.sum() <= 0.01 * len(queries)
    previous = np.zeros(len(queries), dtype=int)
    for nprobe in (1, 2, 4, 8, 32):
        ids, _, probes = ix.search(queries, 10, nprobe, return_probes=True)
        np.testing.assert_array_equal(probes, full_probes[:, :nprobe])  # nested probe sets
        hits = np.array([len(np.intersect1d(ids[r], want_ids[r])) for r in range(len(queries))])
        assert (hits[~excluded] >= previous[~excluded]).all()
        previous = hits
    assert (previous[~excluded] == 10).all()


# ---- 7. determinism --------------------------------------------------------------------------------------------------------
def test_build_and_search_are_deterministic(gpu):
    rng = np.random.default_rng(41)
    vectors = rng.standard_normal((5000, 30)).astype(np.float32)
    init = rng.choice(5000, size=37, replace=False)
    queries = rng.standard_normal((90, 30)).astype(np.float32)
    a = gpu.IVFIndex.build(vectors, 37, 6, init_rows=init)
    b = gpu.IVFIndex.build(vectors, 37, 6, init_rows=init)
    for x, y in zip(_lists(a), _lists(b)):
        assert x.tobytes() == y.tobytes()
    first = a.search(queries, 25, 6, return_probes=True)
    for other in (a.search(queries, 25, 6, return_probes=True), b.search(queries, 25, 6, return_probes=True)):
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()
    # seeded initial rows: the same index again
    c = gpu.IVFIndex.build(vectors, 37, 6, random_state=9)
    d = gpu.IVFIndex.build(vectors, 37, 6, random_state=9)
    assert c.centroids.tobytes() == d.centroids.tobytes() and c.list_ids.tobytes() == d.list_ids.tobytes()
