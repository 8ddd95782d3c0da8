"""The IVF-Flat index (csrc/ivf.hip, implicit_amd.gpu.IVFIndex) at every launch cut, on the cases of tests/ivf_cases.py.

Every case but two is exact: integer-valued vectors and queries with scores below 2^24, `iterations = 0` builds from
initial rows that are zero or +-2^m e_j.  Centroids, list offsets, list ids, probes, result ids and result scores then have
one possible value each (ivf_reference.exact_build / exact_search, proved against the float64 restatement by
tests/test_ivf_cases_host.py) and are compared with assert_array_equal: no audit, no tolerance, no allowance for ties.

The two tolerances of this file: the centroids after two k-means rounds on integer clusters are held to 16 * 2^-24 relative
per element (ivf_cases.PLANTED_TOLERANCE, derived in the host test), and the probes over 2100 general centroids
(test_coarse_wide) are audited by the near-tie rule of ivf_reference.audit, at most 1 % of the positions."""
import ctypes

import numpy as np
import pytest

import ivf_cases as ic
import ivf_reference as ref

pytestmark = pytest.mark.gpu

_WANT = {}


def _num_cus():
    """multiProcessorCount of the current device, asked of the HIP runtime the library has loaded into this process."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    dev, cus = ctypes.c_int(-1), ctypes.c_int(0)
    multiprocessor_count = 63  # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert hip.hipGetDevice(ctypes.byref(dev)) == 0
    assert hip.hipDeviceGetAttribute(ctypes.byref(cus), multiprocessor_count, dev) == 0
    return cus.value


def _build(gpu, c):
    return gpu.IVFIndex.build(ic.cast(c.vectors, c.vdtype), c.nlist, 0, init_rows=c.init_rows)


def _want_build(c):
    """The integer restatement of a case's build, computed once and shared."""
    if c.name not in _WANT:
        _WANT[c.name] = ref.exact_build(c.vectors, c.init_rows)
    return _WANT[c.name]


def _check_build(ix, c):
    coord, sign, _, offsets, ids = _want_build(c)
    n, f = c.vectors.shape
    assert ix.shape == (n, f) and ix.nlist == c.nlist
    np.testing.assert_array_equal(ix.centroids, ref.exact_centroid_matrix(coord, sign, f), err_msg=f"{c.name}: centroids")
    np.testing.assert_array_equal(ix.list_offsets, offsets, err_msg=f"{c.name}: list offsets")
    np.testing.assert_array_equal(ix.list_ids, ids, err_msg=f"{c.name}: list ids")


def _queries(s):
    q = ic.cast(s.queries, s.qdtype)
    return q if s.repeat is None else q[np.arange(s.repeat) % len(q)]


def _want_search(c, s):
    coord, sign, assign, _, _ = _want_build(c)
    probes, ids, scores = ref.exact_search(coord, sign, assign, c.vectors, s.queries, s.k, s.nprobe)
    if s.repeat is not None:
        rows = np.arange(s.repeat) % len(s.queries)
        probes, ids, scores = probes[rows], ids[rows], scores[rows]
    return probes, ids, scores.astype(np.float32)


def _check_search(ix, c, s, what):
    got_ids, got_scores, got_probes = ix.search(_queries(s), s.k, s.nprobe, return_probes=True)
    probes, ids, scores = _want_search(c, s)
    assert got_ids.dtype == np.int32 and got_scores.dtype == np.float32 and got_probes.dtype == np.int32
    np.testing.assert_array_equal(got_probes, probes, err_msg=f"{what}: probes")
    np.testing.assert_array_equal(got_ids, ids, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(got_scores, scores, err_msg=f"{what}: scores")
    return got_ids, got_scores, got_probes


def _run(gpu, c):
    ix = _build(gpu, c)
    _check_build(ix, c)
    for i, s in enumerate(c.searches):
        _check_search(ix, c, s, f"{c.name} search {i} (k = {s.k}, nprobe = {s.nprobe})")
    return ix


@pytest.mark.parametrize("name", ic.names("factors"))
def test_factors(gpu, name):
    _run(gpu, ic.get(name))


@pytest.mark.parametrize("f", ic.PLANTED_FACTORS)
def test_planted_kmeans_rounds(gpu, f):
    """Two rounds on integer clusters: the list sums are exact, so a centroid element is off the float64 one by the
    roundings of the mean, the sum of squares, the square root and the division alone: 16 * 2^-24 relative, zero where the sum is."""
    vectors, init_rows, iterations = ic.planted(f)
    want_cent, want_assign = ref.kmeans(vectors, init_rows, iterations)
    ix = gpu.IVFIndex.build(vectors.astype(np.float32), len(init_rows), iterations, init_rows=init_rows)
    offsets, ids = ref.build_lists(want_assign, len(init_rows))
    np.testing.assert_array_equal(ix.list_offsets, offsets)
    np.testing.assert_array_equal(ix.list_ids, ids)
    got = ix.centroids.astype(np.float64)
    worst = np.max(np.abs(got - want_cent)[want_cent != 0] / np.abs(want_cent[want_cent != 0]))
    print(f"f = {f}: largest relative centroid error {worst / 2.0 ** -24:.2f} * 2^-24")
    assert (got[want_cent == 0] == 0).all()
    assert (np.abs(got - want_cent) <= ic.PLANTED_TOLERANCE * np.abs(want_cent)).all()


@pytest.mark.parametrize("name", ic.names("tiles"))
def test_tiles(gpu, name):
    _run(gpu, ic.get(name))


@pytest.mark.parametrize("name", ic.names("many_lists"))
def test_many_lists(gpu, name):
    c = ic.get(name)
    ix = _run(gpu, c)
    if c.nlist <= ic.K_IVF_MAX_K:
        return
    # more than 1024 lists: a larger nprobe is refused, not clamped, for any number of queries, and changes nothing
    s = c.searches[0]
    before = ix.search(_queries(s), s.k, 7, return_probes=True)
    for nprobe in (ic.K_IVF_MAX_K + 1, c.nlist, 1 << 40):
        for q in (_queries(s), _queries(s)[:0]):
            with pytest.raises(ValueError):
                ix.search(q, s.k, nprobe)
    _check_build(ix, c)
    for x, y in zip(before, ix.search(_queries(s), s.k, 7, return_probes=True)):
        assert x.tobytes() == y.tobytes()
    _check_search(ix, c, c.searches[2], f"{name} after the refusals")


def test_coarse_wide(gpu):
    """2100 general centroids, every coarse score in one bucket of the 11-bit histogram: the coarse select works on the
    scores themselves.  Probes: the near-tie audit against float64.  The scan, given those probes and the index's own lists: exact."""
    vectors, init_rows, queries = ic.coarse_wide()
    ix = gpu.IVFIndex.build(vectors.astype(np.float32), len(init_rows), 0, init_rows=init_rows)
    centroids, offsets, ids = ix.centroids, ix.list_offsets, ix.list_ids
    assert offsets[0] == 0 and offsets[-1] == len(vectors) and (np.diff(offsets) >= 0).all()
    np.testing.assert_array_equal(np.sort(ids), np.arange(len(vectors)))
    assign = np.empty(len(vectors), dtype=np.int64)
    assign[ids] = np.repeat(np.arange(len(init_rows)), np.diff(offsets))
    np.testing.assert_array_equal(ids, ref.build_lists(assign, len(init_rows))[1])  # ascending inside every list
    coarse = queries.astype(np.float64) @ centroids.astype(np.float64).T
    for P in (1, 10):
        got_ids, got_scores, probes = ix.search(queries.astype(np.float32), 10, P, return_probes=True)
        want = np.stack([ref.order_desc(row)[:P] for row in coarse])
        exceptions = ref.audit(probes, want, np.take_along_axis(coarse, want, axis=1), lambda r, l: coarse[r, l], vectors.shape[1])
        print(f"P = {P}: {exceptions} near-tie probes of {probes.size}")
        assert exceptions <= 0.01 * probes.size
        assert all(len(set(row)) == P for row in probes.tolist())
        _, want_ids, want_scores = ref.exact_search(np.zeros(len(init_rows), dtype=np.int64), None, assign, vectors, queries, 10, P,
                                                    probes=probes)
        np.testing.assert_array_equal(got_ids, want_ids)
        np.testing.assert_array_equal(got_scores, want_scores.astype(np.float32))


@pytest.mark.parametrize("name", ic.names("survivors"))
def test_survivors(gpu, name):
    _run(gpu, ic.get(name))


@pytest.mark.parametrize("name", ic.names("ties"))
def test_ties(gpu, name):
    _run(gpu, ic.get(name))


@pytest.mark.parametrize("name", ic.names("k_cuts"))
def test_k_cuts(gpu, name):
    c = ic.get(name)
    ix = _build(gpu, c)
    _check_build(ix, c)
    for s in c.searches:
        got_ids, got_scores, _ = _check_search(ix, c, s, f"{name} k = {s.k}")
        assert (got_ids[-1] == -1).all() and (got_scores[-1] == -np.finfo(np.float32).max).all()  # the empty list alone


@pytest.mark.parametrize("name", ic.names("grouping"))
def test_grouping(gpu, name):
    _run(gpu, ic.get(name))


def test_counter_cap(gpu):
    _run(gpu, ic.get("counter_cap"))


def test_build_in_row_chunks(gpu):
    """n = nlist = 33000: the assignment scores exceed the budget, so the build scores and assigns its rows in two chunks."""
    vectors, init_rows, assign, queries = ic.build_chunks()
    n, f = vectors.shape
    ix = gpu.IVFIndex.build(vectors.astype(np.float32), n, 0, init_rows=init_rows)
    coord, sign = ref.exact_centroids(vectors, init_rows)
    offsets, ids = ref.build_lists(assign, n)
    np.testing.assert_array_equal(ix.centroids, ref.exact_centroid_matrix(coord, sign, f))
    np.testing.assert_array_equal(ix.list_offsets, offsets)
    np.testing.assert_array_equal(ix.list_ids, ids)
    for k, nprobe in ((10, 5), (1024, 1024)):
        probes, want_ids, want_scores = ref.exact_search(coord, sign, assign, vectors, queries, k, nprobe)
        got_ids, got_scores, got_probes = ix.search(queries.astype(np.float32), k, nprobe, return_probes=True)
        np.testing.assert_array_equal(got_probes, probes)
        np.testing.assert_array_equal(got_ids, want_ids)
        np.testing.assert_array_equal(got_scores, want_scores.astype(np.float32))


def test_second_trip(gpu):
    cus = _num_cus()
    assert 32 <= cus <= 1024  # a compute-unit count, not another attribute
    c = ic.second_trip(cus)
    c.name = f"second_trip_{cus}"
    n, f = c.vectors.shape
    assert ic.tiles(1, c.claims["long"]) > ic.scan_grid(cus)  # one query's tiles of the long list alone
    assert n * ic.f_pad(f) > ic.ivf_grid(n * ic.f_pad(f), 256, cus) * 256  # ivf_pad (pad_rows_kernel)
    assert n * (ic.f_pad(f) // 4) > ic.ivf_grid(n * (ic.f_pad(f) // 4), 256, cus) * 256  # ivf_gather_rows_kernel
    _run(gpu, c)


def test_chunks_of_one_query(gpu):
    c = ic.get("tiles")
    ix = _build(gpu, c)
    s = c.searches[1]
    whole = _check_search(ix, c, s, "unchunked")
    ix.set_temp_memory(1)
    try:
        chunked = ix.search(_queries(s), s.k, s.nprobe, return_probes=True)
    finally:
        ix.set_temp_memory(0)
    for x, y in zip(whole, chunked):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(whole, ix.search(_queries(s), s.k, s.nprobe, return_probes=True)):
        assert x.tobytes() == y.tobytes()


def test_workspace_reuse(gpu):
    """One handle searched small, large and small again, k and nprobe changing: the temporaries it keeps never show."""
    c = ic.get("tiles")
    ix = _build(gpu, c)
    q = _queries(c.searches[0])
    for rows, k, nprobe in ((3, 5, 1), (len(q), 300, 7), (2, 7, 2), (len(q), 1, 34), (1, 1024, 3)):
        kept = ix.search(q[:rows], k, nprobe, return_probes=True)
        fresh = _build(gpu, c).search(q[:rows], k, nprobe, return_probes=True)
        for x, y in zip(kept, fresh):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        probes, ids, scores = _want_search(c, ic.search_spec(c.searches[0].queries[:rows], k, nprobe))
        for x, y in zip(kept, (ids, scores, probes)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ic.names("inputs"))
def test_inputs_are_widened(gpu, name):
    _run(gpu, ic.get(name))


def test_zero_queries(gpu):
    c = ic.get("factors_f5_fp32")
    ix = _build(gpu, c)
    for dtype in (np.float32, np.float16):
        ids, scores, probes = ix.search(np.zeros((0, 5), dtype=dtype), 7, 3, return_probes=True)
        assert ids.shape == (0, 7) and scores.shape == (0, 7) and probes.shape == (0, 3)
        assert ids.dtype == np.int32 and scores.dtype == np.float32
    _check_search(ix, c, c.searches[0], "after zero queries")


@pytest.mark.parametrize("iterations", [0, 1])
def test_overflowing_sum_of_squares(gpu, iterations):
    """Entries of 2^100: an initial row whose sum of squares overflows gives a zero centroid, a list whose mean's does keeps
    its centroid; no NaN anywhere, and the scores of these finite inputs are exact."""
    vectors, init_rows, cent0, cent1, assign, queries, scores = ic.overflow()
    ix = gpu.IVFIndex.build(vectors, 2, iterations, init_rows=init_rows)
    np.testing.assert_array_equal(ix.centroids, cent1 if iterations else cent0)
    offsets, ids = ref.build_lists(assign, 2)
    np.testing.assert_array_equal(ix.list_offsets, offsets)
    np.testing.assert_array_equal(ix.list_ids, ids)
    for k in (4, 10, 12):
        got_ids, got_scores = ix.search(queries, k, 2)
        assert not np.isnan(got_scores).any()
        for r in range(len(queries)):
            want_ids, want_scores = ref.topk_candidates(scores[r], np.arange(len(vectors)), k)
            np.testing.assert_array_equal(got_ids[r], want_ids)
            np.testing.assert_array_equal(got_scores[r], want_scores.astype(np.float32))
