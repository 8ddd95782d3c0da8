"""Host-only proof of what tests/test_gpu_ivf_edges.py relies on: the constants and formulas restated in tests/ivf_cases.py are
those of csrc/ivf.hip (matched against its text), every case sits on the cut it claims under that arithmetic, every exact
case keeps its scores below 2^24, and the integer restatement (ivf_reference.exact_build / exact_search) equals the float64
one (ivf_reference.kmeans / search) on every exact case."""
import os
import re

import numpy as np
import pytest

import ivf_cases as ic
import ivf_reference as ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "implicit_amd", "csrc")
FLOAT64_ROWS = 256  # queries per search that also go through the per-query float64 restatement


@pytest.fixture(scope="module")
def built():
    cache = {}

    def of(c):
        if c.name not in cache:
            cache[c.name] = ref.exact_build(c.vectors, c.init_rows)
        return cache[c.name]

    return of


def _exact_cases():
    return [ic.get(n) for n in ic.NAMES] + [_second_trip(256), _second_trip(304)]


def _second_trip(cus):
    c = ic.second_trip(cus)
    c.name = f"second_trip_{cus}"
    return c


# ---- the restated constants and formulas against the source text ----------------------------------------------------------
def test_constants_match_the_source():
    with open(os.path.join(CSRC, "ivf.hip")) as f:
        src = f.read()
    want = {"kIvfBM": ic.K_IVF_BM, "kIvfBN": ic.K_IVF_BN, "kIvfBK": ic.K_IVF_BK, "kIvfRun": ic.K_IVF_RUN,
            "kIvfSurvivors": ic.K_IVF_SURVIVORS, "kIvfMaxK": ic.K_IVF_MAX_K}
    for name, value in want.items():
        m = re.search(rf"^constexpr int {name} = (\d+);", src, re.M)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"^constexpr int64_t kIvfMaxCounters = \(int64_t\)1 << 24;", src, re.M) and ic.K_IVF_MAX_COUNTERS == 1 << 24
    for text in (
            "ix->f_pad = (int)((f + 3) / 4 * 4)",                                                 # f_pad
            "for (int k0 = 0; k0 < a.f_pad; k0 += kIvfBK)",                                        # k_steps
            "for (int d = threadIdx.x; d < f_pad; d += 256)",                                      # elements_per_thread
            "t += ((np + kIvfBM - 1) / kIvfBM) * ((len + kIvfBN - 1) / kIvfBN)",                   # tiles
            "if (len > 0 && np > 0)",
            "const int per = (nlist + 1023) / 1024",                                               # plan_per (ivf_plan_kernel)
            "const int per = (n + 1023) / 1024",                                                   # plan_per (ivf_exclusive_scan_kernel)
            "std::max<int64_t>(1, std::min<int64_t>((n_max + kIvfRun - 1) / kIvfRun, kIvfMaxCounters / nkeys))",  # grouper
            "const int64_t per = (n + nruns - 1) / nruns;",
            "std::max<int64_t>(64, (per + 63) / 64 * 64)",
            "std::max<int64_t>(1, (n + run - 1) / run)",
            "dim3(ctx().num_cus * 8)",                                                             # scan_grid
            "std::min<size_t>((work + block - 1) / block, (size_t)ctx().num_cus * 16)",            # ivf_grid
            "std::min<size_t>(free_b / 2, (size_t)4 << 30)",                                       # DEFAULT_BUDGET
            "std::min<size_t>(n, std::max<size_t>(kIvfBM, ix->budget / (sizeof(float) * nlist)))",  # build_chunk
            "std::max<int64_t>(ix->lens_desc_sum[P], nlist)",                                      # search_chunk
            "sizeof(float) * (max_cand + f_pad + P + k) + sizeof(int32_t) * (3 * (size_t)P + k)",
            "std::min<size_t>(nq, std::max<size_t>(1, ix->budget / per_query))",
            "atomicAdd(&hist[key >> 53], 1u)",                                                     # bucket
            "if (n_lds <= (unsigned)kIvfSurvivors)",                                               # select_path
            "if (P > kIvfMaxK) throw",
            "while (kpad < k) kpad <<= 1;", "while (ppad < P) ppad <<= 1;"):                       # pow2_pad
        assert text in src, text
    with open(os.path.join(CSRC, "select_ops.h")) as f:
        ops = f.read()
    assert "if (u == 0x80000000u) u = 0u;" in ops and "return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);" in ops
    assert "return ((uint64_t)ordered(s) << 32) | (uint32_t)id;" in ops


def test_ordered_and_bucket():
    x = np.array([-np.inf, -3e38, -1025.0, -1.0, -1e-40, -0.0, 0.0, 1e-40, 1.0, 1024.0, 1279.0, 1280.0, 1535.0, 1536.0, np.inf],
                 dtype=np.float32)
    o = ic.ordered(x).astype(np.int64)
    assert o[5] == o[6] == 0x80000000 and (np.diff(np.delete(o, 5)) > 0).all()
    assert ic.ordered(np.float32(1.0)) == 0xBF800000
    b = ic.bucket(x)
    assert b[9] == b[10] and b[11] == b[12] == b[10] + 1 and b[13] == b[12] + 1  # [1024, 1280), [1280, 1536), [1536, ..)
    assert ic.pow2_pad(1) == 1 and ic.pow2_pad(3) == 4 and ic.pow2_pad(256) == 256 and ic.pow2_pad(257) == 512 and ic.pow2_pad(1024) == 1024


def test_select_path_restatement():
    rng = np.random.default_rng(1)
    for n, k in ((50, 7), (3000, 100), (3000, 1024)):
        scores = rng.integers(-50, 50, size=n).astype(np.float32)
        ids = rng.permutation(10 * n)[:n]
        p = ic.select_path(scores, ids, k)
        assert p.total == n and p.path in ("lds", "global") and 0 <= p.digit <= 7
        # the keys at or above the boundary found by the radix walk are exactly the k best
        order = np.lexsort((-ids, -scores.astype(np.float64)))[:k]
        kth = (int(ic.ordered(scores[order[-1:]])[0]) << 32) | int(ids[order[-1]])
        keys = (ic.ordered(scores).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
        assert (keys >= np.uint64(kth)).sum() == k
    assert ic.select_path(np.ones(5, dtype=np.float32), np.arange(5), 5).path == "all"


# ---- every exact case -------------------------------------------------------------------------------------------------------
def test_every_exact_case_is_wellformed(built):
    families = set()
    for c in _exact_cases():
        n, f = c.vectors.shape
        families.add(c.family)
        assert c.vectors.dtype == np.int64 and 1 <= c.nlist <= n and 1 <= f <= 1024, c.name
        assert len(set(c.init_rows.tolist())) == c.nlist, c.name  # distinct initial rows
        vmax = int(np.abs(c.vectors).max())
        dtypes = {c.vdtype} | {s.qdtype for s in c.searches}
        if "float16" in dtypes:
            assert vmax <= 2048 and all(np.abs(s.queries).max() <= 2048 for s in c.searches), c.name
        for s in c.searches:
            assert s.queries.shape[1] == f and 1 <= s.k <= ic.K_IVF_MAX_K and s.nprobe >= 1, c.name
            assert f * vmax * int(np.abs(s.queries).max()) < 1 << 24, c.name  # every partial sum below 2^24
        coord, sign, assign, offsets, ids = built(c)
        if "sizes" in c.claims:
            np.testing.assert_array_equal(np.diff(offsets), c.claims["sizes"], err_msg=c.name)
    assert families == {"factors", "tiles", "many_lists", "counter_cap", "survivors", "ties", "k_cuts", "grouping", "inputs",
                        "second_trip"}


def test_integer_restatement_equals_the_float64_one(built):
    for c in _exact_cases():
        coord, sign, assign, offsets, ids = built(c)
        f = c.vectors.shape[1]
        cent, want_assign = ref.kmeans(c.vectors, c.init_rows, 0)
        np.testing.assert_array_equal(cent, ref.exact_centroid_matrix(coord, sign, f), err_msg=c.name)
        np.testing.assert_array_equal(assign, want_assign, err_msg=c.name)
        want_off, want_ids = ref.build_lists(want_assign, c.nlist)
        np.testing.assert_array_equal(offsets, want_off, err_msg=c.name)
        np.testing.assert_array_equal(ids, want_ids, err_msg=c.name)
        for s in c.searches:
            rows = slice(0, FLOAT64_ROWS)
            got = ref.exact_search(coord, sign, assign, c.vectors, s.queries, s.k, s.nprobe)
            want = ref.search(cent, offsets, ids, c.vectors, s.queries[rows], s.k, s.nprobe)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g[rows], w, err_msg=f"{c.name} k = {s.k} nprobe = {s.nprobe}")


def _pairs(probes, nlist):
    return np.bincount(np.asarray(probes).ravel(), minlength=nlist)


def _scan_shapes(c, s, built):
    """Per list (queries probing it, length) of one search."""
    coord, sign, _, offsets, _ = built(c)
    return list(zip(_pairs(ref.exact_probes(coord, sign, s.queries, s.nprobe), c.nlist).tolist(), np.diff(offsets).tolist()))


def _candidates(c, s, r, built):
    """(scores float32, ids) of the candidates of query r of a search."""
    coord, sign, assign, _, _ = built(c)
    probes = ref.exact_probes(coord, sign, s.queries[r:r + 1], s.nprobe)[0]
    members = np.flatnonzero(np.isin(assign, probes))
    return ref.exact_scores(c.vectors[members], s.queries[r:r + 1])[0].astype(np.float32), members


# ---- the claims, family by family -------------------------------------------------------------------------------------------
def test_factor_claims(built):
    assert ic.FACTORS == (1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 1021, 1024)
    assert sorted({ic.f_pad(f) for f in ic.FACTORS}) == [4, 8, 32, 36, 256, 260, 1024]
    assert sorted({ic.k_steps(f) for f in ic.FACTORS}) == [1, 2, 8, 9, 32]
    assert sorted({ic.elements_per_thread(f) for f in ic.FACTORS}) == [1, 2, 4]
    for f in ic.FACTORS:
        for storage in ("fp32", "fp16"):
            c = ic.get(f"factors_f{f}_{storage}")
            sizes = c.claims["sizes"]
            assert c.vectors.shape[1] == f and len(c.vectors) <= 800 and c.vdtype == {"fp32": "float32", "fp16": "float16"}[storage]
            assert (sizes == 0).sum() >= 2 and (built(c)[1] == 0).sum() == 1  # empty duplicates and a zero centroid
            assert {c.vdtype} | {s.qdtype for s in c.searches} == {"float32", "float16"}
            # coarse ties abound: the probe order rests on the list id
            coord, sign = built(c)[:2]
            coarse = c.searches[0].queries[:, coord] * sign
            assert np.mean([len(set(row)) for row in coarse.tolist()]) < 0.8 * c.nlist or f == 1


def test_planted_claims():
    """The derived bound.  List sums are integers below 2^24: exact.  mean = sum / count: one rounding (2^-24 relative).  The
    sum of squares: a chain of at most 4 fmaf and a tree of 8 additions over positive terms, each rounding 2^-24 relative of a
    partial sum that is at most the total, on top of the 2 * 2^-24 the squared means carry: below 14 * 2^-24 relative.  The
    square root halves that and adds its own rounding (below 8 * 2^-24), the division adds one and the mean's own: below
    8 * 2^-24 + 2 * 2^-24 plus second-order terms.  PLANTED_TOLERANCE = 16 * 2^-24 is what the GPU test holds."""
    assert ic.PLANTED_TOLERANCE == 16 * 2.0 ** -24 and ic.PLANTED_FACTORS == (257, 1024)
    for f in ic.PLANTED_FACTORS:
        vectors, init_rows, iterations = ic.planted(f)
        assert iterations == 2 and ic.elements_per_thread(f) in (2, 4) and np.abs(vectors).max() <= 67
        history = []
        cent, assign = ref.kmeans(vectors, init_rows, iterations, history=history)
        assert len(history) == iterations + 1
        # a score is off by at most (f_pad + 1) 2^-24 |v|.|c| from summation and 16 * 2^-24 |v|.|c| from the centroid;
        # |v|.|c| <= ||v|| (unit centroid).  Twice that on both scores of a margin, and a factor two to spare.
        norm = np.sqrt((vectors.astype(np.float64) ** 2).sum(axis=1))
        moved = 4 * (ic.f_pad(f) + 17) * 2.0 ** -24 * norm
        for round_assign, margin in history:
            assert (margin > moved).all() and margin.min() > 10
            np.testing.assert_array_equal(round_assign, np.arange(len(vectors)) % 16)
        sums = np.zeros((16, f))
        np.add.at(sums, assign, vectors)
        assert np.abs(sums).max() < 1 << 24
        assert (sums == 0).any() and ((sums == 0) == (cent == 0)).all()  # the exactly-zero elements exist
        assert cent[15, f - 1] > 0.9  # the last element of the last trip carries a cluster


def test_tile_claims(built):
    c = ic.get("tiles")
    assert ic.TILE_LENS == (0, 1, 127, 128, 129, 257) and ic.TILE_QUERIES == (1, 63, 64, 65, 129)
    assert {ic.K_IVF_BN - 1, ic.K_IVF_BN, ic.K_IVF_BN + 1, 2 * ic.K_IVF_BN + 1} <= set(ic.TILE_LENS)
    assert {ic.K_IVF_BM - 1, ic.K_IVF_BM, ic.K_IVF_BM + 1, 2 * ic.K_IVF_BM + 1} <= set(ic.TILE_QUERIES)
    one, two = _scan_shapes(c, c.searches[0], built), _scan_shapes(c, c.searches[1], built)
    assert c.searches[0].nprobe == 1 and c.searches[1].nprobe == 2
    assert {(q, n) for q in ic.TILE_QUERIES for n in ic.TILE_LENS[1:]} <= set(one)  # exact counts on both sides, crossed
    assert {(q, 0) for q in ic.TILE_QUERIES} <= set(two)                              # probed and empty
    assert {(0, 5), (0, 200), (0, 2)} <= set(one)                                     # non-empty and unprobed
    assert sum(ic.tiles(q, n) for q, n in one) == sum(-(-q // 64) * -(-n // 128) for q, n in one if q and n) > 25
    # lists without tiles before, between and after the lists that have them (nprobe = 1; with two probes the second one
    # of many queries is the last list, by the tie rule)
    has = np.array([ic.tiles(q, n) > 0 for q, n in one])
    first, last = np.flatnonzero(has)[[0, -1]]
    assert first > 0 and last < c.nlist - 1 and (~has[first:last]).any()
    assert not all(ic.tiles(q, n) > 0 for q, n in two)
    assert ic.f_pad(20) == 20 and ic.k_steps(20) == 1 and c.searches[2].qdtype == "float16"
    assert any(s.k > 257 for s in c.searches)  # holes behind every list


def test_many_lists_claims(built):
    assert [ic.plan_per(n) for n in ic.MANY_LISTS] == [1, 2, 2] and ic.MANY_LISTS == (1024, 1025, 2048)
    for nlist in ic.MANY_LISTS:
        c = ic.get(f"many_lists_{nlist}")
        n, f = c.vectors.shape
        assert c.nlist == nlist and f == 1024 and nlist < n <= nlist + 100 and (c.claims["sizes"] == 0).sum() == 40
        assert sorted({s.nprobe for s in c.searches}) == [1, 1023, 1024]
        assert max(s.k for s in c.searches) == 1024 and ic.pow2_pad(1023) == 1024
        shapes = _scan_shapes(c, c.searches[0], built)
        has = np.array([ic.tiles(q, m) > 0 for q, m in shapes])
        assert 0 < has.sum() <= len(c.searches[0].queries) and (~has).sum() > 1000  # a search among tile-less lists
        # the coarse select of nlist <= 2048 candidates always fits the LDS copy; coarse ties abound
        coord, sign = built(c)[:2]
        coarse = (c.searches[0].queries[:, coord] * sign).astype(np.float32)
        for P in (1, 1023):
            assert ic.select_path(coarse[0], np.arange(nlist), P).path == "lds"
        assert len(set(coarse[0].tolist())) <= 9


def test_counter_cap_claims(built):
    c = ic.get("counter_cap")
    s = c.searches[0]
    R, P = s.repeat, s.nprobe
    assert c.nlist == 2048 and P == ic.K_IVF_MAX_K == 1024 and R == 8193 and len(s.queries) == ic.COUNTER_CAP_DISTINCT
    longest = int(np.sort(c.claims["sizes"])[::-1][:P].sum())
    assert ic.search_chunk(R, longest, c.nlist, 1024, P, s.k) == R  # one chunk at the default budget
    g = ic.grouper(R * P, c.nlist)
    assert g.nruns == ic.K_IVF_MAX_COUNTERS // c.nlist == 8192 < -(-R * P // ic.K_IVF_RUN) and g.run == 1088 and g.used == 7712
    below = ic.grouper((R - 1) * P, c.nlist)
    assert below.nruns == 8192 == -(-(R - 1) * P // ic.K_IVF_RUN) and below.run == 1024  # one query fewer: not capped
    # the other shape that reaches the cap, a build with n = nlist = 2^17 + 1 (127 runs where 129 are asked for), writes
    # n * nlist * 4 bytes = 64 GiB of assignment scores in 17 chunks: seconds of memory traffic against this search's 70 MB
    n = (1 << 17) + 1
    assert ic.grouper(n, n).nruns == 127 < -(-n // ic.K_IVF_RUN) and ic.grouper(n - 1, n - 1).nruns == 128 == (n - 1) // 1024
    assert ic.build_chunk(n, n) < n and -(-n // ic.build_chunk(n, n)) == 17 and n * n * 4 > 64 << 30
    assert R * (longest + 1024) * 4 < 80 << 20


def test_survivor_claims(built):
    for which in ic.SURVIVOR_CASES:
        for lists in ("one_list", "four_lists"):
            c = ic.get(f"survivors_{which}_{lists}")
            s = c.searches[0]
            assert c.vectors.shape[1] == 2 and s.queries.tolist() == [[1, 0]]
            sizes = np.diff(built(c)[3])
            assert (len(sizes) == 4 and (sizes > 100).sum() >= 3 and (sizes > 0).all()) if lists == "four_lists" else len(sizes) == 1
            scores, ids = _candidates(c, s, 0, built)
            assert len(ids) == len(c.vectors)  # every list probed
            p = ic.select_path(scores, ids, s.k)
            assert p.n_lds == c.claims["n_lds"] == (2048 if which.endswith("2048") else 2049)
            assert p.path == ("lds" if which.endswith("2048") else "global")
            assert (p.above > 0) == c.claims["second"] and (p.above == 500 or p.above == 0)
            top = np.sort(scores)[::-1][:s.k]
            assert len(set(top.tolist())) < s.k / 2  # ties among the winners


def test_tie_claims(built):
    want = {(200, 10): ("lds", 0), (200, 199): ("lds", 0), (2000, 100): ("lds", 0), (2000, 208): ("lds", 1), (2000, 1024): ("lds", 0),
            (3000, 100): ("global", 0), (3000, 184): ("global", 1), (3000, 1024): ("global", 0)}
    seen = {}
    for n, ks in ic.TIE_CASES:
        c = ic.get(f"ties_n{n}")
        assert np.diff(built(c)[3]).tolist() == [0, n]  # an empty duplicate and the list of everything
        for s in c.searches:
            scores, ids = _candidates(c, s, 0, built)
            assert len(ids) == n and len(set(scores.tolist())) == 1
            p = ic.select_path(scores, ids, s.k)
            seen[(n, s.k)] = (p.path, p.digit)
        assert (n > 256) == (len(set((np.arange(n) >> 8).tolist())) > 1) and n < 65536  # byte 1 of the id; never byte 2
    assert seen == want
    for cus in (256, 304):  # byte 2: the zero query of second_trip, whose candidates all score 0
        c = _second_trip(cus)
        scores, ids = _candidates(c, c.searches[0], 1, built)
        assert len(ids) == len(c.vectors) > 1 << 18 and len(set(scores.tolist())) == 1
        assert len(set((ids >> 16).tolist())) >= 4 and ic.select_path(scores, ids, c.searches[0].k).path == "global"


def test_k_cut_claims(built):
    c = ic.get("k_cuts")
    assert ic.K_CUTS == (1, 2, 3, 255, 256, 257, 1023, 1024)
    coord, sign, _, offsets, _ = built(c)
    sizes = np.diff(offsets)
    assert sorted(sizes.tolist()) == [0] + ic.k_cut_sizes() and sizes[sign == 0].tolist() == [0]
    assert [s.k for s in c.searches] == list(ic.K_CUTS)
    for s in c.searches:
        assert s.nprobe == 1
        totals = sizes[ref.exact_probes(coord, sign, s.queries, 1)[:, 0]].tolist()
        assert totals[-1] == 0 and set(totals) == {s.k - 1, s.k, s.k + 1, 1025, 0}
    assert [ic.pow2_pad(k) for k in ic.K_CUTS] == [1, 2, 4, 256, 256, 512, 1024, 1024]


def test_grouping_claims(built):
    assert ic.GROUP_NS == (1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097) and ic.GROUP_KEYS == (3, 300)
    runs = {n: ic.grouper(n, 3) for n in ic.GROUP_NS}
    assert [runs[n].used for n in ic.GROUP_NS] == [1, 1, 1, 1, 1, 1, 2, 3, 5]
    assert [runs[n].run for n in ic.GROUP_NS] == [64, 64, 64, 128, 1024, 1024, 576, 704, 832]  # `per` rounded up to 64
    for keys in ic.GROUP_KEYS:
        for n in ic.GROUP_NS:
            if keys == 300 and n < 300:
                continue
            c = ic.get(f"grouping_n{n}_keys{keys}")
            assert len(c.vectors) == n and c.nlist == min(n, keys) and (c.claims["sizes"] >= 1).all()
            ids = built(c)[4]
            assert n < 3 or (np.diff(ids) < 0).any()  # the lists interleave in id order: stability is needed
        c = ic.get(f"grouping_n1025_keys{keys}")
        assert [len(s.queries) * s.nprobe for s in c.searches] == list(ic.GROUP_NS)
        for s in c.searches:
            g = ic.grouper(len(s.queries) * s.nprobe, c.nlist)
            assert (g.run, g.used) == (runs[len(s.queries) * s.nprobe].run, runs[len(s.queries) * s.nprobe].used)
            assert ic.search_chunk(len(s.queries), len(c.vectors), c.nlist, c.vectors.shape[1], s.nprobe, s.k) == len(s.queries)
    assert 300 > 256  # ivf_group_colscan_kernel: a second workgroup of 256 keys


def _group_model(keys, nkeys, inclusive_rank=False):
    """IvfGrouper::run step by step: the runs, cnt[run][key], the scan over the runs and over the keys, and the scatter's walk
    of every run in steps of 64 lanes.  inclusive_rank: the scatter's rank counts `j <= lane`; no lane then has rank 0, so no
    lane fetches or advances the counter and every base is 0.  `order` has one spare slot, which only that mutant writes."""
    keys = np.asarray(keys)
    n = len(keys)
    g = ic.grouper(n, nkeys)
    cnt = np.stack([np.bincount(keys[r * g.run:(r + 1) * g.run], minlength=nkeys) for r in range(g.used)])
    base = np.cumsum(cnt, axis=0) - cnt
    off = np.concatenate([[0], np.cumsum(cnt.sum(axis=0))])
    order = np.full(n + 1, -1, dtype=np.int64)
    for r in range(g.used):
        end = min(n, (r + 1) * g.run)
        for i0 in range(r * g.run, end, 64):
            step = keys[i0:min(end, i0 + 64)]
            for lane, key in enumerate(step.tolist()):
                rank = int((step[:lane] == key).sum()) + (1 if inclusive_rank else 0)
                order[off[key] + (0 if inclusive_rank else base[r, key]) + rank] = i0 + lane
            if not inclusive_rank:
                base[r] += np.bincount(step, minlength=nkeys)
    return off[:-1].tolist() + [off[-1]], order


def test_the_cases_discriminate(built):
    """Two one-line breaks of ivf.hip that cannot be tried on a device, because they write outside their buffers (the first
    one element past `order`, the second through list offsets that were never written), tried on the restatement instead."""
    # (1) the scatter's rank counting `j <= lane`: other list ids in every grouping case of two vectors or more
    for name in ic.names("grouping"):
        c = ic.get(name)
        _, _, assign, offsets, ids = built(c)
        off, order = _group_model(assign, c.nlist)
        assert off == offsets.tolist() and order[:-1].tolist() == ids.tolist() and order[-1] == -1, name
        _, broken = _group_model(assign, c.nlist, inclusive_rank=True)
        assert broken[:-1].tolist() != ids.tolist(), name
    # (2) `per` of ivf_plan_kernel fixed at 1: lists 1024 and beyond get no tile offset.  Every search on more than 1024
    # lists has tiles there (a single probe too: coarse ties go to the largest list id); at 1024 lists nothing changes.
    for nlist in ic.MANY_LISTS:
        c = ic.get(f"many_lists_{nlist}")
        for s in c.searches:
            shapes = _scan_shapes(c, s, built)
            beyond = sum(ic.tiles(q, n) for q, n in shapes[1024:])
            assert (beyond > 0) == (nlist > 1024), (nlist, s.nprobe)


def test_build_chunk_claims():
    n = ic.BUILD_CHUNKS_N
    assert ic.build_chunk(n, n) == (4 << 30) // (4 * n) < n < 2 * ic.build_chunk(n, n)   # two chunks at the default budget
    assert ic.build_chunk(32768, 32768) == 32768  # n = nlist = 2^15 is still one chunk
    assert ic.plan_per(n) == 33 and ic.grouper(n, n).nruns == 33 and n * n * 4 < 5 << 30
    vectors, init_rows, assign, queries = ic.build_chunks()
    assert vectors.shape == (n, 4) and sorted(init_rows.tolist()) == list(range(n)) and len(set(assign.tolist())) == 8
    # the shortcut (every vector to the last list of its direction) against the full restatement, at a size that allows it
    vectors, init_rows, assign, queries = ic.build_chunks(1500)
    coord, sign, want_assign, offsets, ids = ref.exact_build(vectors, init_rows)
    np.testing.assert_array_equal(assign, want_assign)
    cent, float_assign = ref.kmeans(vectors, init_rows, 0)
    np.testing.assert_array_equal(assign, float_assign)
    for k, nprobe in ((10, 5), (1024, 1024)):
        got = ref.exact_search(coord, sign, assign, vectors, queries, k, nprobe)
        want = ref.search(cent, offsets, ids, vectors, queries, k, nprobe)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_second_trip_claims(built):
    for cus in (256, 304):
        c = _second_trip(cus)
        n, f = c.vectors.shape
        long = c.claims["long"]
        assert ic.f_pad(f) == 16 and long in c.claims["sizes"] and long == 128 * 8 * cus + 300
        assert ic.tiles(1, long) > ic.scan_grid(cus) and ic.tiles(1, long - 300) == ic.scan_grid(cus)
        assert n * 16 > ic.ivf_grid(n * 16, 256, cus) * 256 and n * 4 > ic.ivf_grid(n * 4, 256, cus) * 256
        assert ic.grouper(n, 3).used == -(-n // 1024) and ic.build_chunk(n, 3) == n
        s = c.searches[0]
        scores, ids = _candidates(c, s, 0, built)  # e_0: thousands of ties at the k-th score, far beyond the LDS copy
        p = ic.select_path(scores, ids, s.k)
        assert p.path == "global" and p.digit <= 2 and (scores == np.sort(scores)[-s.k]).sum() > 2 * s.k
        assert ic.search_chunk(len(s.queries), n, 3, f, 3, s.k) == len(s.queries)


def test_coarse_wide_claims():
    vectors, init_rows, queries = ic.coarse_wide()
    nlist, f = len(init_rows), vectors.shape[1]
    assert nlist == 2100 > ic.K_IVF_SURVIVORS and len(set(init_rows.tolist())) == nlist and ic.plan_per(nlist) == 3
    assert f * np.abs(vectors).max() * np.abs(queries).max() < 1 << 24  # the scan is exact
    cent32 = ref.normalise_rows(vectors[init_rows]).astype(np.float32)
    coarse32 = queries.astype(np.float32) @ cent32.T  # a float32 product standing in for the kernel
    assert len(set(ic.bucket(coarse32).ravel().tolist())) == 1 and 112 <= coarse32.min() and coarse32.max() < 128
    coarse = queries.astype(np.float64) @ cent32.astype(np.float64).T
    for P in (1, 10):
        for r in range(len(queries)):
            assert ic.select_path(coarse32[r], np.arange(nlist), P).path == "global"
        got = np.stack([ref.order_desc(row)[:P] for row in coarse32])
        want = np.stack([ref.order_desc(row)[:P] for row in coarse])
        exceptions = ref.audit(got, want, np.take_along_axis(coarse, want, axis=1), lambda r, l: coarse[r, l], f)
        assert exceptions <= 0.01 * got.size


def test_input_claims():
    assert {n for n in ic.names("inputs")} == {"inputs_float32_index_float16_queries", "inputs_float16_index_float32_queries",
                                               "inputs_float16_index_float16_queries"}
    vectors, init_rows, cent0, cent1, assign, queries, scores = ic.overflow()
    assert vectors.dtype == np.float32 and np.isfinite(vectors).all() and np.isfinite(scores).all()
    with np.errstate(over="ignore"):
        assert np.isinf((vectors[init_rows[1]] ** 2).sum(dtype=np.float32))                 # the initial row of list 1
        members = vectors[assign == 0]
        mean = members.sum(axis=0, dtype=np.float32) / np.float32(len(members))
        assert np.isfinite(mean).all() and np.isinf((mean ** 2).sum(dtype=np.float32))      # the updated mean of list 0
    assert (vectors[assign == 1] == [-4, 0]).all() and (assign == 1).sum() == 4             # list 1: mean (-4, 0), norm 4
    assert (scores.astype(np.float32).astype(np.float64) == scores).all()                   # exact in fp32
    # round 0 (centroids e_0 and zero) and the final round (e_0 and -e_0) assign alike
    for cent in (cent0, cent1):
        np.testing.assert_array_equal(ref.argmax_rows(vectors.astype(np.float64) @ cent.astype(np.float64).T), assign)
    assert any(len(set(row.tolist())) < len(row) for row in scores)
