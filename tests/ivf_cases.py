"""The inputs of the IVF-Flat index's edge tests (tests/test_gpu_ivf_edges.py) and a Python restatement of the arithmetic of
csrc/ivf.hip that decides which code runs.  tests/test_ivf_cases_host.py proves on the CPU that every case sits on the cut it
claims and that the integer restatement the GPU is judged by (ivf_reference.exact_build / exact_search) equals the float64
one.  Test infrastructure only; nothing here touches a GPU and this file holds no test.

Why the cases are exact.  Vectors and queries are integer-valued with every score below 2^24, so a score has one possible
fp32 value in any summation order.  The builds run `iterations = 0` from initial rows that are zero or +-2^m e_j, so the
centroids are exactly 0 or +-e_j, the coarse score of a query against list c is +-q[coord c] and the assignment score of a
vector +-v[coord c]: probes, assignment, offsets, ids inside a list, result ids and scores have one answer each.

A case is (vectors, vdtype, init_rows, searches, claims): integer arrays, the storage type the test casts them to, and per
search (queries, qdtype, k, nprobe).  `claims` names what the case was built for; the host test asserts each claim.

Families and the cuts of ivf.hip they sit on:
  factors      f_pad, K steps of 32, elements per thread of the centroid kernels (f = 1 .. 1024), fp32 and fp16 storage
  planted      two k-means rounds at f = 257 / 1024 on integer clusters: the mean, its norm and the division (16 * 2^-24)
  tiles        lists of 0 / 1 / 127 / 128 / 129 / 257 vectors probed by 1 / 63 / 64 / 65 / 129 queries; lists without tiles around
  many_lists   1024 / 1025 / 2048 lists: `per` of the one-workgroup scans, the tile search, the 1024-probe limit
  coarse_wide  2100 general centroids whose coarse scores share one bucket: the coarse select off the scores themselves
  survivors    exactly 2048 / 2049 keys in the boundary bucket and above, the k-th key in the top or the second bucket
  ties         one score for every candidate: the k-th key is decided in byte 0, 1 (and 2: second_trip) of the id
  k_cuts       k = 1, 2, 3, 255 .. 257, 1023, 1024 against probed totals of k - 1, k, k + 1 and 0
  grouping     1 .. 4097 elements over 3 and 300 keys: one run or several, a run that is not 1024, a second colscan group
  counter_cap  more than 2^23 (query, probe) pairs over 2048 keys: the counter table's cap lengthens the runs
  build_chunks n = nlist = 33000: the build's assignment scores exceed the budget and its rows go in two chunks
  second_trip  one list of more than 128 * 8 * CUs vectors: a second trip of every persistent and grid-stride loop
  inputs       fp16 queries on an fp32 index and the reverse, entries of 2^100 whose sum of squares overflows"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

# ---- implicit_amd/csrc/ivf.hip, restated -------------------------------------------------------------------------------
K_IVF_BM = 64
K_IVF_BN = 128
K_IVF_BK = 32
K_IVF_RUN = 1024
K_IVF_MAX_COUNTERS = 1 << 24
K_IVF_SURVIVORS = 2048
K_IVF_MAX_K = 1024
SCAN_WORKGROUPS_PER_CU = 8   # IvfProduct::launch: dim3(num_cus * 8)
GRID_WORKGROUPS_PER_CU = 16  # ivf_grid: at most num_cus * 16 workgroups of 256
DEFAULT_BUDGET = 4 << 30     # ivf_default_budget: min(free / 2, 4 GiB)


def _ceil(a, b):
    return -(-a // b)


def f_pad(f):
    return _ceil(f, 4) * 4


def k_steps(f):
    """Trips of the k0 loop of ivf_scan_kernel."""
    return _ceil(f_pad(f), K_IVF_BK)


def elements_per_thread(f):
    """Trips of `d += 256` in ivf_block_sumsq and the centroid kernels (acc[j], j below this, in ivf_update_centroids_kernel)."""
    return _ceil(f_pad(f), 256)


def tiles(pairs, length):
    """ivf_plan_kernel: the tiles of a list of `length` vectors probed by `pairs` queries."""
    return _ceil(pairs, K_IVF_BM) * _ceil(length, K_IVF_BN) if pairs > 0 and length > 0 else 0


def plan_per(n):
    """Entries per thread of the one-workgroup scans (ivf_plan_kernel, ivf_exclusive_scan_kernel)."""
    return _ceil(n, 1024)


def pow2_pad(k):
    """kpad / ppad of imp_ivf_search."""
    p = 1
    while p < k:
        p <<= 1
    return p


def grouper(n_max, nkeys, n=None):
    """IvfGrouper: (nruns) of the constructor, (run, used) of run() for n elements."""
    n = n_max if n is None else n
    nruns = max(1, min(_ceil(n_max, K_IVF_RUN), K_IVF_MAX_COUNTERS // nkeys))
    per = _ceil(n, nruns)
    run = max(64, _ceil(per, 64) * 64)
    return SimpleNamespace(nruns=nruns, run=run, used=max(1, _ceil(n, run)))


def scan_grid(num_cus):
    return num_cus * SCAN_WORKGROUPS_PER_CU


def ivf_grid(work, block, num_cus):
    return min(_ceil(work, block), num_cus * GRID_WORKGROUPS_PER_CU)


def build_chunk(n, nlist, budget=DEFAULT_BUDGET):
    """Rows per assignment chunk of imp_ivf_build."""
    return min(n, max(K_IVF_BM, budget // (4 * nlist)))


def search_chunk(nq, longest, nlist, f, P, k, budget=DEFAULT_BUDGET):
    """Queries per chunk of imp_ivf_search; `longest` = the sum of the P longest lists' lengths."""
    per_query = 4 * (max(longest, nlist) + f_pad(f) + P + k) + 4 * (3 * P + k)
    return min(nq, max(1, budget // per_query))


def ordered(scores):
    """select_ops.h ordered(): float32 -> uint32 of the same order, -0.0 as +0.0."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def bucket(scores):
    """The 11-bit bucket of ivf_select_kernel's first pass: key >> 53 = ordered(score) >> 21."""
    return ordered(scores) >> np.uint32(21)


def select_path(scores, ids, k):
    """What ivf_select_kernel does with these candidates: .path "all" (total <= k, no select), "lds" (the boundary bucket and
    those above hold at most kIvfSurvivors keys) or "global"; .n_lds those keys, .above the keys above the boundary bucket
    (found[1]), .digit the byte of the 64-bit key at which the radix select stops (bytes 0 .. 3 are the id's)."""
    keys = (ordered(scores).astype(np.uint64) << np.uint64(32)) | np.asarray(ids).astype(np.uint64)
    total = len(keys)
    if total <= k:
        return SimpleNamespace(total=total, path="all", n_lds=0, above=0, digit=None)
    b = keys >> np.uint64(53)
    first = np.sort(keys)[total - k] >> np.uint64(53)
    above, n_lds = int((b > first).sum()), int((b >= first).sum())
    path = "lds" if n_lds <= K_IVF_SURVIVORS else "global"
    pool = keys[b >= first] if path == "lds" else keys
    prefix, mask, remaining, stop = np.uint64(0), np.uint64(0), k, 0
    for digit in range(7, -1, -1):
        shift = np.uint64(8 * digit)
        hist = np.bincount(((pool[(pool & mask) == prefix] >> shift) & np.uint64(0xFF)).astype(np.int64), minlength=256)
        acc, bb = 0, 255
        while bb > 0 and acc + hist[bb] < remaining:
            acc += hist[bb]
            bb -= 1
        prefix, mask, remaining = prefix | (np.uint64(bb) << shift), mask | (np.uint64(0xFF) << shift), remaining - acc
        if hist[bb] == remaining:
            stop = digit
            break
    return SimpleNamespace(total=total, path=path, n_lds=n_lds, above=above, digit=stop)


# ---- planted lists -----------------------------------------------------------------------------------------------------
def _spec(rng, dirs, zeros=0):
    """dirs: (coord, sign, count, empty duplicates) per direction.  Returns the lists in id order as (coord, sign, count):
    list ids are shuffled, the members of a direction belong to the LAST list of that direction (a tie goes to the larger
    list id), so its duplicates are empty; `zeros` lists get a zero initial row (a zero centroid, empty); the last list is
    non-empty, because the zero rows tie everywhere and go there."""
    entries = []
    for j, s, c, dup in dirs:
        assert s in (-1, 1) and c >= dup + 1
        entries += [(j, s, c)] + [(j, s, 0)] * dup
    entries += [(0, 0, 0)] * zeros
    while True:
        spec = [entries[i] for i in rng.permutation(len(entries))]
        at = {}
        for i, (j, s, c) in enumerate(spec):
            if s:
                at.setdefault((j, s), []).append(i)
        for (j, s), where in at.items():
            c = max(spec[i][2] for i in where)
            for i in where:
                spec[i] = (j, s, c if i == where[-1] else 0)
        j, s, c = spec[-1]
        if s and c >= len(at[(j, s)]) + zeros:
            return spec


def _planted(rng, f, spec, big=(64, 127), noise=3):
    """(vectors int64 [n x f], init_rows [nlist], sizes [nlist]).  A member of list (j, s) has v[j] = s * a with a in `big`
    and every other entry within +-noise < a, so its best list is that direction's last list and nothing ties; the initial
    rows are one-hot powers of two among the members (zero rows among the last list's).  Rows are shuffled."""
    assert noise < big[0]
    nlist = len(spec)
    last = {(j, s): l for l, (j, s, c) in enumerate(spec) if s}
    zero_lists = [l for l, (j, s, c) in enumerate(spec) if not s]
    lists_of = {}
    for l, (j, s, c) in enumerate(spec):
        lists_of.setdefault((j, s), []).append(l)
    blocks, init_at, base = [], {}, 0
    for l, (j, s, c) in enumerate(spec):
        if not s or last[(j, s)] != l:
            assert c == 0
            continue
        block = rng.integers(-noise, noise + 1, size=(c, f))
        block[:, j] = s * rng.integers(big[0], big[1] + 1, size=c)
        owners = lists_of[(j, s)]
        for t, d in enumerate(owners):
            block[t] = 0
            block[t, j] = s * 2 ** int(rng.integers(0, 7))
            init_at[d] = base + t
        if l == nlist - 1:
            for t, z in enumerate(zero_lists):
                block[len(owners) + t] = 0
                init_at[z] = base + len(owners) + t
        blocks.append(block)
        base += c
    vectors = np.concatenate(blocks).astype(np.int64)
    perm = rng.permutation(len(vectors))
    place = np.empty(len(vectors), dtype=np.int64)
    place[perm] = np.arange(len(vectors))
    init_rows = np.array([place[init_at[l]] for l in range(nlist)], dtype=np.int64)
    return vectors[perm], init_rows, np.array([c for _, _, c in spec], dtype=np.int64)


def _dominant(rng, f, dirs_counts, big=(8, 15), noise=2):
    """Queries with one dominant coordinate: `count` of them per (coord, sign), shuffled.  Under nprobe = 1 such a query
    probes that direction's last list."""
    rows = []
    for (j, s), count in dirs_counts:
        block = rng.integers(-noise, noise + 1, size=(count, f))
        block[:, j] = s * rng.integers(big[0], big[1] + 1, size=count)
        rows.append(block)
    q = np.concatenate(rows).astype(np.int64)
    return q[rng.permutation(len(q))]


def search_spec(queries, k, nprobe, qdtype="float32"):
    """repeat = R (counter_cap only): the search runs R queries, query r being row r % len(queries)."""
    return SimpleNamespace(queries=np.asarray(queries, dtype=np.int64), k=k, nprobe=nprobe, qdtype=qdtype, repeat=None)


def _case(family, vectors, init_rows, searches, claims, vdtype="float32"):
    return SimpleNamespace(family=family, vectors=vectors, vdtype=vdtype, init_rows=np.asarray(init_rows, dtype=np.int64),
                           nlist=len(init_rows), searches=searches, claims=claims)


def _directions(f):
    return [(j, s) for j in range(f) for s in (1, -1)]


# ---- factors -----------------------------------------------------------------------------------------------------------
FACTORS = (1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 1021, 1024)


@lru_cache(maxsize=None)
def _factors(f, vdtype):
    rng = np.random.default_rng(1000 + f)
    dirs = _directions(f)
    picked = [dirs[i] for i in rng.permutation(len(dirs))[:24]]
    spec = _spec(rng, [(j, s, int(rng.integers(5, 31)), 1 if t < 2 else 0) for t, (j, s) in enumerate(picked)], zeros=1)
    vectors, init_rows, sizes = _planted(rng, f, spec)
    queries = rng.integers(-4, 5, size=(70, f))
    other = "float16" if vdtype == "float32" else "float32"
    searches = [search_spec(queries, 10, 3), search_spec(queries[:9], 50, len(spec), other)]
    return _case("factors", vectors, init_rows, searches, {"f": f, "sizes": sizes}, vdtype)


# ---- planted clusters, two k-means rounds ------------------------------------------------------------------------------
PLANTED_FACTORS = (257, 1024)
PLANTED_TOLERANCE = 16 * 2.0 ** -24  # relative, per centroid element (twice the bound derived in the host test)


@lru_cache(maxsize=None)
def planted(f):
    """400 vectors 64 e_c + integer noise in [-3, 3] around 16 coordinates spread over [0, f); initial row c = the first
    member of cluster c.  Returns (vectors int64, init_rows, iterations)."""
    rng = np.random.default_rng(2000 + f)
    nlist, n = 16, 400
    coords = np.sort(rng.choice(f, size=nlist, replace=False))
    coords[-1] = f - 1  # the last element of the last thread's last trip
    cluster = np.arange(n) % nlist
    vectors = rng.integers(-3, 4, size=(n, f))
    vectors[np.arange(n), coords[cluster]] += 64
    return vectors.astype(np.int64), np.arange(nlist), 2


# ---- tiles -------------------------------------------------------------------------------------------------------------
TILE_LENS = (0, 1, 127, 128, 129, 257)
TILE_QUERIES = (1, 63, 64, 65, 129)


@lru_cache(maxsize=None)
def _tiles():
    """f = 20.  One list per (length, query count) with length in 1 .. 257; the five lists of 257 vectors have an empty
    duplicate each, which the same queries probe second (the length-0 column); three lists nobody probes and a zero list."""
    rng = np.random.default_rng(3000)
    f = 20
    free = iter(_directions(f)[i] for i in rng.permutation(2 * f))
    dirs, targets = [], []
    for length in TILE_LENS[1:]:
        for count in TILE_QUERIES:
            j, s = next(free)
            dirs.append((j, s, length, 1 if length == 257 else 0))
            targets.append(((j, s), count))
    unprobed = [(*next(free), c, 0) for c in (5, 200, 2)]
    quiet = {(j, s) for j, s, _, _ in unprobed}
    while True:  # a list that no query of one probe reaches at either end of the id range
        spec = _spec(rng, dirs + unprobed, zeros=1)
        if spec[-1][:2] in quiet and (spec[0][2] == 0 or spec[0][:2] in quiet):
            break
    vectors, init_rows, sizes = _planted(rng, f, spec)
    queries = _dominant(rng, f, targets)
    searches = [search_spec(queries, 10, 1), search_spec(queries, 300, 2), search_spec(queries[:100], 40, 7, "float16")]
    return _case("tiles", vectors, init_rows, searches,
                 {"sizes": sizes, "spec": spec, "targets": targets, "unprobed": [(j, s) for j, s, _, _ in unprobed]})


# ---- many lists ----------------------------------------------------------------------------------------------------------
MANY_LISTS = (1024, 1025, 2048)


@lru_cache(maxsize=None)
def _many_lists(nlist):
    """f = 1024, nlist - 40 directions and 40 empty duplicates, n = nlist + 100."""
    rng = np.random.default_rng(4000 + nlist)
    f = 1024
    dirs = _directions(f)
    picked = [dirs[i] for i in rng.permutation(len(dirs))[:nlist - 40]]
    plan = [[j, s, 1, 0] for j, s in picked]
    for t in range(40):
        plan[t][2], plan[t][3] = 2, 1
    for t in rng.integers(0, len(plan), size=100):
        plan[t][2] += 1
    spec = _spec(rng, [tuple(p) for p in plan])
    vectors, init_rows, sizes = _planted(rng, f, spec)
    queries = rng.integers(-4, 5, size=(6, f))
    searches = [search_spec(queries, 10, 1), search_spec(queries, 10, 1023), search_spec(queries, 1024, 1024),
                search_spec(queries[:2], 3, 1024)]
    return _case("many_lists", vectors, init_rows, searches, {"sizes": sizes})


# ---- counter cap -------------------------------------------------------------------------------------------------------
COUNTER_CAP_QUERIES = (1 << 23) // K_IVF_MAX_K + 1  # 8193 queries x 1024 probes: the first pair count above 2^23
COUNTER_CAP_DISTINCT = 16


@lru_cache(maxsize=None)
def _counter_cap():
    """The index of many_lists_2048 under 8193 queries of 1024 probes.  Query r is row r % 16 of 16 distinct queries, so the
    expected result is that of 16 queries repeated (the restatement stays cheap) while the pairs of equal queries sit in
    different runs of the grouping."""
    base = _many_lists(2048)
    rng = np.random.default_rng(4999)
    distinct = rng.integers(-4, 5, size=(COUNTER_CAP_DISTINCT, 1024))
    search = search_spec(distinct, 10, K_IVF_MAX_K)
    search.repeat = COUNTER_CAP_QUERIES
    return _case("counter_cap", base.vectors, base.init_rows, [search], dict(base.claims))


# ---- coarse select beyond the LDS copy ---------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def coarse_wide():
    """(vectors int64 [2300 x 8], init_rows [2100], queries int64 [40 x 8]).  Every vector is (1000, seven entries in
    [-100, 100]): the 2100 general centroids lie within 15 degrees of e_0, so against a query (120, noise in [-3, 3]) all
    2100 coarse scores fall into the bucket [112, 128)."""
    rng = np.random.default_rng(5000)
    vectors = rng.integers(-100, 101, size=(2300, 8))
    vectors[:, 0] = 1000
    queries = rng.integers(-3, 4, size=(40, 8))
    queries[:, 0] = 120
    return vectors.astype(np.int64), rng.choice(2300, size=2100, replace=False), queries.astype(np.int64)


# ---- survivors ---------------------------------------------------------------------------------------------------------
SURVIVOR_CASES = {  # name: (keys in the top bucket [1280, 1536), keys in the second bucket [1024, 1280), k)
    "top_2048": (2048, 500, 600), "top_2049": (2049, 500, 600), "second_2048": (500, 1548, 600), "second_2049": (500, 1549, 600)}


@lru_cache(maxsize=None)
def _survivors(which, four):
    """f = 2, query (1, 0): a vector's score is its first coordinate.  `four`: the second coordinate (0, +-4000) sends the
    vectors to the lists +e_0, -e_0, +e_1, -e_1; otherwise one list holds them all."""
    top, second, k = SURVIVOR_CASES[which]
    rng = np.random.default_rng(6000 + top + second + four)
    first = np.concatenate([rng.integers(1280, 1536, size=top), rng.integers(1024, 1280, size=second),
                            rng.integers(3, 1024, size=300), -rng.integers(3, 1024, size=50)])
    vectors = np.stack([first, rng.choice([0, 4000, -4000], size=len(first)) if four else np.zeros(len(first), dtype=np.int64)], axis=1)
    onehot = np.array([[2, 0], [-2, 0], [0, 2], [0, -2]]) if four else np.array([[2, 0]])
    vectors = np.concatenate([vectors, onehot])
    perm = rng.permutation(len(vectors))
    place = np.empty(len(vectors), dtype=np.int64)
    place[perm] = np.arange(len(vectors))
    init_rows = place[len(first) + rng.permutation(len(onehot))]
    return _case("survivors", vectors[perm].astype(np.int64), init_rows, [search_spec([[1, 0]], k, 4)],
                 {"n_lds": top if which.startswith("top") else top + second, "second": which.startswith("second")})


# ---- ties --------------------------------------------------------------------------------------------------------------
TIE_CASES = ((200, (10, 199)), (2000, (100, 208, 1024)), (3000, (100, 184, 1024)))  # n, ks


@lru_cache(maxsize=None)
def _ties(n):
    """n vectors (8, 0) in one list (and an empty duplicate of it): every candidate of the query (1, 0) scores 8, so the k
    winners are the k largest ids and the select is decided in the id bytes alone."""
    vectors = np.zeros((n, 2), dtype=np.int64)
    vectors[:, 0] = 8
    ks = dict(TIE_CASES)[n]
    return _case("ties", vectors, [n // 3, n // 2], [search_spec([[1, 0]], k, 2) for k in ks], {"n": n})


# ---- k cuts ------------------------------------------------------------------------------------------------------------
K_CUTS = (1, 2, 3, 255, 256, 257, 1023, 1024)


def k_cut_sizes():
    return sorted({t for k in K_CUTS for t in (k - 1, k, k + 1)} - {0})


@lru_cache(maxsize=None)
def _k_cuts():
    """f = 13, one list +e_j per size of k_cut_sizes() and a zero list, which is empty.  A query dominant in coordinate j probes
    (nprobe = 1) the list of that size; the query of -1s scores below zero against every +e_j and probes the empty list."""
    rng = np.random.default_rng(7000)
    sizes = k_cut_sizes()
    f = len(sizes)
    spec = _spec(rng, [(j, 1, c, 0) for j, c in enumerate(sizes)], zeros=1)
    vectors, init_rows, got_sizes = _planted(rng, f, spec)
    searches = []
    for k in K_CUTS:
        q = _dominant(rng, f, [((sizes.index(t), 1), 1) for t in (k - 1, k, k + 1, 1025) if t > 0])
        searches.append(search_spec(np.concatenate([q, -np.ones((1, f), dtype=np.int64)]), k, 1))
    return _case("k_cuts", vectors, init_rows, searches, {"sizes": got_sizes})


# ---- grouping ----------------------------------------------------------------------------------------------------------
GROUP_NS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)
GROUP_KEYS = (3, 300)
GROUP_SEARCHES = {  # keys: (queries, nprobe) whose product is each of GROUP_NS
    3: ((1, 1), (21, 3), (64, 1), (65, 1), (341, 3), (512, 2), (1025, 1), (683, 3), (4097, 1)),
    300: ((1, 1), (21, 3), (32, 2), (13, 5), (341, 3), (512, 2), (205, 5), (683, 3), (241, 17))}


@lru_cache(maxsize=None)
def _grouping(n, keys, searched=False):
    """n vectors over min(n, keys) lists of random sizes >= 1 (f = 2 for 3 keys, 150 for 300); `searched` adds the searches of
    GROUP_SEARCHES, whose (query, probe) pairs go through the same grouping."""
    rng = np.random.default_rng(8000 + 10 * n + keys)
    f = 2 if keys == 3 else 150
    nlist = min(n, keys)
    dirs = _directions(f)[:nlist]
    counts = 1 + rng.multinomial(n - nlist, rng.dirichlet(np.ones(nlist)))
    spec = _spec(rng, [(j, s, int(c), 0) for (j, s), c in zip(dirs, counts)])
    vectors, init_rows, sizes = _planted(rng, f, spec)
    searches = []
    if searched:
        queries = rng.integers(-4, 5, size=(4097, f))
        searches = [search_spec(queries[:rows], 5, P) for rows, P in GROUP_SEARCHES[keys]]
    return _case("grouping", vectors, init_rows, searches, {"sizes": sizes, "n": n, "keys": nlist})


# ---- the build's row chunks --------------------------------------------------------------------------------------------
BUILD_CHUNKS_N = 33000  # n = nlist: n * nlist * 4 bytes of assignment scores exceed the 4 GiB budget


@lru_cache(maxsize=None)
def build_chunks(n=BUILD_CHUNKS_N):
    """n = nlist one-hot rows +-2^m e_j at f = 4, every row the initial row of one list: eight directions with thousands of
    duplicate centroids each, so every vector belongs to the LAST list of its direction and all other lists are empty.
    Returns (vectors int64, init_rows, assign, queries): the n x nlist score matrix is never formed on the host."""
    rng = np.random.default_rng(8500 + n)
    f = 4
    j, s = rng.integers(0, f, size=n), rng.choice([-1, 1], size=n)
    vectors = np.zeros((n, f), dtype=np.int64)
    vectors[np.arange(n), j] = s * 2 ** rng.integers(0, 7, size=n)
    init_rows = rng.permutation(n)
    direction = 2 * j + (s < 0)
    last = np.zeros(2 * f, dtype=np.int64)
    last[direction[init_rows]] = np.arange(n)  # repeated indices: the last assignment, the largest list id, stays
    queries = np.array([[3, -1, 0, 2], [0, 0, 0, 0], [-2, -2, 1, 1]], dtype=np.int64)
    return vectors, init_rows, last[direction], queries


# ---- second trip -------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def second_trip(num_cus):
    """f = 16, three lists; the list +e_0 holds 128 * 8 * num_cus + 300 vectors, so one query alone needs more tiles than
    the scan has workgroups.  Queries: e_0 (scores 64 .. 127, thousands of ties at each), zero (every vector scores 0: the k
    largest ids win, decided in byte 2 of the id), -e_0, and one small general query."""
    rng = np.random.default_rng(9000 + num_cus)
    f, long = 16, K_IVF_BN * SCAN_WORKGROUPS_PER_CU * num_cus + 300
    spec = _spec(rng, [(0, 1, long, 0), (0, -1, 700, 0), (5, 1, 300, 0)])
    vectors, init_rows, sizes = _planted(rng, f, spec, noise=2)
    queries = np.zeros((4, f), dtype=np.int64)
    queries[0, 0], queries[2, 0] = 1, -1
    queries[3] = rng.integers(-2, 3, size=f)
    return _case("second_trip", vectors, init_rows, [search_spec(queries, 1000, 3), search_spec(queries[:2], 7, 1)],
                 {"sizes": sizes, "long": long, "num_cus": num_cus})


# ---- inputs ------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _widening(vdtype, qdtype):
    base = _factors(33, "float32")
    return _case("inputs", base.vectors, base.init_rows, [search_spec(base.searches[0].queries, 20, 5, qdtype)], dict(base.claims), vdtype)


BIG = 2.0 ** 100


def overflow():
    """f = 2.  Row 1 = (2^100, 2^100) is the initial row of list 1: its sum of squares overflows, so centroid 1 starts as
    zero.  Round 0: rows with x > 0 go to list 0 (centroid e_0; the two big rows among them), rows with x <= 0 to list 1
    (score 0 against the zero centroid, ties to the larger list).  Update: list 0's mean has a 2^99-sized entry whose
    square overflows, so centroid 0 is KEPT at e_0; list 1's members are all (-4, 0), mean (-4, 0), centroid -e_0
    exactly.  Final assignment: x > 0 to list 0, x <= 0 to list 1.  Returns (vectors float32, init_rows, centroids after 0
    rounds, centroids after 1 round, the assignment (the same after both), queries, scores of every query and vector)."""
    x = np.array([1, BIG, 3, -4, 5, -4, BIG, -4, 7, -4], dtype=np.float32)
    y = np.array([0, BIG, 0, 0, 0, 0, BIG, 0, 0, 0], dtype=np.float32)
    vectors = np.stack([x, y], axis=1)
    assign = np.where(x > 0, 0, 1)
    queries = np.array([[1, 0], [1, 1], [-2, 0]], dtype=np.float32)
    scores = queries.astype(np.float64) @ vectors.astype(np.float64).T  # sums of at most two powers of two: exact
    return (vectors, np.array([0, 1]), np.array([[1, 0], [0, 0]], dtype=np.float32), np.array([[1, 0], [-1, 0]], dtype=np.float32),
            assign, queries, scores)


# ---- the table ---------------------------------------------------------------------------------------------------------
_TABLE = {}
for _f in FACTORS:
    _TABLE[f"factors_f{_f}_fp32"] = (lambda f=_f: _factors(f, "float32"))
    _TABLE[f"factors_f{_f}_fp16"] = (lambda f=_f: _factors(f, "float16"))
_TABLE["tiles"] = _tiles
for _n in MANY_LISTS:
    _TABLE[f"many_lists_{_n}"] = (lambda n=_n: _many_lists(n))
_TABLE["counter_cap"] = _counter_cap
for _w in SURVIVOR_CASES:
    _TABLE[f"survivors_{_w}_one_list"] = (lambda w=_w: _survivors(w, False))
    _TABLE[f"survivors_{_w}_four_lists"] = (lambda w=_w: _survivors(w, True))
for _n, _ in TIE_CASES:
    _TABLE[f"ties_n{_n}"] = (lambda n=_n: _ties(n))
_TABLE["k_cuts"] = _k_cuts
for _keys in GROUP_KEYS:
    for _n in GROUP_NS:
        if _keys == 3 or _n >= 300:
            _TABLE[f"grouping_n{_n}_keys{_keys}"] = (lambda n=_n, keys=_keys: _grouping(n, keys, n == 1025))
for _v, _q in (("float32", "float16"), ("float16", "float32"), ("float16", "float16")):
    _TABLE[f"inputs_{_v}_index_{_q}_queries"] = (lambda v=_v, q=_q: _widening(v, q))
NAMES = list(_TABLE)


def names(family):
    return [n for n in NAMES if get_family(n) == family]


def get_family(name):
    for family in ("factors", "tiles", "many_lists", "counter_cap", "survivors", "ties", "k_cuts", "grouping", "inputs"):
        if name.startswith(family):
            return family
    raise KeyError(name)


def get(name):
    """The exact case `name`.  Arrays are built once and shared: treat them as read-only."""
    c = _TABLE[name]()
    return SimpleNamespace(name=name, **vars(c))


def cast(array, dtype):
    """The integer array in its storage type; the values must survive (fp16: magnitudes up to 2048)."""
    out = np.asarray(array).astype(dtype)
    assert (out.astype(np.int64) == np.asarray(array)).all()
    return out
