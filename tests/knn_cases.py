"""The inputs of the sparse top-k product's edge tests (tests/test_gpu_knn_edges.py).  tests/test_knn_cases_host.py proves on
the CPU that every case is what it claims to be and that the restatement the GPU is judged by (knn_reference.product_topk) is
bitwise a literal triple loop.  Test infrastructure only; nothing here touches a GPU and this file holds no test.

A case is (A, B, k, zero_own) with A and B scipy CSR matrices built directly from (data, indices, indptr): the stored order of
a row's entries, repeated columns and explicit zeros survive, because the order of A[r] is the summation order of the contract.
Every case has A.cols == B.rows == B.cols except the stored-order and batch-edge ones, so zero_own is allowed almost everywhere.
`claims` names the properties a case was built for; the host test asserts each of them.

The cuts of csrc/knn.hip that the families sit on (restated below, see knn_hash, kHashSlots and kHashLimit there):
  stored_order  unsorted A rows with repeats, stored zeros, negative weights, 16 decades of magnitude (hash pass)
  batch_edges   A rows and B rows of 0, 1, 63, 64, 65, 128, 129 entries: the 64-entry batches of KnnEntries and the lane steps
  table_cut     rows touching exactly 1535, 1536, 1537, 1600 columns: kHashLimit, where a row leaves the LDS table
  probe_wrap    C = 65536, columns chosen by hash: a 1536-column cluster in the last 384 slots, and one slot's whole chain
  select_*      k at 64 / 65 (TopList<1> / <4>) and 256 / 257, 512 / 513 (selection rounds), touched counts around every k
  own_*         zero_own rows whose zeroed columns rank first, liked but untouched columns, repeated own columns; both passes
  dense_reuse   more overflow rows than twice the dense workers: every worker's accumulator and touched list are reused
  empty_*       no rows, only empty rows, an empty B, A entries that reach only empty B rows"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

# implicit_amd/csrc/knn.hip
K_HASH_SLOTS = 2048
K_HASH_LIMIT = 1536
BATCH = 64  # entries of A[r] per KnnEntries load, and of B[u] per lane step
DENSE_WORKERS_PER_CU = 4

BATCH_LENS = (0, 1, 63, 64, 65, 128, 129)
CUT_TOUCHED = (1535, 1536, 1537, 1600)
KS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
EXTRA_KS = (1536, 1537, 1538, 5000)  # counts around k on dense-pass rows, and k > C
TIE_LEVELS = (40, 300)  # columns with a 3-term and with an at least 2-term sum in a tie row
REUSE_ROWS = 2500
MAX_SOLO_ROWS = 64  # the cut cases stay below this, so that every row can also be run alone


def knn_hash(j):
    """knn.hip knn_hash: Knuth's multiplicative hash of a column id, the top 11 bits of the 32-bit product."""
    return ((np.asarray(j, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)).astype(np.int64) \
        & (K_HASH_SLOTS - 1)


def dense_workers(num_cus, C):
    """The number of dense-pass workers imp_sparse_topk_product launches."""
    return max(1, min(num_cus * DENSE_WORKERS_PER_CU, (3 << 29) // max(1, C * 12)))


def probe_slots(cols):
    """Slot of every column after inserting `cols` in this order with linear probing.  The SET of occupied slots does not
    depend on the order (so not on which lane of a step wins a slot), only a column's own slot does."""
    table = np.full(K_HASH_SLOTS, -1, dtype=np.int64)
    slots = np.empty(len(cols), dtype=np.int64)
    for i, (c, s) in enumerate(zip(np.asarray(cols).tolist(), knn_hash(cols).tolist())):
        while table[s] != -1:
            s = (s + 1) & (K_HASH_SLOTS - 1)
        table[s] = c
        slots[i] = s
    return slots


def csr_from_rows(rows, ncols):
    """CSR with exactly these entries in exactly this order; rows is a list of (column ids, values)."""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(i) for i, _ in rows])
    indices = np.concatenate([np.asarray(i, dtype=np.int32) for i, _ in rows] + [np.zeros(0, np.int32)])
    data = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows] + [np.zeros(0)])
    m = sp.csr_matrix((data, indices, indptr), shape=(len(rows), ncols))
    assert np.array_equal(m.indices, indices) and np.array_equal(m.data.view(np.int64), data.view(np.int64))
    return m


def csr_from_dict(rows, nrows, ncols):
    empty = (np.zeros(0, np.int32), np.zeros(0))
    return csr_from_rows([rows.get(u, empty) for u in range(nrows)], ncols)


def one_row(A, r):
    """Row r of A alone, entries as stored."""
    lo, hi = A.indptr[r], A.indptr[r + 1]
    return csr_from_rows([(A.indices[lo:hi], A.data[lo:hi])], A.shape[1])


def touched_counts(A, B):
    """Distinct columns reached by every row of A."""
    out = np.zeros(A.shape[0], dtype=np.int64)
    for r in range(A.shape[0]):
        us = A.indices[A.indptr[r]:A.indptr[r + 1]]
        if len(us):
            out[r] = len(np.unique(np.concatenate([B.indices[B.indptr[u]:B.indptr[u + 1]] for u in us])))
    return out


def pair_count(A, B):
    return int(np.diff(B.indptr)[A.indices].sum())


def row_flags(A):
    """(rows with an unsorted stored order, rows with a repeated column)."""
    unsorted = dup = 0
    for r in range(A.shape[0]):
        i = A.indices[A.indptr[r]:A.indptr[r + 1]]
        unsorted += bool(np.any(np.diff(i) < 0))
        dup += len(np.unique(i)) < len(i)
    return unsorted, dup


def _wide(rng, n):
    """Both signs, magnitudes over 16 decades: any other summation order changes bits."""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8.0, 8.0, n)


def _subset(rng, pool, n):
    return np.sort(rng.choice(pool, n, replace=False)).astype(np.int32)


# ---- stored order ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _stored_order():
    rng = np.random.default_rng(101)
    U, C = 300, 400
    brows = []
    for _ in range(U):
        cols = _subset(rng, C, rng.binomial(C, 0.2))
        vals = _wide(rng, len(cols))
        vals[rng.random(len(cols)) < 0.05] = 0.0
        brows.append((cols, vals))
    brows[7][1][:2] = 0.0  # row 1 of A reaches these with a negative weight: sums of -0.0 terms only
    lens = [0, 1, 130, 1, 64, 65] + rng.integers(2, 130, 34).tolist()
    arows = []
    for n in lens:
        vals = _wide(rng, n)
        vals[rng.random(n) < 0.05] = 0.0
        arows.append((rng.integers(0, U, n), vals))  # drawn with replacement, left as drawn
    arows[1] = ([7], [-3.0])
    return csr_from_rows(arows, U), csr_from_rows(brows, C), {"neg_zero_row": 1}


# ---- batch edges -------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _batch_edges():
    """A row (la, lb): la entries, each reaching one of three B rows of lb entries (so sums have about la / 3 terms)."""
    rng = np.random.default_rng(102)
    C, per = 300, 3
    brows = []
    for lb in BATCH_LENS:
        for _ in range(per):
            brows.append((_subset(rng, C, lb), _wide(rng, lb)))
    arows, shape = [], []
    for la in BATCH_LENS:
        for g, lb in enumerate(BATCH_LENS):
            arows.append((g * per + rng.integers(0, per, la), _wide(rng, la)))
            shape.append((la, lb))
    return csr_from_rows(arows, len(brows)), csr_from_rows(brows, C), {"shape": shape}


# ---- table cut ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _table_cut(C, seed):
    """For every T of CUT_TOUCHED three rows that touch exactly T columns: `single` through one B row of T entries; `overlap`
    through 30 A entries over 24 B rows of 448 entries that cover the T columns about 7 times; `late` through one B row of T
    entries and then 300 A entries over short B rows inside the same T columns.  Light rows and an empty row sit between."""
    rng = np.random.default_rng(seed)
    free = iter(rng.permutation(C).tolist())  # B row ids, each used once
    b, arows, kinds = {}, [], []
    for T in CUT_TOUCHED:
        S = rng.permutation(C)[:T]
        u = next(free)
        b[u] = (np.sort(S).astype(np.int32), _wide(rng, T))
        arows.append(([u], _wide(rng, 1)))
        kinds.append(("single", T))
        us = []
        for g in range(24):
            u = next(free)
            us.append(u)
            b[u] = (np.sort(S[(g * 64 + np.arange(448)) % T]).astype(np.int32), _wide(rng, 448))
        idx = np.concatenate([us, rng.choice(us, 6)])
        rng.shuffle(idx)
        arows.append((idx, _wide(rng, len(idx))))
        kinds.append(("overlap", T))
        u, short = next(free), []
        b[u] = (np.sort(S).astype(np.int32), _wide(rng, T))
        for _ in range(40):
            v = next(free)
            short.append(v)
            n = int(rng.integers(5, 41))
            b[v] = (_subset(rng, S, n), _wide(rng, n))
        idx = np.concatenate([[u], rng.choice(short, 300)])
        arows.append((idx, _wide(rng, len(idx))))
        kinds.append(("late", T))
        light = rng.choice(short, 5)
        arows.append((light, _wide(rng, 5)))
        kinds.append(("light", None))
    arows.insert(3, (np.zeros(0, np.int32), np.zeros(0)))
    kinds.insert(3, ("empty", 0))
    return csr_from_rows(arows, C), csr_from_dict(b, C, C), {"kinds": kinds}


# ---- probe wrap and clustering -----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _probe_wrap():
    """Row 0: 1500 columns that all hash into the last 384 slots, then (a later A entry, so later steps) 36 more that include
    the row's own columns: the cluster has filled slots 1664 .. 2047 by then, so these sit past the wrap and zero_own's lookup
    has to follow them there.  Row 1: every column below C that hashes to one slot near the end of the table, twice."""
    rng = np.random.default_rng(103)
    C = 65536
    h = knn_hash(np.arange(C))
    pool = rng.permutation(np.flatnonzero(h >= K_HASH_SLOTS - 384))
    first, late = pool[:1500], pool[1500:1536]
    u1, u2, u3 = (int(x) for x in late[:3])
    b = {u1: (np.sort(first).astype(np.int32), _wide(rng, 1500)),
         u2: (np.sort(late).astype(np.int32), _wide(rng, 36)),
         u3: (_subset(rng, pool[:1536], 200), _wide(rng, 200))}
    tail = np.arange(K_HASH_SLOTS - 24, K_HASH_SLOTS - 4)
    slot = int(tail[np.argmax(np.bincount(h, minlength=K_HASH_SLOTS)[tail])])
    chain = np.flatnonzero(h == slot)
    v1, v2 = int(chain[0]), int(chain[-1])
    b[v1] = (chain.astype(np.int32), _wide(rng, len(chain)))
    b[v2] = (chain[::-1].astype(np.int32).copy(), _wide(rng, len(chain)))
    arows = [([u1, u2, u3], _wide(rng, 3)), ([v1, v2], _wide(rng, 2)), ([u3, v1], _wide(rng, 2))]
    return csr_from_rows(arows, C), csr_from_dict(b, C, C), {"cluster": (first, late), "own": (u1, u2, u3), "slot": slot,
                                                             "chain": chain}


# ---- selection cuts ----------------------------------------------------------------------------------------------------
def select_touched():
    """The touched counts of the selection cases' rows: k - 1, k, k + 1 of every k that a table row can hold, the table cut
    itself, and dense-pass rows (1537 and 1538 sit at k - 1, k, k + 1 of EXTRA_KS; 1800 and 3000 are far above every k)."""
    t = {x for k in KS for x in (k - 1, k, k + 1) if 1 <= x <= K_HASH_LIMIT}
    return sorted(t | {1535, 1536, 1537, 1538, 1800, 3000})


@lru_cache(maxsize=None)
def _select(ties):
    """One row per touched count t: three A entries over nested B rows of t, min(t, 300) and min(t, 40) columns.  With every
    value 1.0 the scores are 3.0 on 40 columns, 2.0 on the next 260 and 1.0 on the rest: runs of ties over positions 0 .. 39,
    40 .. 299 (across 64 and 256) and 300 .. t - 1 (across 512), ordered by column descending alone."""
    rng = np.random.default_rng(104 + ties)
    C = 4096
    free = iter(rng.permutation(C).tolist())
    b, arows = {}, []
    for t in select_touched():
        S = rng.permutation(C)[:t]
        us = []
        for n in (t, min(t, TIE_LEVELS[1]), min(t, TIE_LEVELS[0])):
            u = next(free)
            us.append(u)
            b[u] = (np.sort(S[:n]).astype(np.int32), np.ones(n) if ties else _wide(rng, n))
        rng.shuffle(us)
        arows.append((us, np.ones(3) if ties else _wide(rng, 3)))
    return csr_from_rows(arows, C), csr_from_dict(b, C, C), {"touched": select_touched()}


# ---- zeroed own columns ------------------------------------------------------------------------------------------------
OWN_TOUCHED = (200, 1700)  # one row per pass


@lru_cache(maxsize=None)
def _own():
    """Per row: 8 own columns that are touched, 2 that are liked but touched by nothing, one own column stored three times.
    Weights are positive and B is negative, so every score that is not zeroed is negative and the 8 zeroed columns lead."""
    rng = np.random.default_rng(105)
    C = 4096
    perm = rng.permutation(C)
    b, arows, own_t, own_u, at = {}, [], [], [], 0
    for t in OWN_TOUCHED:
        S, outside = perm[at:at + t], perm[at + t:at + t + 2]
        at += t + 2
        own = S[:8]
        for i, u in enumerate(own.tolist()):
            cols = np.sort(S) if i == 0 else np.union1d(own, rng.choice(S, t // 2, replace=False))
            b[u] = (cols.astype(np.int32), -rng.uniform(0.5, 2.0, len(cols)))
        idx = np.concatenate([own, outside, [own[0], own[0]]])
        rng.shuffle(idx)
        arows.append((idx, rng.uniform(0.5, 2.0, len(idx))))
        own_t.append(np.sort(own)[::-1])
        own_u.append(outside)
    return csr_from_rows(arows, C), csr_from_dict(b, C, C), {"own_touched": own_t, "own_untouched": own_u}


# ---- dense worker reuse ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _dense_reuse():
    """REUSE_ROWS rows of 1 to 3 A entries over 40 B rows of 1537 .. 1700 entries drawn from 2000 of C = 4096 columns: every row
    goes to the dense pass, and on 256 CUs (1024 workers) every worker takes two or three of them in turn."""
    rng = np.random.default_rng(106)
    C = 4096
    pool = rng.permutation(C)[:2000]
    us = rng.permutation(C)[:40]
    b = {}
    for u in us.tolist():
        n = int(rng.integers(K_HASH_LIMIT + 1, 1701))
        b[u] = (_subset(rng, pool, n), _wide(rng, n))
    arows = []
    for _ in range(REUSE_ROWS):
        n = int(rng.integers(1, 4))
        arows.append((rng.choice(us, n), _wide(rng, n)))
    return csr_from_rows(arows, C), csr_from_dict(b, C, C), {}


# ---- empty shapes ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _empty(kind):
    rng = np.random.default_rng(107)
    C = 50
    b = {u: (_subset(rng, C, 9), _wide(rng, 9)) for u in range(0, 40, 2)}  # the odd B rows are empty
    if kind == "no_rows":
        arows = []
    elif kind == "empty_rows":
        arows = [(np.zeros(0, np.int32), np.zeros(0))] * 5
    elif kind == "empty_b":
        b = {}
        arows = [([3, 4, 4], [1.0, -2.0, 3.0]), ([], []), ([0], [1.0])]
    else:  # rows 1 and 3 reach only empty B rows; the last row is empty
        arows = [([0, 2, 1], [1.0, 2.0, 3.0]), ([1, 3, 3, 49], [1.0, 2.0, 3.0, 4.0]), ([4], [0.0]), ([5], [7.0]), ([], [])]
    return csr_from_rows(arows, C), csr_from_dict(b, C, C), {}


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(name, family, build, k, zero_own):
    return name, SimpleNamespace(name=name, family=family, build=build, k=k, zero_own=zero_own)


_TABLE = dict([
    _case("stored_order_k100", "stored_order", _stored_order, 100, False),
    _case("stored_order_k450", "stored_order", _stored_order, 450, False),  # k > C
    _case("batch_edges_k70", "batch_edges", _batch_edges, 70, False),
    _case("table_cut_k100", "table_cut", lambda: _table_cut(4096, 201), 100, False),
    _case("table_cut_own_k1600", "table_cut", lambda: _table_cut(4096, 201), 1600, True),
    _case("table_cut_c5000_k100", "table_cut", lambda: _table_cut(5000, 202), 100, False),
    _case("table_cut_c3000_k300", "table_cut", lambda: _table_cut(3000, 203), 300, True),
    _case("probe_wrap_own_k1600", "probe_wrap", _probe_wrap, 1600, True),
    _case("probe_wrap_own_k10", "probe_wrap", _probe_wrap, 10, True),
    _case("probe_wrap_k1536", "probe_wrap", _probe_wrap, 1536, False),
] + [_case(f"select_distinct_k{k}", "select", lambda: _select(0), k, False) for k in KS + EXTRA_KS]
  + [_case(f"select_ties_k{k}", "select", lambda: _select(1), k, False) for k in KS + EXTRA_KS] + [
    _case("own_k50", "own", _own, 50, True),
    _case("own_k2000", "own", _own, 2000, True),
    _case("own_off_k50", "own", _own, 50, False),
    _case("dense_reuse_k20", "dense_reuse", _dense_reuse, 20, False),
    _case("dense_reuse_own_k70", "dense_reuse", _dense_reuse, 70, True),
    _case("empty_no_rows", "empty", lambda: _empty("no_rows"), 5, False),
    _case("empty_rows", "empty", lambda: _empty("empty_rows"), 5, True),
    _case("empty_b", "empty", lambda: _empty("empty_b"), 70, True),
    _case("empty_b_rows_reached", "empty", lambda: _empty("reached"), 300, True),
])
NAMES = list(_TABLE)
CUT_FAMILIES = ("batch_edges", "table_cut", "probe_wrap", "select", "own")  # every row of these is also run alone
# the order of the accumulator-state test: C = 4096, another B of the same C, a larger C, a smaller C, the first again
STATE_SEQUENCE = ("table_cut_k100", "own_k50", "table_cut_c5000_k100", "table_cut_c3000_k300", "table_cut_k100")


def get(name):
    """The case `name`: .A, .B, .k, .zero_own, .family, .claims.  Matrices are built once and shared: treat them as read-only."""
    c = _TABLE[name]
    A, B, claims = c.build()
    return SimpleNamespace(name=name, family=c.family, A=A, B=B, k=c.k, zero_own=c.zero_own, claims=claims)
