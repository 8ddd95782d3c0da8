"""Host-only proof of what tests/test_gpu_knn_edges.py relies on: every case of tests/knn_cases.py has the properties it claims,
the restatement knn_reference.product_topk is bit for bit a literal triple loop on them (so it can serve as the bitwise
reference), and the cases discriminate: restatements that sum in another order, fuse the multiply-add or break ties the other
way give other bits or other ids."""
from fractions import Fraction

import numpy as np
import pytest

import knn_cases as kc
import knn_reference as kr

LITERAL_PAIRS = 300_000  # cases up to this many (A entry, B entry) pairs are also run through the literal loop


def literal(A, B, k, zero_own, fma=False, start_at_v=False, ascending=False):
    """The contract as a triple loop: a dict per row, A[r]'s stored order, every sum started as 0.0 + v.
    fma: acc + b*w rounded once (exact in Fraction; float(Fraction) rounds correctly).  start_at_v: sums started at v.
    ascending: ties broken by the smaller column."""
    R = A.shape[0]
    ids = np.full((R, k), -1, dtype=np.int32)
    scores = np.full((R, k), -np.inf)
    counts = np.zeros(R, dtype=np.int32)
    ap, ai, ad = A.indptr.tolist(), A.indices.tolist(), A.data.tolist()
    bp, bi, bd = B.indptr.tolist(), B.indices.tolist(), B.data.tolist()
    for r in range(R):
        sums = {}
        for p in range(ap[r], ap[r + 1]):
            u, w = ai[p], ad[p]
            for q in range(bp[u], bp[u + 1]):
                j, b = bi[q], bd[q]
                if fma:
                    sums[j] = float(Fraction(b) * Fraction(w) + Fraction(sums.get(j, 0.0)))
                elif j in sums:
                    sums[j] = sums[j] + b * w
                else:
                    sums[j] = b * w if start_at_v else 0.0 + b * w
        if zero_own:
            for p in range(ap[r], ap[r + 1]):
                if ai[p] in sums:
                    sums[ai[p]] = 0.0
        best = sorted(sums.items(), key=lambda cs: (-cs[1], cs[0] if ascending else -cs[0]))[:k]
        counts[r] = len(best)
        ids[r, :len(best)] = [c for c, _ in best]
        scores[r, :len(best)] = [s for _, s in best]
    return ids, scores, counts


def same_bits(x, y):
    return all(np.array_equal(a, b) for a, b in ((x[0], y[0]), (x[1].view(np.int64), y[1].view(np.int64)), (x[2], y[2])))


def rows_differing(x, y):
    """Share of non-empty rows whose ids or score bits differ."""
    diff = np.any(x[0] != y[0], axis=1) | np.any(x[1].view(np.int64) != y[1].view(np.int64), axis=1)
    return diff[x[2] > 0].mean()


@pytest.fixture(scope="module")
def want():
    cache = {}

    def of(name):
        if name not in cache:
            c = kc.get(name)
            cache[name] = kr.product_topk(c.A, c.B, c.k, c.zero_own)
        return cache[name]

    return of


def test_hash_restatement():
    # knn.hip: (uint32)j * 2654435761u >> 21; spot values worked out by hand in 32-bit arithmetic
    assert kc.knn_hash(0) == 0 and kc.knn_hash(1) == (2654435761 >> 21) and kc.knn_hash(3) == ((3 * 2654435761) % 2**32) >> 21
    h = kc.knn_hash(np.arange(65536))
    assert h.min() == 0 and h.max() == kc.K_HASH_SLOTS - 1
    assert kc.dense_workers(256, 4096) == 1024 and kc.dense_workers(256, 1 << 20) == 128 and kc.dense_workers(1, 10) == 4


def test_every_case_is_wellformed():
    for name in kc.NAMES:
        c = kc.get(name)
        A, B = c.A, c.B
        assert A.shape[1] == B.shape[0] and B.shape[1] <= 65536 and c.k >= 1, name
        assert not c.zero_own or A.shape[1] == B.shape[1], name
        assert kc.row_flags(B)[1] == 0, name  # B free of in-row repeats
        assert kc.pair_count(A, B) <= 1.1e7, name
        assert np.all(np.isfinite(A.data)) and np.all(np.isfinite(B.data)), name
        if c.family in kc.CUT_FAMILIES:
            assert A.shape[0] <= kc.MAX_SOLO_ROWS, name
    for family in ("batch_edges", "table_cut", "probe_wrap", "select", "own", "stored_order", "empty"):
        assert any(kc.get(n).family == family and kc.pair_count(kc.get(n).A, kc.get(n).B) <= LITERAL_PAIRS for n in kc.NAMES), family
    assert kc.STATE_SEQUENCE[0] == kc.STATE_SEQUENCE[-1]
    cols = [kc.get(n).B.shape[1] for n in kc.STATE_SEQUENCE]
    assert cols[0] == cols[1] == 4096 and cols[2] > cols[1] and cols[3] < cols[1]
    assert kc.get(kc.STATE_SEQUENCE[0]).B is not kc.get(kc.STATE_SEQUENCE[1]).B
    for n in kc.STATE_SEQUENCE:  # every call of the sequence reaches the dense pass
        c = kc.get(n)
        assert kc.touched_counts(c.A, c.B).max() > kc.K_HASH_LIMIT, n


def test_restatement_equals_the_literal_loop(want):
    ran = set()
    for name in kc.NAMES:
        c = kc.get(name)
        if kc.pair_count(c.A, c.B) > LITERAL_PAIRS:
            continue
        assert same_bits(want(name), literal(c.A, c.B, c.k, c.zero_own)), name
        ran.add(c.family)
    assert ran >= {"stored_order", "batch_edges", "table_cut", "probe_wrap", "select", "own", "empty"}


def test_restatement_equals_the_literal_loop_on_a_slice_of_dense_reuse(want):
    c = kc.get("dense_reuse_own_k70")
    rows = slice(0, 60)
    sub = kc.csr_from_rows([(kc.one_row(c.A, r).indices, kc.one_row(c.A, r).data) for r in range(60)], c.A.shape[1])
    w = want(c.name)
    assert same_bits((w[0][rows], w[1][rows], w[2][rows]), literal(sub, c.B, c.k, c.zero_own))
    assert kc.touched_counts(sub, c.B).min() > kc.K_HASH_LIMIT


def test_stored_order_claims():
    c = kc.get("stored_order_k100")
    A, B = c.A, c.B
    lens = np.diff(A.indptr)
    assert A.shape[0] == 40 and lens.min() == 0 and lens.max() == 130 and {1, 64, 65} <= set(lens.tolist())
    unsorted, dup = kc.row_flags(A)
    assert unsorted >= 30 and dup >= 25
    assert np.any(A.data == 0.0) and np.any(B.data == 0.0) and np.any(A.data < 0) and np.any(B.data < 0)
    for m in (A, B):
        mag = np.abs(m.data[m.data != 0])
        assert mag.max() / mag.min() > 1e15
    assert B.shape == (300, 400) and 0.18 < B.nnz / (300 * 400) < 0.22
    assert kc.touched_counts(A, B).max() <= kc.K_HASH_LIMIT  # the hash pass alone
    assert kc.get("stored_order_k450").k > B.shape[1]
    r = c.claims["neg_zero_row"]  # a negative weight on stored zeros: every term is -0.0
    lo = A.indptr[r]
    assert lens[r] == 1 and A.data[lo] < 0 and np.sum(B.data[B.indptr[A.indices[lo]]:B.indptr[A.indices[lo] + 1]] == 0.0) >= 2


def test_batch_edge_claims():
    c = kc.get("batch_edges_k70")
    la = np.diff(c.A.indptr)
    assert set(la.tolist()) == set(kc.BATCH_LENS) == set(np.diff(c.B.indptr).tolist())
    seen = set()
    for r, (a_len, b_len) in enumerate(c.claims["shape"]):
        us = c.A.indices[c.A.indptr[r]:c.A.indptr[r + 1]]
        assert la[r] == a_len and np.all(np.diff(c.B.indptr)[us] == b_len)
        seen.add((a_len, b_len))
    assert seen == {(a, b) for a in kc.BATCH_LENS for b in kc.BATCH_LENS}  # crossed in one matrix pair


@pytest.mark.parametrize("name", ["table_cut_k100", "table_cut_c5000_k100", "table_cut_c3000_k300"])
def test_table_cut_claims(name):
    c = kc.get(name)
    A, B = c.A, c.B
    touched = kc.touched_counts(A, B)
    blen = np.diff(B.indptr)
    seen = set()
    for r, (kind, T) in enumerate(c.claims["kinds"]):
        us = A.indices[A.indptr[r]:A.indptr[r + 1]]
        if kind in ("single", "overlap", "late"):
            assert touched[r] == T, (r, kind)
            seen.add((kind, T))
        if kind == "single":
            assert len(us) == 1 and blen[us[0]] == T
        elif kind == "overlap":
            cover = np.bincount(np.concatenate([B.indices[B.indptr[u]:B.indptr[u + 1]] for u in us]), minlength=B.shape[1])
            assert len(us) == 30 and np.mean(cover[cover > 0] >= 2) > 0.99 and blen[us].max() < 512
            assert kc.row_flags(kc.one_row(A, r)) == (1, 1)
        elif kind == "late":
            # the first A entry alone reaches all T columns; hundreds of entries follow
            assert blen[us[0]] == T and len(us) == 301 and blen[us[1:]].max() <= 40
        elif kind == "light":
            assert 0 < touched[r] < 300
        else:
            assert len(us) == 0
    assert seen == {(kind, T) for kind in ("single", "overlap", "late") for T in kc.CUT_TOUCHED}
    assert set(kc.CUT_TOUCHED) == {kc.K_HASH_LIMIT - 1, kc.K_HASH_LIMIT, kc.K_HASH_LIMIT + 1, kc.K_HASH_LIMIT + 64}
    # rows that stay in the table and rows that leave it, in one call
    assert np.sum(touched > kc.K_HASH_LIMIT) == 6 and np.sum((touched > 0) & (touched <= kc.K_HASH_LIMIT)) == 10


def test_probe_wrap_claims():
    c = kc.get("probe_wrap_own_k1600")
    A, B = c.A, c.B
    first, late = c.claims["cluster"]
    own = c.claims["own"]
    assert B.shape[1] == 65536 and c.zero_own
    assert kc.touched_counts(A, B)[0] == kc.K_HASH_LIMIT == len(first) + len(late)
    assert kc.knn_hash(np.concatenate([first, late])).min() >= kc.K_HASH_SLOTS - 384
    # row 0's stored order: the 1500 columns first.  They fill every slot from 1664 to 2047 whatever the order inside a step.
    us = A.indices[A.indptr[0]:A.indptr[1]]
    assert np.array_equal(np.sort(B.indices[B.indptr[us[0]]:B.indptr[us[0] + 1]]), np.sort(first))
    slots_first = kc.probe_slots(first)
    assert set(range(kc.K_HASH_SLOTS - 384, kc.K_HASH_SLOTS)) <= set(slots_first.tolist()) and slots_first.min() == 0
    # so every later column, the own columns among them, lies beyond the wrap: probing from its hash passes 2047 -> 0
    assert set(own) <= set(late.tolist()) and set(own) == set(us.tolist())
    slots = kc.probe_slots(np.concatenate([first, late]))[len(first):]
    assert slots.max() < kc.K_HASH_SLOTS - 384 and np.all(slots < kc.knn_hash(late))
    # row 1: one slot's whole chain, through two B rows of opposite order; the chain crosses the end of the table too
    chain = c.claims["chain"]
    assert 28 <= len(chain) <= 40 and np.all(kc.knn_hash(chain) == c.claims["slot"])
    assert c.claims["slot"] + len(chain) > kc.K_HASH_SLOTS
    cs = kc.probe_slots(chain)
    assert cs.max() == kc.K_HASH_SLOTS - 1 and cs.min() == 0
    vs = A.indices[A.indptr[1]:A.indptr[2]]
    assert set(vs.tolist()) <= set(chain.tolist()) and kc.touched_counts(A, B)[1] == len(chain)
    assert np.any(np.diff(B.indices[B.indptr[vs[1]]:B.indptr[vs[1] + 1]]) < 0)  # B's stored order is free as well


def test_selection_claims(want):
    assert {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025} == set(kc.KS)
    for ties in (0, 1):
        prefix = "select_ties_k" if ties else "select_distinct_k"
        c = kc.get(prefix + "64")
        touched = kc.touched_counts(c.A, c.B)
        assert touched.tolist() == c.claims["touched"]
        for k in kc.KS:
            assert {k - 1, k, k + 1, 1800, 3000} - {0} <= set(touched.tolist())
        for k in (1537,):
            assert {k - 1, k, k + 1} <= set(touched.tolist())
        assert max(kc.EXTRA_KS) > c.B.shape[1]
        assert np.sum(touched > kc.K_HASH_LIMIT) == 4  # both passes
        ids, scores, counts = kr.product_topk(c.A, c.B, 3000, False)
        for r, t in enumerate(touched):
            s = scores[r, :t]
            if not ties:
                assert len(np.unique(s)) == t
                continue
            # runs of equal scores over positions [0, 40), [40, 300), [300, t): across 64, 256 and 512
            n3, n2 = min(t, kc.TIE_LEVELS[0]), min(t, kc.TIE_LEVELS[1])
            assert np.all(s[:n3] == 3.0) and np.all(s[n3:n2] == 2.0) and np.all(s[n2:] == 1.0)
            for lo, hi in ((0, n3), (n3, n2), (n2, t)):
                assert np.all(np.diff(ids[r, lo:hi]) < 0)  # column descending alone
        assert kc.TIE_LEVELS[0] < 64 < 256 < kc.TIE_LEVELS[1] < 512
    # a restatement that breaks ties by the smaller column gives other ids at every k
    for k in kc.KS + kc.EXTRA_KS:
        c = kc.get(f"select_ties_k{k}")
        got = literal(c.A, c.B, k, False, ascending=True)
        w = want(c.name)
        assert np.array_equal(got[2], w[2]) and np.array_equal(got[1], w[1])
        assert rows_differing(got, w) > 0.9, k


def test_own_claims(want):
    c = kc.get("own_k50")
    A, B = c.A, c.B
    touched = kc.touched_counts(A, B)
    assert touched.tolist() == list(kc.OWN_TOUCHED) and touched[0] <= kc.K_HASH_LIMIT < touched[1]  # both passes
    ids, scores, counts = want("own_k50")
    off = want("own_off_k50")
    for r in range(2):
        own_t, own_u = c.claims["own_touched"][r], c.claims["own_untouched"][r]
        us = A.indices[A.indptr[r]:A.indptr[r + 1]]
        assert set(own_t.tolist()) | set(own_u.tolist()) == set(us.tolist()) and len(us) > len(set(us.tolist()))  # repeats
        # the zeroed columns lead, by column descending; every other score is negative
        assert np.array_equal(ids[r, :8], own_t) and np.all(scores[r, :8] == 0.0) and np.all(scores[r, 8:counts[r]] < 0)
        assert np.all(off[1][r, :off[2][r]] < 0)
    full = want("own_k2000")
    for r in range(2):  # liked but never touched: no candidate
        assert full[2][r] == touched[r] and not set(c.claims["own_untouched"][r].tolist()) & set(full[0][r, :full[2][r]].tolist())


def test_dense_reuse_and_empty_claims(want):
    c = kc.get("dense_reuse_k20")
    lens = np.diff(c.A.indptr)
    blen = np.diff(c.B.indptr)
    assert c.A.shape[0] == kc.REUSE_ROWS > 2 * kc.dense_workers(256, c.B.shape[1])
    assert lens.min() == 1 and lens.max() == 3 and np.sum(blen > 0) == 40
    assert blen[blen > 0].min() > kc.K_HASH_LIMIT and blen.max() <= 1700  # every row overflows in its first A entry
    assert len(np.unique(c.B.indices)) <= 2000  # heavy overlap
    assert kc.get("empty_no_rows").A.shape[0] == 0 and want("empty_no_rows")[0].shape == (0, 5)
    e = kc.get("empty_rows")
    assert e.A.shape[0] == 5 and e.A.nnz == 0 and want("empty_rows")[2].tolist() == [0] * 5
    e = kc.get("empty_b")
    assert e.B.nnz == 0 and e.A.nnz > 0 and want("empty_b")[2].tolist() == [0] * 3
    e = kc.get("empty_b_rows_reached")
    assert want(e.name)[2].tolist() == kc.touched_counts(e.A, e.B).tolist() == [17, 0, 9, 0, 0] and e.A.nnz == 9
    assert np.all(want(e.name)[0][1] == -1) and np.all(np.isneginf(want(e.name)[1][1]))
    assert np.all(want(e.name)[1][2, :9] == 0.0)  # a zero weight still touches


def _overlap_rows(c):
    rows = [r for r, (kind, _) in enumerate(c.claims["kinds"]) if kind == "overlap"]
    return kc.csr_from_rows([(kc.one_row(c.A, r).indices, kc.one_row(c.A, r).data) for r in rows], c.A.shape[1])


def test_the_cases_discriminate_on_summation():
    """Share of non-empty rows whose bits change under each mutant of the restatement, as measured by this test:
      (a) A canonicalised (sorted, duplicates summed): stored_order 37 of 39 rows (0.949), overlapping table-cut rows 4 of 4;
      (b) every acc + b*w one correctly rounded FMA:      stored_order 37 of 39 rows (0.949), overlapping table-cut rows 4 of 4;
      (c) sums started at v instead of 0.0 + v: differs only where every term of a sum is -0.0 (0.0 + -0.0 is +0.0).
          stored_order has one such row by construction (a negative weight on stored zeros); the table-cut rows have none
          and are bitwise identical under (c), so nothing is claimed for them.
    Half of each measured share is asserted."""
    so = kc.get("stored_order_k100")
    tc = kc.get("table_cut_k100")
    A_tc = _overlap_rows(tc)
    for A, B, k, floor_a, floor_b in ((so.A, so.B, so.k, 0.47, 0.47), (A_tc, tc.B, tc.k, 0.5, 0.5)):
        base = kr.product_topk(A, B, k)
        canon = A.copy()
        canon.sum_duplicates()
        a = rows_differing(kr.product_topk(canon, B, k), base)
        b = rows_differing(literal(A, B, k, False, fma=True), base)
        print(f"rows differing: canonical A {a:.3f}, fma {b:.3f}")
        assert a >= floor_a and b >= floor_b
    base = kr.product_topk(so.A, so.B, so.k)
    v = literal(so.A, so.B, so.k, False, start_at_v=True)
    r = so.claims["neg_zero_row"]
    assert np.any(v[1][r].view(np.int64) != base[1][r].view(np.int64)) and np.array_equal(v[1], base[1])  # -0.0 against +0.0
    assert same_bits(literal(A_tc, tc.B, tc.k, False, start_at_v=True), kr.product_topk(A_tc, tc.B, tc.k))
