"""The row schedule and the long-row plans of CSRMatrix (csrc/csr_schedule.hip), checked on the host through
imp_host_csr_plan: the entry point runs the planner imp_csr_create uploads from, so no device is needed.  A wrong execution
order costs speed, never parity -- these invariants are the only thing that sees it."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

from implicit_amd.synthetic import synthetic_csr

CLASS_BORDERS = (512, 256, 128, 64, 32, 16, 0)
WHICH = {"all": 0, "chol": 1, "nm": 2}


@pytest.fixture(scope="module")
def schedule():
    import os

    from implicit_amd import _build, utils
    from implicit_amd.gpu import _hip

    if not os.path.exists(_hip.LIB_PATH):
        _build.build(verbose=False)
    return utils.csr_schedule


def auto_stripe(cols):
    return min(12288, max(4096, (cols // 24 + 1023) // 1024 * 1024))


def from_lengths(lengths, cols, seed=0):
    """Rows of the given lengths with sorted random column ids."""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(cols, n, replace=False)) for n in lengths] + [np.empty(0, np.int64)]).astype(np.int32)
    return sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(len(lengths), cols))


def check_plan(m, p, n_plan, segment, stripe):
    """Every invariant of one plan; `stripe` is the width a striped plan was cut at."""
    indptr, indices = m.indptr, m.indices
    lens = np.diff(indptr)
    rows = m.shape[0]
    # order and classes
    order = p["order"]
    assert np.array_equal(np.sort(order), np.arange(rows))
    assert np.array_equal(order, np.lexsort((np.arange(rows), -lens)))  # descending length, ascending id within a length
    want_bins = [0] + [int((lens > b).sum()) for b in CLASS_BORDERS] + [rows]
    assert p["bin_start"].tolist() == want_bins
    # row_seg and seg_row
    n_long, n_seg = p["n_long"], p["n_seg"]
    assert n_long == n_plan
    row_seg, seg_row, seg_begin, seg_end, seg_exec = (p[k] for k in ("row_seg", "seg_row", "seg_begin", "seg_end", "seg_exec"))
    assert len(row_seg) == n_long + 1 and all(len(a) == n_seg for a in (seg_row, seg_begin, seg_end, seg_exec))
    assert row_seg[0] == 0 and row_seg[n_long] == n_seg and (np.diff(row_seg) >= 0).all()
    assert np.array_equal(seg_row, np.repeat(np.arange(n_long), np.diff(row_seg)))
    # segment coverage
    seg_len = seg_end - seg_begin
    assert n_seg == 0 or (seg_len.min() >= 1 and seg_len.max() <= segment)
    for li in range(n_long):
        r, lo, hi = order[li], row_seg[li], row_seg[li + 1]
        assert hi > lo and seg_begin[lo] == indptr[r] and seg_end[hi - 1] == indptr[r + 1]
        assert np.array_equal(seg_begin[lo + 1:hi], seg_end[lo:hi - 1])
    # seg_exec and xcd_start
    xcd = p["xcd_start"]
    assert np.array_equal(np.sort(seg_exec), np.arange(n_seg))
    assert xcd[0] == 0 and xcd[8] == n_seg and (np.diff(xcd) >= 0).all()
    ids = np.arange(n_seg)
    if not p["striped"]:
        for x in range(8):
            assert np.array_equal(seg_exec[xcd[x]:xcd[x + 1]], ids[(ids // 4) % 8 == x])
        return
    first, last = indices[seg_begin] // stripe, indices[seg_end - 1] // stripe
    for s in range(n_seg):
        cols_of = indices[seg_begin[s]:seg_end[s]] // stripe
        assert cols_of.min() == cols_of.max() == first[s] == last[s]
    seg_stripe = first
    exec_stripe = seg_stripe[seg_exec]
    slot = np.searchsorted(xcd[1:], np.arange(n_seg), side="right")  # XCD slice of every position of seg_exec
    weight = {}
    for st in np.unique(seg_stripe):
        at = np.flatnonzero(exec_stripe == st)
        assert np.array_equal(at, np.arange(at[0], at[0] + len(at)))  # contiguous
        assert (np.diff(seg_exec[at]) > 0).all()  # ascending segment id
        assert slot[at[0]] == slot[at[-1]]  # one XCD
        weight[st] = int((seg_len[seg_stripe == st] + 16).sum())
    load = [int((seg_len[seg_exec[xcd[x]:xcd[x + 1]]] + 16).sum()) for x in range(8)]
    assert max(load) - min(load) <= max(weight.values())  # greedy: the heaviest XCD was the lightest before its last stripe


def check_all(schedule, m, segment=512, stripe=-1, nm_segment=0, num_cus=256):
    """The three plans of one matrix; returns them by name."""
    lens = np.diff(m.indptr)
    width = stripe if stripe >= 0 else auto_stripe(m.shape[1])
    out = {}
    for name, which in WHICH.items():
        p = out[name] = schedule(m, which, segment=segment, stripe=stripe, nm_segment=nm_segment, num_cus=num_cus)
        n_plan = int((lens > (1024 if name == "chol" else 512)).sum())
        seg = {"all": segment, "chol": 1024, "nm": p["nm_segment"]}[name]
        assert name == "all" or not p["striped"]
        check_plan(m, p, n_plan, seg, width)
        assert p["n_chol_long"] == int((lens > 1024).sum())
    return out


def test_class_borders(schedule):
    lengths = np.repeat([0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2049], 2)
    np.random.default_rng(1).shuffle(lengths)
    m = from_lengths(lengths, 2049)
    plans = check_all(schedule, m, stripe=0)
    assert not plans["all"]["striped"]
    assert plans["all"]["bin_start"].tolist() == [0, 8, 12, 16, 20, 24, 28, 32, 34]
    assert plans["all"]["n_long"] == 8 and plans["chol"]["n_long"] == 4


@pytest.fixture(scope="module")
def striped_matrix():
    users, items = 200, 3000
    dense_rows = sp.random(14, items, density=0.45, format="csr", dtype=np.float32, random_state=2)
    rest = synthetic_csr(users - 14, items, 9_000, seed=4, neg_frac=0.1, empty_frac=0.05)
    C = sp.vstack([rest[:50], dense_rows, rest[50:]]).tocsr().astype(np.float32)
    C.sort_indices()
    lens = np.diff(C.indptr)
    assert lens[lens > 512].sum() >= 4 * items and lens[lens > 512].sum() >= 32 * 12 * 14
    return C


@pytest.mark.parametrize("stripe", [256, 1024, -1])
def test_striped_plan(schedule, striped_matrix, stripe):
    plans = check_all(schedule, striped_matrix, stripe=stripe)
    assert plans["all"]["striped"]


def test_stripe_zero_and_unsorted_row_are_plain(schedule, striped_matrix):
    assert not check_all(schedule, striped_matrix, stripe=0)["all"]["striped"]
    U = striped_matrix.copy()
    r = int(np.argmax(np.diff(U.indptr)))
    lo, hi = U.indptr[r], U.indptr[r + 1]
    U.indices[lo:hi] = U.indices[lo:hi][::-1].copy()
    for stripe in (256, -1):
        assert not check_all(schedule, U, stripe=stripe)["all"]["striped"]


def test_stripes_need_32_nonzeros_per_row(schedule):
    m = from_lengths([1100] * 16, 4096, seed=3)
    assert 17_600 >= 4 * 4096 and 17_600 < 32 * 128 * 16  # re-use rule holds, the per-stripe rule does not
    assert not check_all(schedule, m, stripe=32)["all"]["striped"]
    assert check_all(schedule, m, stripe=1024)["all"]["striped"]


def test_nm_plan(schedule):
    lengths = np.array([513, 600, 64 * 9, 64 * 9 + 1, 5000])
    np.random.default_rng(5).shuffle(lengths)
    m = from_lengths(lengths, 5000, seed=7)
    nm = check_all(schedule, m, nm_segment=64)["nm"]
    assert not nm["striped"] and nm["nm_segment"] == 64
    assert nm["nm_multi_rows"] == int((lengths > 64).sum()) == 5
    assert nm["nm_multi_segs"] == int(sum(-(-n // 64) for n in lengths))
    assert nm["row_seg"][nm["nm_multi_rows"]] == nm["nm_multi_segs"] == nm["n_seg"]
    # a segment some long rows fit into: only the longer ones are cut, and they come first
    nm = check_all(schedule, m, nm_segment=600)["nm"]
    assert nm["nm_multi_rows"] == 1 and nm["nm_multi_segs"] == 9 and nm["row_seg"][1] == 9 and nm["n_seg"] == 9 + 4
    assert check_all(schedule, m, nm_segment=0, num_cus=256)["nm"]["nm_segment"] == 2048


def test_chol_plan(schedule):
    m = from_lengths([1024, 3000, 1025], 3000, seed=9)
    chol = check_all(schedule, m, stripe=0)["chol"]
    assert not chol["striped"] and chol["n_chol_long"] == 2 and chol["n_long"] == 2
    assert (chol["seg_end"] - chol["seg_begin"]).tolist() == [1024, 1024, 952, 1024, 1]


@pytest.mark.parametrize("lengths,cols", [([], 10), ([0] * 5, 10), ([0, 512, 3, 17], 600)], ids=["no-rows", "all-empty", "no-long-row"])
def test_degenerate(schedule, lengths, cols):
    m = from_lengths(np.array(lengths, dtype=np.int64), cols)
    for p in check_all(schedule, m).values():
        assert p["n_long"] == 0 and p["n_seg"] == 0 and not p["striped"] and not p["xcd_start"].any()


@pytest.mark.parametrize("indptr,indices,message", [
    ([0, 3, 2, 4], [0, 1, 2, 3], "indptr must be non-decreasing for CSRMatrix (row 1)"),
    ([0, 2, 4], [0, 1, -1, 3], "column index out of range for CSRMatrix (-1 not in [0, 5))"),
    ([0, 2, 4], [0, 1, 5, 3], "column index out of range for CSRMatrix (5 not in [0, 5))"),
], ids=["decreasing-indptr", "negative-column", "column-past-the-end"])
def test_validation(schedule, indptr, indices, message):
    m = types.SimpleNamespace(shape=(len(indptr) - 1, 5), indptr=np.array(indptr, np.int32), indices=np.array(indices, np.int32))
    with pytest.raises(ValueError) as e:
        schedule(m)
    assert str(e.value) == message


def test_segment_capacity_is_checked(schedule):
    from implicit_amd.gpu import _hip

    m = from_lengths([600, 700], 1000)
    indptr, indices = m.indptr.astype(np.int32), m.indices.astype(np.int32)
    small = [np.full(n, -7, np.int32) for n in (2, 9, 3, 2, 2, 2, 2, 9, 8)]  # room for 2 of the 4 segments
    order, bin_start, row_seg, seg_row, seg_begin, seg_end, seg_exec, xcd, info = (a.ctypes.data for a in small)
    status = _hip.lib().imp_host_csr_plan(2, 1000, indptr.ctypes.data, indices.ctypes.data, 512, 0, 0, 256, 0, order, bin_start, row_seg,
                                          2, seg_row, seg_begin, seg_end, seg_exec, xcd, info)
    assert status == _hip.IMP_INVALID_ARGUMENT
    assert all((a == -7).all() for a in small)  # nothing was written
