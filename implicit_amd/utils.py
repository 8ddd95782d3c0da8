"""Small host-side helpers shared by the model layer (semantics of implicit/utils.py)."""
import time
import warnings

import numpy as np
import scipy.sparse


class ParameterWarning(Warning):
    """Raised (as a warning) when an input had to be converted (implicit/utils.py:155-156)."""


def check_csr(user_items):
    """Accepts only CSR; anything else is converted with a ParameterWarning (implicit/utils.py:159-169)."""
    if isinstance(user_items, scipy.sparse.csr_matrix):
        return user_items
    kind = type(user_items).__name__
    t0 = time.time()
    converted = user_items.tocsr()
    warnings.warn(
        f"Method expects CSR input, and was passed {kind} instead. "
        f"Converting to CSR took {time.time() - t0} seconds",
        ParameterWarning,
    )
    return converted


def check_random_state(random_state):
    """numpy Generator from None / int / RandomState / Generator (implicit/utils.py:65-83; the
    reference's RandomState branch calls a non-existent `rand_int` -- here it works)."""
    if isinstance(random_state, np.random.RandomState):
        return np.random.default_rng(random_state.randint(2**31))
    return np.random.default_rng(random_state)


def nonzeros(m, row):
    """(index, value) pairs of one CSR row (implicit/utils.py:9-12)."""
    for k in range(m.indptr[row], m.indptr[row + 1]):
        yield m.indices[k], m.data[k]


def _id_array(a, what):
    a = np.asarray(a)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{what} must hold integer item ids, got dtype {a.dtype}")
    return a if a.dtype.kind in "iu" else a.astype(np.int32)  # (an empty float array: what np.asarray makes of [])


def candidate_form(selected_items):
    """How rank_items / score_items read `selected_items`: "shared" (1-d ids: one list for every user), "padded" (a 2-d
    ndarray, one row per user, entries < 0 are padding) or "ragged" (a sequence of 1-d arrays, one per user)."""
    if isinstance(selected_items, np.ndarray) and selected_items.dtype != object:
        if selected_items.ndim == 1:
            return "shared"
        if selected_items.ndim == 2:
            return "padded"
        raise ValueError(f"selected_items must be 1- or 2-dimensional, got {selected_items.ndim} dimensions")
    if np.isscalar(selected_items) or not hasattr(selected_items, "__len__"):
        raise ValueError("selected_items must be an array of item ids or a sequence of such arrays")
    if all(np.isscalar(x) for x in selected_items):
        return "shared"
    return "ragged"


def candidate_lists(selected_items, batch):
    """The candidate lists of `batch` users as CSR: (offsets [batch + 1] int64, candidates int32), user r owning
    candidates[offsets[r]:offsets[r + 1]] in the order given.  Pure host code."""
    form = candidate_form(selected_items)
    if form == "shared":
        ids = _id_array(selected_items, "selected_items")
        lengths = np.full(batch, len(ids), dtype=np.int64)
        flat = np.tile(ids, batch)
    elif form == "padded":
        ids = _id_array(selected_items, "selected_items")
        if ids.shape[0] != batch:
            raise ValueError("selected_items must contain 1 row for every user in userids")
        keep = ids >= 0
        lengths = keep.sum(axis=1).astype(np.int64)
        flat = ids.reshape(-1) if keep.all() else ids[keep]  # row-major: every row's entries in their own order
    else:
        if len(selected_items) != batch:
            raise ValueError("selected_items must contain 1 list for every user in userids")
        rows = [_id_array(x, "every list of selected_items") for x in selected_items]
        if any(x.ndim != 1 for x in rows):
            raise ValueError("every list of selected_items must be 1-dimensional")
        lengths = np.array([len(x) for x in rows], dtype=np.int64)
        flat = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32)
    if flat.size and flat.dtype != np.int32 and (flat.max() > np.iinfo(np.int32).max or flat.min() < np.iinfo(np.int32).min):
        raise IndexError("Some itemids are not in the model")
    offsets = np.zeros(batch + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return offsets, np.ascontiguousarray(flat, dtype=np.int32)


def random_factors(rng, rows, cols, scale=0.01, workers=None):
    """`rng.random((rows, cols), dtype=float32) * scale` -- the CPU path's initial factors (implicit/cpu/als.py:144-147) --
    with the SAME bits and the same generator state afterwards, drawn by a pool of threads: PCG64 can jump ahead, one 64-bit
    step feeds two float32 draws, so every thread fills its slice from a copy of the generator advanced to the slice's start
    (83 M draws at configs[2]: 0.13 s on one core, the largest item of fit()'s set-up).  Any other bit generator, an odd
    element count or a half-consumed 64-bit word takes the plain call."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    n = rows * cols
    bg = rng.bit_generator
    state = bg.state if type(bg).__name__ == "PCG64" else None
    if state is None or n % 2 or n < (1 << 20) or state.get("has_uint32", 0):
        return rng.random((rows, cols), dtype=np.float32) * scale
    if workers is None:
        workers = max(1, min(16, (os.cpu_count() or 2) // 2))
    out = np.empty(n, dtype=np.float32)
    chunk = ((n // workers + 1) // 2) * 2
    scale32 = np.float32(scale)

    def fill(start):
        stop = min(n, start + chunk)
        g = np.random.PCG64()
        g.state = state
        g.advance(start // 2)
        np.random.Generator(g).random(stop - start, dtype=np.float32, out=out[start:stop])
        out[start:stop] *= scale32

    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(fill, range(0, n, chunk)))
    bg.advance(n // 2)
    return out.reshape(rows, cols)


def transpose_csr(m, threads=0):
    """`m.T.tocsr()` for a canonical float32 CSR with 32-bit offsets, by the library's threaded counting transpose
    (imp_host_csr_transpose: host code, no device involved) -- scipy's single-threaded conversion is a third of fit()'s
    set-up at configs[2].  Anything else (64-bit offsets, other dtypes, unsorted or duplicated entries, library not
    built) goes through scipy."""
    ok = (isinstance(m, scipy.sparse.csr_matrix) and m.dtype == np.float32 and m.indptr.dtype == np.int32
          and m.indices.dtype == np.int32 and m.nnz < 2**31 - 1 and m.has_canonical_format)
    if ok:
        try:
            from .gpu._hip import check, lib

            fn = lib().imp_host_csr_transpose
        except (ImportError, OSError, AttributeError):
            ok = False
    if not ok:
        return m.T.tocsr()
    rows, cols = m.shape
    indptr, indices, data = (np.ascontiguousarray(a) for a in (m.indptr, m.indices, m.data))
    t_indptr = np.empty(cols + 1, dtype=np.int32)
    t_indices = np.empty(m.nnz, dtype=np.int32)
    t_data = np.empty(m.nnz, dtype=np.float32)
    check(fn(rows, cols, m.nnz, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, t_indptr.ctypes.data,
             t_indices.ctypes.data, t_data.ctypes.data, int(threads)))
    out = scipy.sparse.csr_matrix((t_data, t_indices, t_indptr), shape=(cols, rows), copy=False)
    out.has_sorted_indices = True
    out.has_canonical_format = True
    return out


def csr_schedule(m, which=0, segment=512, stripe=-1, nm_segment=0, num_cus=256):
    """The row schedule and one long-row plan `CSRMatrix(m)` would build, computed on the host (imp_host_csr_plan: the
    planner of imp_csr_create with its knobs as arguments, no device involved).  `which`: 0 the streamed plan, 1 the
    Cholesky plan, 2 the normal-matrix work list; stripe < 0 and nm_segment 0 select the automatic values.  Returns a dict
    of numpy arrays (order, bin_start, row_seg, seg_row, seg_begin, seg_end, seg_exec, xcd_start) and the scalars n_long,
    n_seg, striped, n_chol_long, nm_segment, nm_multi_rows, nm_multi_segs."""
    from .gpu._hip import check, lib

    rows, cols = m.shape
    indptr = np.ascontiguousarray(m.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(m.indices, dtype=np.int32)
    capacity = max(int(indptr[-1]), 0) if rows else 0
    out = {"order": np.empty(rows, np.int32), "bin_start": np.empty(9, np.int32), "row_seg": np.empty(rows + 1, np.int32)}
    segs = {k: np.empty(capacity, np.int32) for k in ("seg_row", "seg_begin", "seg_end", "seg_exec")}
    out["xcd_start"] = np.empty(9, np.int32)
    info = np.zeros(8, np.int32)
    check(lib().imp_host_csr_plan(rows, cols, indptr.ctypes.data, indices.ctypes.data, segment, stripe, nm_segment, num_cus, which,
                                  out["order"].ctypes.data, out["bin_start"].ctypes.data, out["row_seg"].ctypes.data, capacity,
                                  *(segs[k].ctypes.data for k in ("seg_row", "seg_begin", "seg_end", "seg_exec")),
                                  out["xcd_start"].ctypes.data, info.ctypes.data))
    names = ("n_long", "n_seg", "striped", "n_chol_long", "nm_segment", "nm_multi_rows", "nm_multi_segs")
    out.update({k: int(v) for k, v in zip(names, info)})
    out["striped"] = bool(out["striped"])
    out["row_seg"] = out["row_seg"][:out["n_long"] + 1]
    out.update({k: v[:out["n_seg"]] for k, v in segs.items()})
    return out


def chain_tickets(state, counts, workgroups, teams_per_workgroup=(1, 2, 4)):
    """One launch of the ticket bookkeeping of the chained mid-row CG classes (imp_host_chain_tickets, host code): `state`, a
    uint32 array [3, 8] of the counter values of the classes' queues, is advanced in place; returns (base, draws) of the
    launch, [3, 8] each, for the row counts per class, the workgroups of the grid and the teams of each class in one."""
    from .gpu._hip import check, lib

    assert state.dtype == np.uint32 and state.shape == (3, 8) and state.flags.c_contiguous
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    teams = np.ascontiguousarray(teams_per_workgroup, dtype=np.int32)
    assert counts.shape == teams.shape == (3,)
    base, draws = np.empty((3, 8), np.uint32), np.empty((3, 8), np.uint32)
    check(lib().imp_host_chain_tickets(state.ctypes.data, counts.ctypes.data, int(workgroups), teams.ctypes.data, base.ctypes.data,
                                       draws.ctypes.data))
    return base, draws


def wide_tickets(state, rows, workgroups):
    """The same for the chained 1024-thread CG classes (imp_host_wide_tickets): `state` is uint32 [2, 8]; `rows` holds the rows
    of (256,512] and the short rows, which are ticketed in groups of 16.  Returns (base, draws), [2, 8] each."""
    from .gpu._hip import check, lib

    assert state.dtype == np.uint32 and state.shape == (2, 8) and state.flags.c_contiguous
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    assert rows.shape == (2,)
    base, draws = np.empty((2, 8), np.uint32), np.empty((2, 8), np.uint32)
    check(lib().imp_host_wide_tickets(state.ctypes.data, rows.ctypes.data, int(workgroups), base.ctypes.data, draws.ctypes.data))
    return base, draws


def long_tail_route(chain_counts, wide_counts, n_multi, capacity, chained):
    """Who runs the tail of the long-row path of a CG half sweep (imp_host_long_tail_route, host code) for the row counts of the
    three chained 512-thread classes and the two 1024-thread ones, `n_multi` long rows of more than one segment, a fix list of
    `capacity` entries, on the chained route or not.  Returns (finish, fixup): finish 0 nothing, 1 stand-alone, 2 the team
    chain; fixup 0 nothing, 1 stand-alone ahead of the classes, 2 stand-alone behind the team chain, 3 the wide chain."""
    from .gpu._hip import check, lib

    chain = np.ascontiguousarray(chain_counts, dtype=np.int32)
    wide = np.ascontiguousarray(wide_counts, dtype=np.int32)
    assert chain.shape == (3,) and wide.shape == (2,)
    out = np.zeros(2, np.int32)
    check(lib().imp_host_long_tail_route(chain.ctypes.data, wide.ctypes.data, int(n_multi), int(capacity), int(bool(chained)),
                                         out.ctypes.data))
    return int(out[0]), int(out[1])
