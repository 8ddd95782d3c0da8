"""The inputs of tests/test_gpu_call_history.py (tests/history_cases.py) are what they claim to be; no GPU is touched.

1. Every `bigger` predecessor has more rows and more nonzeros (or elements) than its probe.
2. Every matrix puts rows into the schedule classes its probe names, under the schedule CSRMatrix builds (imp_host_csr_plan).
3. Every `refused` predecessor fails in its restatement for the stated reason: the argument kind by the shapes that are handed
   over, the pivot kind by the float64 factorisation of the case module it was taken from.
4. Every probe's reference answer exists and is finite.
5. The sequences' class counts sit on both sides of the static-ticket cut, computed with imp_host_chain_tickets /
   imp_host_wide_tickets for 256 CUs."""
import numpy as np
import pytest

import cholesky_cases as cc
import explain_cases as xc
import explain_reference as xref
import history_cases as h
import subspace_cases as sc

NAMES = list(h.PROBES)


@pytest.fixture(scope="module")
def built():
    import os

    from implicit_amd import _build
    from implicit_amd.gpu import _hip

    if not os.path.exists(_hip.LIB_PATH):
        _build.build(verbose=False)


def test_the_table_names_what_exists():
    for p in h.PROBES.values():
        assert p.exact and p.why, p.name  # no probe here rides a floating-point atomic whose order can show
        assert p.before[0] == "quiet" and "released" in p.before and "bigger" in p.before
        assert set(h.POOL_PATTERNS) <= set(p.before)  # each pattern a cell of its own: a second fill would overwrite the first
        assert "refused_args_operands" in p.extra
        for pred in p.before:
            if pred.startswith("cross:"):
                assert pred[6:] in h.PROBES and pred[6:] != p.name, (p.name, pred)
            else:
                assert pred in h.PREDECESSORS, (p.name, pred)
                assert pred in ("quiet", "released", "released_pool_nan", "sequence") + tuple(h.POOL_PATTERNS) or pred in p.extra, (p.name, pred)
            if pred.startswith("refused"):
                assert p.extra.get(pred + "_reason") or pred == "refused_pivot", (p.name, pred)
    assert len(set(h.cells())) == len(h.cells())
    # one sequence per solver family
    assert sorted(p.extra["kind"] for p in h.PROBES.values() if "sequence" in p.before) == ["cg", "cg", "cholesky", "subspace"]


@pytest.mark.parametrize("name", NAMES)
def test_bigger_is_bigger(name):
    p = h.PROBES[name]
    (rows, nnz), (big_rows, big_nnz) = p.size(), p.bigger_size()
    print(f"{name}: {rows} rows / {nnz} against {big_rows} / {big_nnz}")
    assert big_rows > rows and big_nnz > nnz


@pytest.mark.parametrize("name", [n for n in NAMES if h.PROBES[n].matrix is not None])
def test_matrix_reaches_the_classes_its_probe_names(built, name):
    p = h.PROBES[name]
    counts = h.class_counts(p.matrix())
    print(name, counts)
    assert p.classes
    for cls in p.classes:
        assert counts[cls] > 0, (name, cls, counts)


def test_bigger_solver_matrices_keep_every_class(built):
    """Four times the rows of the routes matrix in every class, the multi-segment rows included."""
    small, big = h.class_counts(h._routes()._matrix()), h.class_counts(h._routes_bigger("cg", 128, "float32")[0])
    for cls, n in small.items():
        assert big[cls] == 4 * n, (cls, n, big[cls])
    small, big = h.class_counts(h.PROBES["subspace"].matrix()), h.class_counts(h._subspace_bigger_inputs()[0])
    assert all(big[cls] == 4 * n for cls, n in small.items())
    for which, counts in h.DRAWN_BIGGER.items():
        drawn = h.class_counts(h.class_matrix(counts, 31))
        assert [drawn[c] for c in ("team2", "team4", "team8", "team16")] == list(counts[:4])
        assert drawn["short32"] + drawn["short16"] == counts[4] + 1


# ---- 3. refused predecessors ------------------------------------------------------------------------------------------------------
def test_pivot_refusals_fail_in_float64_for_the_stated_rows():
    seen = set()
    for p in h.PROBES.values():
        make = p.extra.get("refused_pivot_problem")
        if make is None:
            continue
        q = make()
        if q.name in seen:
            continue
        seen.add(q.name)
        if p.extra["kind"] == "subspace":
            bad = sc.reference("failing", q.f, 16, 1, tuple(q.failing))[2]
        else:
            _, bad = cc.solve_f64(q.C, q.Y.astype(np.float32), q.gram, q.reg)
        assert bad == sorted(q.failing) and min(bad) == 4, (q.name, bad)
    assert len(seen) >= 6  # Cholesky at f = 64 (fp16 and fp32), 100, 128, 200, 260 and the subspace problem


def test_explain_refusal_is_not_positive_definite_from_its_first_row():
    Y = xc.factors(16)
    rows = xc.accuracy_matrix()[h.EXPLAIN_FAILING_USERS]
    for b in range(3):
        lo, hi = rows.indptr[b], rows.indptr[b + 1]
        A = xref.normal_matrix(Y, rows.indices[lo:hi], rows.data[lo:hi], h.EXPLAIN_FAILING_REG)
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(A)
    # and the probe's own batch is sound
    m, _ = xc.edge_matrix()
    Y = xc.factors(h.EXPLAIN_F, xc.EDGE_ITEMS)
    for b in range(m.shape[0]):
        lo, hi = m.indptr[b], m.indptr[b + 1]
        np.linalg.cholesky(xref.normal_matrix(Y, m.indices[lo:hi], m.data[lo:hi], xc.REG))


def test_spd_refusal_fails_at_its_pivot():
    A = h._spd_failing_matrix().astype(np.float64)
    n, bad = h.SPD_FAILING
    assert A.shape == (n, n) and np.array_equal(A, np.diag(np.diag(A)))  # diagonal: pivot j is A[j, j]
    assert (np.diag(A)[:bad] > 0).all() and A[bad, bad] < 0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A)


def test_argument_refusals_state_what_the_arrays_show():
    """The reason every argument refusal names, read off the arrays it hands over (the calls themselves need the device)."""
    ops = lambda p: p.extra["refused_args_operands"]()  # noqa: E731
    facts = {
        "YtY has one column more than Y": lambda p: ops(p)[1] == (ops(p)[0].shape[1] + 1,) * 2,
        "1025 factors: calculate_loss takes at most 1024": lambda p: ops(p)[1].shape[1] == ops(p)[2].shape[1] == 1025,
        # (C, X, Y, gramian): only the column count of X is off
        "X has one column more than Y": lambda p: ops(p)[1].shape[1] == ops(p)[2].shape[1] + 1 and ops(p)[1].shape[0] >= ops(p)[0].shape[0]
        and ops(p)[3].shape == (ops(p)[2].shape[1],) * 2 and ops(p)[2].shape[0] >= ops(p)[0].shape[1] and ops(p)[1].dtype == ops(p)[2].dtype,
        "block_size 33: the subspace sweep takes 1 .. 32": lambda p: ops(p)[0] == 33 and ops(p)[1] >= 1,
        # (user rows, Y, shape of weights)
        "weights is 16 x 16 for three users of 16 factors: it must have 48 rows": lambda p: ops(p)[2] == (16, 16)
        and ops(p)[2][0] != ops(p)[0].shape[0] * ops(p)[1].shape[1] == 48 and ops(p)[0].shape[1] <= ops(p)[1].shape[0],
        "a 4 x 5 matrix is not square": lambda p: ops(p)[0] != ops(p)[1],
        "the same orientation twice: not the two orientations of one matrix": lambda p: ops(p)[0] is ops(p)[1]
        or ops(p)[0].shape == ops(p)[1].shape and ops(p)[0].shape[0] != ops(p)[1].shape[1],
        "a zero on the diagonal": lambda p: ops(p).shape[0] == ops(p).shape[1] and (np.diag(ops(p)) == 0).sum() == 1
        and np.isfinite(ops(p)).all(),
        "D has one row more than A has columns": lambda p: ops(p)[1].shape[0] == ops(p)[0].shape[1] + 1,
        "W has one row more than Y has columns": lambda p: ops(p)[1].shape[0] == ops(p)[0].shape[1] + 1,
        "the queries have one column more than the items": lambda p: ops(p)[0].shape[1] + 1 == ops(p)[1].shape[1]
        if p.name.startswith("topk") else ops(p)[0].shape[1] == ops(p)[1].shape[1] + 1,
        "k = 1025: ease_topk takes 1 .. 1024": lambda p: ops(p) == 1025,
        "the queries have one column more than the index": lambda p: ops(p).shape[1] == h.ic.get(h.IVF_CASE).vectors.shape[1] + 1,
        "ids has K + 1 columns": lambda p: ops(p)[0].shape[1] == h.EVAL_K + 1,
        "B repeats a column within a row": lambda p: max(np.bincount(ops(p)[1].indices[ops(p)[1].indptr[0]:ops(p)[1].indptr[1]])) == 2,
        # (matrix, X, Y, deriv_sum_sq): everything else agrees
        "deriv_sum_sq has one column less than X": lambda p: ops(p)[3].shape == (ops(p)[1].shape[0], ops(p)[1].shape[1] - 1)
        and ops(p)[0].shape == (ops(p)[1].shape[0], ops(p)[2].shape[0]) and ops(p)[1].shape[1] == ops(p)[2].shape[1],
        # (matrix, X, Y)
        "X has one column less than Y": lambda p: ops(p)[1].shape == (ops(p)[0].shape[0], ops(p)[2].shape[1] - 1)
        and ops(p)[2].shape[0] == ops(p)[0].shape[1],
    }
    for p in h.PROBES.values():
        reason = p.extra["refused_args_reason"]
        assert reason in facts and reason in h.REFUSAL_TEXT and facts[reason](p), (p.name, reason)
    assert sorted(facts) == sorted(h.REFUSAL_TEXT)


# ---- 4. references ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reference_exists_and_is_finite(oracle, name):
    arrays = h.PROBES[name].reference(oracle)
    assert arrays
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        assert a.size > 0 and np.isfinite(a).all(), name


def test_pool_patterns_read_as_the_issue_says():
    loud, finite = (h.pool_arrays(h.POOL_PATTERNS[name], 8) for name in ("pool_nan", "pool_finite"))
    assert loud.nbytes == 256 and h.pool_arrays(h.POOL_PATTERNS["pool_nan"], 22).nbytes == 4 << 20
    assert np.isnan(loud).all() and np.isnan(loud.view(np.float16)).all() and (loud.view(np.int32) == -1).all()
    assert (loud.view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert np.isfinite(finite).all() and (finite > 1e38).all()
    assert list(h.POOL_CLASSES) == list(range(8, 23)) and h.POOL_BLOCKS >= 8


# ---- 5. sequences -------------------------------------------------------------------------------------------------------------------
def test_sequence_shapes_sit_on_both_sides_of_the_static_ticket_cut(built):
    from implicit_amd.utils import chain_tickets, wide_tickets

    num_cus = 256
    shapes = h.sequence_counts(num_cus)
    assert 10 <= len(shapes) <= 14
    chain_wg, wide_wg = num_cus * h.CHAIN_WORKGROUPS_PER_CU, num_cus * h.WIDE_WORKGROUPS_PER_CU

    def draws(counts):
        """Draws per class (team2, team4, team8, team16, short rows) of one launch from fresh counters."""
        _, d = chain_tickets(np.zeros((3, 8), np.uint32), [counts[2], counts[1], counts[0]], chain_wg, h.CHAIN_TEAMS)
        _, w = wide_tickets(np.zeros((2, 8), np.uint32), [counts[3], counts[4]], wide_wg)
        return [int(d[2].sum()), int(d[1].sum()), int(d[0].sum()), int(w[0].sum()), int(w[1].sum())]

    # the cut itself: the largest class that draws nothing holds three rows (groups) per team, the first that draws a ticket
    # INSIDE the class holds more than four
    cut = h.static_cut(num_cus)
    assert cut == (8192, 4096, 2048, 1024, 16384)  # tests/test_gpu_cg_class_chain.py, tests/test_gpu_cg_wide_chain.py
    for c in range(5):
        at = [0] * 5
        at[c] = cut[c] * 3 // 4
        assert draws(at)[c] == 0
        at[c] = cut[c]
        teams = cut[c] // 4 // (16 if c == 4 else 1)
        assert draws(at)[c] == teams  # one draw past the end per team, none inside
        at[c] = cut[c] + (16 if c == 4 else 1)
        assert draws(at)[c] == teams + 1
    seen = [set() for _ in range(5)]
    for counts in shapes:
        d = draws(counts)
        for c in range(5):
            units = -(-counts[c] // 16) if c == 4 else counts[c]
            teams = cut[c] // 4 // (16 if c == 4 else 1)
            kind = ("empty" if counts[c] == 0 else "static" if d[c] == 0 else "past-the-end" if units <= 4 * teams else "drawn")
            seen[c].add(kind)
    for c in range(5):
        assert seen[c] == {"empty", "static", "past-the-end", "drawn"}, (c, seen[c])
    # the matrices really hold those counts, and stay at the size of `drawn`
    drawn_rows = max(h._drawn_inputs(which)[0].shape[0] for which in ("chain", "wide"))
    for i, counts in enumerate(shapes):
        m = h.class_matrix(tuple(counts), 100 + i)
        got = h.class_counts(m)
        assert [got["team2"], got["team4"], got["team8"]] == list(counts[:3])
        assert got["team16"] == counts[3] and got["short32"] + got["short16"] == counts[4] + 1  # + the 5-entry row of `extra`
        assert m.shape[0] <= 2 * drawn_rows
