"""CPU-side checks of tests/sgd_cases.py: that the shape lists the SGD and ranking-metric GPU tests run at cover what they
claim -- both ends of every (G, CPL) instantiation, a conflict-free seed for every C of the two-round call, the coverage
conditions of the search-cut matrix and the share of BPR samples too close to a zero score to be counted."""
import numpy as np
import pytest

import sgd_cases as sc
import warp_reference as wref


# ---- 1. the dispatch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cases, instantiation_of, min_c", [(sc.DISPATCH_C, sc.pair_instantiation, sc.PAIR_MIN_C),
                                                            (sc.LMF_DISPATCH_C, sc.lmf_instantiation, sc.LMF_MIN_C)])
def test_dispatch_lists_hold_both_ends_of_every_instantiation(cases, instantiation_of, min_c):
    ends = sc.dispatch_ends(instantiation_of, min_c)
    assert sorted(ends) == sorted(sc.INSTANTIATIONS) and len(ends) == 12
    for inst, (lo, hi) in ends.items():
        assert lo in cases and hi in cases, inst
        assert instantiation_of(lo) == instantiation_of(hi) == inst
        assert lo == min_c or instantiation_of(lo - 1) != inst
        assert hi == sc.MAX_C or instantiation_of(hi + 1) != inst
    assert min(cases) == min_c and max(cases) == sc.MAX_C and len(set(cases)) == len(cases)


def test_dispatch_ends_are_the_ranges_of_the_launch_code():
    want = {(16, 1): (2, 16), (16, 2): (17, 32), (16, 3): (33, 48), (16, 4): (49, 64), (16, 6): (65, 96), (16, 8): (97, 128),
            (32, 6): (129, 192), (32, 8): (193, 256), (64, 6): (257, 384), (64, 8): (385, 512), (64, 12): (513, 768),
            (64, 16): (769, 1024)}
    assert sc.dispatch_ends(sc.pair_instantiation, sc.PAIR_MIN_C) == want
    want[(16, 1)] = (3, 16)
    assert sc.dispatch_ends(sc.lmf_instantiation, sc.LMF_MIN_C) == want
    # the two restatements agree wherever both entry points accept C
    assert all(sc.pair_instantiation(C) == sc.lmf_instantiation(C) for C in range(3, 1025))
    # what the dispatcher compiles for LMF (rule_reaches) is the twelve pairs the rule picks, no more
    assert {(G, CPL) for G in (16, 32, 64) for CPL in (1, 2, 3, 4, 6, 8, 12, 16) if sc.rule_reaches(G, CPL)} == set(sc.INSTANTIATIONS)
    # the values the tests ran at before are still there
    assert {2, 17, 33, 65, 101, 129, 257, 1024} <= set(sc.DISPATCH_C) and set(sc.LMF_EXISTING_C) <= set(sc.LMF_DISPATCH_C)
    # a C with one wholly masked register: cpl = 5 on CPL = 6 and cpl = 7 on CPL = 8
    assert -(-65 // 16) == 5 and sc.pair_instantiation(65) == (16, 6) and -(-97 // 16) == 7 and sc.pair_instantiation(97) == (16, 8)


def test_lane_overrides_reach_what_they_say():
    for lanes, C, inst in sc.LANE_OVERRIDES:
        assert sc.pair_instantiation(C, lanes) == inst
    reached = {inst for _, _, inst in sc.LANE_OVERRIDES[:-1]}
    # every (G, CPL) the two chains can form, less the twelve the dispatch picks by itself
    only_by_switch = {(G, CPL) for G in (16, 32, 64) for CPL in (1, 2, 3, 4, 6, 8, 12, 16)} - set(sc.INSTANTIATIONS)
    assert reached == only_by_switch and len(reached) == 12
    lanes, C, inst = sc.LANE_OVERRIDES[-1]
    assert C > 16 * lanes and inst == sc.pair_instantiation(C)  # ignored
    assert sc.pair_group(17, 48) == 16  # not a group size: ignored as well


# ---- 2. the two-round conflict-free call ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounds():
    m = sc.rounds_matrix()
    return m, wref.liked_sets(m)


def test_rounds_matrix_takes_two_rounds_the_second_half_empty(rounds):
    m, _ = rounds
    groups = sc.hogwild_in_flight(sc.ROUNDS_N, *m.shape)
    assert m.shape == (256, 20000) and groups == 16
    assert groups < sc.ROUNDS_N < 2 * groups  # the prefetch guard s + 16 < 24 holds for groups 0 .. 7 only
    assert {sc.pair_group(C) for C in sc.ROUNDS_C} == {16, 32, 64} and set(sc.ROUNDS_C) <= set(sc.DISPATCH_C)
    for G in (16, 32, 64):  # 16 groups at every G: the grid is (16 G + 255) / 256 workgroups of 256 / G groups
        assert (groups * G + 255) // 256 * (256 // G) == 16


def test_bpr_rounds_seed_exists(rounds):
    m, _ = rounds
    found = sc.bpr_rounds_seed(m)
    assert found is not None
    seed, u, i, j = found
    assert len(set(u.tolist())) == sc.ROUNDS_N and len(set(i.tolist()) | set(j.tolist())) == 2 * sc.ROUNDS_N


@pytest.mark.parametrize("C", sc.ROUNDS_C)
def test_warp_rounds_seed_exists(rounds, C):
    m, rows = rounds
    case = sc.warp_rounds_case(m, rows, C)
    assert case is not None
    assert case["satisfied"] < sc.ROUNDS_N <= case["trials"]
    assert len(set(case["us"])) == sc.ROUNDS_N and len(set(case["touched"])) == len(case["touched"]) >= 2 * sc.ROUNDS_N - case["satisfied"]


# ---- 3. the search-cut matrix -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def search():
    return sc.search_matrix()


def test_search_matrix_has_every_length(search):
    m = search
    lens = np.diff(m.indptr)
    assert set(lens.tolist()) == set(sc.SEARCH_LENGTHS) | {0}
    for G in (16, 32, 64):
        assert {G - 1, G, G + 1, G * G - 1, G * G, G * G + 1} <= set(lens.tolist())
    assert m.shape[1] == sc.SEARCH_ITEMS and sc.hogwild_in_flight(m.nnz, *m.shape) == 16
    for r in range(m.shape[0]):
        assert (np.diff(m.indices[m.indptr[r]:m.indptr[r + 1]]) > 0).all()  # sorted, no duplicates
    assert m.indices.min() == 0 and m.indices.max() < sc.SEARCH_ITEMS


def _check_search_coverage(m, users, js, sample_users):
    lens = np.diff(m.indptr)
    per_len = np.bincount(lens[sample_users], minlength=lens.max() + 1)
    for n in sc.SEARCH_LENGTHS:
        assert per_len[n] >= 20, (n, per_len[n])
    hit, first, last, below, above = sc.search_outcomes(m, users, js)
    row_len = lens[users]
    for n in sc.SEARCH_LENGTHS:
        if n >= 15:
            at = row_len == n
            assert hit[at].any() and (~hit[at]).any(), n
    for G in (16, 32, 64):
        longer = row_len > G
        for name, what in (("first", first), ("last", last), ("below", below), ("above", above)):
            assert what[longer].any(), (G, name)
    return hit


@pytest.mark.parametrize("C", sc.SEARCH_C)
def test_bpr_frozen_epoch_covers_the_search(search, C):
    m = search
    X0, Y0 = sc.bpr_frozen_factors(m, C)
    skipped, correct, unsure, users, js = sc.bpr_frozen_counts(m, X0, Y0)
    hit = _check_search_coverage(m, users, js, users)
    assert skipped == int(hit.sum()) and 0 < skipped < m.nnz
    assert unsure <= 0.001 * m.nnz  # the share of samples the `correct` comparison leaves out
    assert 0 < correct < m.nnz - skipped - unsure


@pytest.mark.parametrize("C", sc.SEARCH_C)
def test_warp_frozen_epoch_covers_the_search(search, C):
    m = search
    X0, Y0 = sc.warp_frozen_factors(m, C)
    (satisfied, trials), closest, users, js = sc.warp_frozen_counts(m, X0, Y0)
    _check_search_coverage(m, users, js, wref.positives(m, sc.SEARCH_EPOCH_SEED)[0])
    assert closest >= sc.MARGIN
    assert 0.02 * m.nnz < satisfied < 0.98 * m.nnz  # satisfied and violating samples both occur
    assert m.nnz + satisfied * (sc.SEARCH_MAX_SAMPLED - 1) < trials < sc.SEARCH_MAX_SAMPLED * m.nnz  # late violations too


# ---- 4. LMF and evaluation shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [c for c in sc.LMF_DISPATCH_C if c not in sc.LMF_EXISTING_C])
def test_lmf_reduced_matrix_has_its_classes(C):
    mt = sc.lmf_reduced_matrix(C, seed=C).T.tocsr()
    G = sc.lmf_instantiation(C)[0]
    lens = np.diff(mt.indptr).tolist()
    assert max(lens) > 512 and {512, G - 1, G, G + 1, 1, 0} <= set(lens)
    m = sc.lmf_reduced_matrix(C, seed=C)
    assert (np.diff(m.indptr) == 0).any()
    # the float64 restatement holds a few C-wide rows per term: under 100 MB an array on both sides
    for csr, neg_prop in ((mt, 30), (m, 3)):
        n = np.diff(csr.indptr)
        assert (csr.nnz + np.minimum(C, n * neg_prop).sum()) * C * 8 < 100e6


def test_lmf_round_shapes_outnumber_the_groups_in_flight():
    assert [sc.lmf_instantiation(C)[0] for _, C, _ in sc.LMF_ROUND_SHAPES] == [16, 32, 64]
    assert [sc.lmf_groups_in_flight(C) for _, C, _ in sc.LMF_ROUND_SHAPES] == [32768, 16384, 8192]
    for rows, C, entries in sc.LMF_ROUND_SHAPES:
        if C == 130:
            continue  # the class matrix of test_gpu_lmf: its 24 000 users, less the empty ones, are checked there
        m = sc.lmf_round_matrix(rows, entries, seed=C)
        order = sc.lmf_schedule_order(m)
        lens = np.diff(m.indptr)
        assert sc.lmf_groups_in_flight(C) < len(order) < 2 * sc.lmf_groups_in_flight(C)
        assert (lens == 0).any() and (np.diff(lens[order]) <= 0).all() and lens[order[-1]] >= 1


def test_eval_shapes_take_the_steps_they_are_for():
    launches = {shape: sc.eval_launch(*shape) for shape in sc.EVAL_ROUND_SHAPES}
    assert launches == {(1029, 64): (64, 258, 258), (4101, 64): (64, 1026, 1024), (4101, 130): (64, 1026, 1024),
                        (16391, 10): (16, 1025, 1024), (262147, 1): (1, 1025, 1024)}
    assert [sc.eval_launch(1000, K)[0] for K in sc.EVAL_NEW_K] == [2, 8, 8, 32, 32, 64, 64, 64]
    assert sc.eval_launch(1000, 64)[1] == 250  # the largest case before: one tile per workgroup, 250 slots
