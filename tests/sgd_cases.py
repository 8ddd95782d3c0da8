"""The shapes the SGD and ranking-metric GPU tests run at, derived from the launch code of csrc/sgd_group.h, csrc/pair_sgd.hip,
csrc/bpr.hip, csrc/warp.hip, csrc/lmf.hip and csrc/evaluation.hip, and the host-side searches for the inputs those tests need.
tests/test_sgd_cases_host.py proves on the CPU that every list covers what it claims.  Test infrastructure only.

DISPATCH_C / LMF_DISPATCH_C: both ends of every (G, CPL) instantiation.  rounds_matrix, bpr_rounds_seed, warp_rounds_case:
the conflict-free call that takes two rounds of the persistent loops.  search_matrix and the *_frozen_* functions: the whole
epochs at zero learning rate.  lmf_reduced_matrix, LMF_ROUND_SHAPES: the LMF cases.  EVAL_ROUND_SHAPES: the evaluation
shapes with their tile and slot counts."""
import numpy as np
from scipy.sparse import csr_matrix

import bpr_reference as bref
import warp_reference as wref

LR, REG = 0.05, 0.01
MARGIN = 1e-4  # test_gpu_warp.MARGIN: no examined trial is closer to the violation threshold
NUM_CUS = 256  # the MI355X; the round counts quoted below hold there and are not asserted against the device


# ---- 1. the dispatch over lanes per sample and columns per lane ---------------------------------------------------------------
def pair_group(C, lanes=None):
    """pair_sgd.hip pair_group_lanes:
        if ((g == 16 || g == 32 || g == 64) && C <= 16 * g) return g;      (g = IMP_BPR_LANES)
        return group_lanes(C);"""
    if lanes in (16, 32, 64) and C <= 16 * lanes:
        return lanes
    return group_lanes(C)


def group_lanes(C):
    """sgd_group.h group_lanes: `return C <= 128 ? 16 : C <= 256 ? 32 : 64;`"""
    return 16 if C <= 128 else 32 if C <= 256 else 64


def columns_per_lane(cpl):
    """sgd_group.h columns_per_lane: `for (int v : {1, 2, 3, 4, 6, 8, 12}) if (cpl <= v) return v;  return 16;`"""
    return next(v for v in (1, 2, 3, 4, 6, 8, 12, 16) if cpl <= v)


def pair_instantiation(C, lanes=None):
    """imp_bpr_update / imp_warp_update: `for_group_shape<false>(G, a.C, ...)` with G = pair_group_lanes(C) (pair_sgd.hip
    pair_update); sgd_group.h for_columns_per_lane: `cpl = columns_per_lane((C + G - 1) / G)`, every one of the 24 pairs
    compiled."""
    G = pair_group(C, lanes)
    return G, columns_per_lane((C + G - 1) // G)


def lmf_instantiation(C):
    """lmf.hip launch_lmf: `G = group_lanes(a.C);  for_group_shape<true>(G, a.C, ...)`: the dispatcher of the pairwise
    kernels under the rule alone (IMP_BPR_LANES is not read), compiled for the pairs `rule_reaches` (sgd_group.h) only."""
    G = group_lanes(C)
    return G, columns_per_lane((C + G - 1) // G)


def rule_reaches(G, CPL):
    """sgd_group.h rule_reaches: `for (int C = 1; C <= 1024; ++C) if (group_lanes(C) == G && columns_per_lane((C + G - 1) /
    G) == CPL) return true;  return false;`"""
    return any(group_lanes(C) == G and columns_per_lane((C + G - 1) // G) == CPL for C in range(1, 1025))


INSTANTIATIONS = [(16, 1), (16, 2), (16, 3), (16, 4), (16, 6), (16, 8), (32, 6), (32, 8), (64, 6), (64, 8), (64, 12), (64, 16)]
PAIR_MIN_C, LMF_MIN_C, MAX_C = 2, 3, 1024  # the entry points' limits (imp_bpr_update / imp_warp_update, imp_lmf_update)


def dispatch_ends(instantiation_of, min_c):
    """{(G, CPL): (lowest C, highest C)} over the C the entry point accepts."""
    ends = {}
    for C in range(min_c, MAX_C + 1):
        lo, _ = ends.setdefault(instantiation_of(C), (C, C))
        ends[instantiation_of(C)] = (lo, C)
    return ends


def _with_ends(existing, instantiation_of, min_c):
    ends = dispatch_ends(instantiation_of, min_c)
    return sorted(set(existing) | {c for pair in ends.values() for c in pair})


# the values the tests had before (kept) plus both ends of every instantiation
DISPATCH_C = _with_ends([2, 17, 33, 65, 101, 129, 257, 1024], pair_instantiation, PAIR_MIN_C)
LMF_EXISTING_C = [3, 5, 32, 34, 66, 130, 1024]
LMF_DISPATCH_C = _with_ends(LMF_EXISTING_C, lmf_instantiation, LMF_MIN_C)

# IMP_BPR_LANES (read per call in pair_group_lanes): (lanes, C, the instantiation it must reach).  The first five and the last are
# the cases the switch was first tested at; with the others every instantiation that only the switch reaches is launched:
# <16, 12>, <16, 16>, <32, 1 .. 4>, <32, 12>, <32, 16>, <64, 1 .. 4>.  The last one must be ignored: C > 16 * lanes.
LANE_OVERRIDES = [(32, 17, (32, 1)), (64, 17, (64, 1)), (32, 64, (32, 2)), (64, 64, (64, 1)), (64, 129, (64, 3)),
                  (16, 192, (16, 12)), (16, 256, (16, 16)), (32, 96, (32, 3)), (32, 128, (32, 4)), (32, 384, (32, 12)),
                  (32, 512, (32, 16)), (64, 128, (64, 2)), (64, 256, (64, 4)),
                  (16, 257, (64, 6))]


def hogwild_in_flight(samples, users, items):
    """sgd_group.h: `std::min<int64_t>(samples, std::max<int64_t>(16, (int64_t)std::min(users, items) / 16))`."""
    return min(samples, max(16, min(users, items) // 16))


def factors(rows, C, rng, bias=None, scale=0.3):
    a = (rng.standard_normal((rows, C)) * scale).astype(np.float32)
    if bias is not None:
        a[:, C - 1] = bias
    return a


# ---- 2. the conflict-free call over two rounds ----------------------------------------------------------------------------
# 256 users: hogwild_in_flight is 16, so 16 groups at every G (grid = (16 G + 255) / 256 workgroups of 256 / G groups) take
# 24 samples in two rounds, the second half empty: `s + ngroups < samples` (bpr_update_kernel's prefetch guard) is true for
# groups 0 .. 7 and false for 8 .. 15, and in warp_update_kernel groups 0 .. 7 start a second sample while 8 .. 15 are done.
ROUNDS_N = 24
ROUNDS_C = [17, 128, 129, 256, 257, 1024]  # the bottom and the top of a range for each G
ROUNDS_MAX_SAMPLED = 4


def rounds_matrix():
    from implicit_amd.synthetic import synthetic_csr

    return synthetic_csr(256, 20000, 8000, gamma=1.0, seed=3)


def bpr_rounds_seed(m, n=ROUNDS_N):
    """The first seed whose n samples have distinct users and 2 n distinct items, with the triples; None if there is none."""
    for seed in range(1, 5000):
        u, i, j = bref.sample_ids(m, seed, n)
        if len(set(u.tolist())) == n and len(set(i.tolist()) | set(j.tolist())) == 2 * n:
            return seed, u, i, j
    return None


def rounds_factors(m, C):
    rng = np.random.default_rng(C)
    return factors(m.shape[0], C, rng, bias=1.0), factors(m.shape[1], C, rng)


def warp_rounds_case(m, rows, C, n=ROUNDS_N, max_sampled=ROUNDS_MAX_SAMPLED):
    """The first seed whose n samples have distinct users, distinct positives and examined candidates distinct from those and
    from each other, with no margin below MARGIN, on rounds_factors(m, C).  Returns a dict (seed, us, touched, satisfied,
    trials, X0, Y0 and the float64 result X64, Y64), or None."""
    items = m.shape[1]
    X0, Y0 = rounds_factors(m, C)
    X64, Y64 = X0.astype(np.float64), Y0.astype(np.float64)
    for seed in range(1, 5000):
        us, iis = (v.tolist() for v in wref.positives(m, seed, n))
        if len(set(us)) < n or len(set(iis)) < n:
            continue
        satisfied = trials = 0
        touched, closest = list(iis), np.inf
        for s, (u, i) in enumerate(zip(us, iis)):
            cand = wref.candidates(seed, s, items, max_sampled)
            t, used, margin = wref.step64(X64, Y64, rows[u], u, i, cand, LR, REG)
            satisfied, trials, closest = satisfied + (t is None), trials + used, min(closest, margin)
            touched += [j for j in cand[:used].tolist() if j not in rows[u]]  # the candidates it examined
        if len(set(touched)) == len(touched) and closest >= MARGIN:
            return dict(seed=seed, us=us, touched=touched, satisfied=satisfied, trials=trials, X0=X0, Y0=Y0, X64=X64, Y64=Y64)
        X64[us], Y64[touched] = X0[us], Y0[touched]  # as before this seed
    return None


# ---- 3. whole epochs at zero learning rate: the search-cut matrix -----------------------------------------------------------
# group_row_contains (sgd_group.h) runs `while (hi - lo > G)` with slices of ceil((hi - lo) / G): no splitter level up to G
# entries, one up to G^2, two above.  Row lengths on both sides of G and G^2 for G = 16, 32, 64 (and the lengths next to them):
SEARCH_LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
# short rows are the user of few samples (a sample picks its user by nonzero), so they are repeated
SEARCH_REPEATS = {1: 40, 15: 40, 16: 40, 17: 40, 31: 20, 32: 20, 33: 20, 63: 10, 64: 10, 65: 10}
SEARCH_EMPTY_ROWS = 5
SEARCH_ITEMS = 6000
SEARCH_MATRIX_SEED = 1
SEARCH_EPOCH_SEED = 1234
SEARCH_C = [17, 129, 257]  # one per G
SEARCH_MAX_SAMPLED = 10
SCORE_FLOOR = 1e-6  # BPR samples with a float64 |score| below this are left out of the `correct` comparison


def search_matrix(seed=SEARCH_MATRIX_SEED):
    """Rows of every SEARCH_LENGTHS length (and empty ones) in shuffled order over SEARCH_ITEMS items.  Columns are drawn
    without replacement with a popularity that falls from 1 to 0.02 along the item axis, as test_gpu_bpr._small_matrix does,
    and ten times two hundred for the first ten items, which about half of the short rows hold: BPR draws its negatives by
    popularity, so the liked check comes out both ways in short rows too.  Every other row draws only from items at or above
    a small offset (popular items fall below its first entry), every third row holds the last item of the catalogue (a
    popular item that is a row's last entry)."""
    rng = np.random.default_rng(seed)
    lens = [n for n in SEARCH_LENGTHS for _ in range(SEARCH_REPEATS.get(n, 1))] + [0] * SEARCH_EMPTY_ROWS
    lens = np.array(lens)[rng.permutation(len(lens))]
    weight = np.linspace(1.0, 0.02, SEARCH_ITEMS - 1)  # the last item is placed, not drawn
    weight[:10] *= 200.0
    rows = []
    for r, n in enumerate(lens.tolist()):
        first = int(rng.integers(1, 40)) if r % 2 else 0
        tail = [SEARCH_ITEMS - 1] if r % 3 == 0 and n >= 2 else []
        p = weight[first:] / weight[first:].sum()
        drawn = first + rng.choice(SEARCH_ITEMS - 1 - first, size=n - len(tail), replace=False, p=p)
        rows.append(np.sort(np.concatenate([drawn, tail]).astype(np.int64)))
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32)
    m = csr_matrix((np.ones(len(indices), dtype=np.float32), indices, indptr), shape=(len(lens), SEARCH_ITEMS))
    m.has_sorted_indices = True
    return m


def search_outcomes(m, users, js):
    """What the membership search of item js[k] in row users[k] meets: arrays (hit, first, last, below, above) -- found;
    found as the row's first / last entry; not found and below the first / above the last entry."""
    users, js = np.asarray(users, dtype=np.int64), np.asarray(js, dtype=np.int64)
    lens = np.diff(m.indptr)[users]
    assert (lens > 0).all()
    lo = m.indices[m.indptr[users]].astype(np.int64)
    hi = m.indices[m.indptr[users + 1] - 1].astype(np.int64)
    hit = bref.liked(m, users, js)
    return hit, hit & (js == lo), hit & (js == hi), ~hit & (js < lo), ~hit & (js > hi)


def bpr_frozen_factors(m, C):
    rng = np.random.default_rng(7000 + C)
    return factors(m.shape[0], C, rng, bias=1.0), factors(m.shape[1], C, rng)


def bpr_frozen_counts(m, X0, Y0, seed=SEARCH_EPOCH_SEED):
    """One verify_negative epoch on factors that stand still (lr = reg = 0): (skipped, correct, unsure, users, js) -- the
    skipped count, the float64 count of score >= SCORE_FLOOR among the others, the number with |score| < SCORE_FLOOR, and
    every sample's searched (user, item)."""
    u, i, j = bref.sample_ids(m, seed)
    skip = bref.liked(m, u, j)
    X, Y = X0.astype(np.float64), Y0.astype(np.float64)
    score = np.einsum("ij,ij->i", X[u[~skip]], Y[i[~skip]] - Y[j[~skip]])
    return int(skip.sum()), int((score >= SCORE_FLOOR).sum()), int((np.abs(score) < SCORE_FLOOR).sum()), u, j


def warp_frozen_factors(m, C):
    """Small factors (every |dot| without the bias stays below 0.3) and an item bias of -4 on six items in seven, 0 on the
    others: a candidate with the low bias never violates against a positive with the high one, any other pair does, so
    satisfied samples, first-trial violations and late ones all occur and no margin is near the threshold."""
    rng = np.random.default_rng(8000 + C)
    X0 = factors(m.shape[0], C, rng, scale=0.3 / np.sqrt(C))
    Y0 = factors(m.shape[1], C, rng, scale=0.3 / np.sqrt(C))
    X0[:, -1] = 1.0
    Y0[:, -1] = np.where(rng.random(m.shape[1]) < 6 / 7, -4.0, 0.0)
    return X0, Y0


def warp_frozen_counts(m, X0, Y0, seed=SEARCH_EPOCH_SEED, max_sampled=SEARCH_MAX_SAMPLED):
    """One epoch on factors that stand still: ((satisfied, trials), closest margin, users, js) with every consumed trial's
    searched (user, item)."""
    _, _, counts, closest = wref.serial_epochs(m, X0, Y0, [seed], 0.0, 0.0, max_sampled, with_margin=True)
    # the consumed trials again: a sample consumes its candidates up to the first that is not liked and violates
    X, Y = X0.astype(np.float64), Y0.astype(np.float64)
    us, iis = wref.positives(m, seed)
    users, js = [], []
    for k, (u, i) in enumerate(zip(us.tolist(), iis.tolist())):
        cand = wref.candidates(seed, k, m.shape[1], max_sampled)
        viol = ~np.isin(cand, m.indices[m.indptr[u]:m.indptr[u + 1]]) & (Y[cand] @ X[u] > float(X[u] @ Y[i]) - 1.0)
        used = int(np.argmax(viol)) + 1 if viol.any() else max_sampled
        users += [u] * used
        js += cand[:used].tolist()
    assert len(js) == counts[0][1]
    return counts[0], closest, np.array(users), np.array(js)


# ---- 4. LMF -------------------------------------------------------------------------------------------------------------------
def lmf_reduced_matrix(C, seed=0):
    """The class matrix of test_gpu_lmf._class_matrix cut down for wide rows (the float64 restatement holds a C-wide row per
    term): 700 users, some of them empty; the item side has a segmented row (600 entries), one of exactly 512, rows of G - 1, G and G + 1 entries
    for the G of C (one chunk of lmf_accumulate, exactly one, one and a lane), 300, 100, 5, 1, 1 and 0 entries."""
    G = lmf_instantiation(C)[0]
    users = 700
    rng = np.random.default_rng(seed)
    lens = [600, 512, G - 1, G, G + 1, 300, 100, 5, 1, 1, 0, 0]
    rows = np.concatenate([rng.choice(users, n, replace=False) for n in lens])
    cols = np.repeat(np.arange(len(lens)), lens)
    m = csr_matrix((rng.uniform(0.5, 4.0, len(rows)).astype(np.float32), (rows, cols)), shape=(users, len(lens)))
    m.sort_indices()
    return m


def lmf_groups_in_flight(C):
    """lmf.hip launch_lmf: `grid = min((work * G + 255) / 256, num_cus * 8)` workgroups of 256 / G groups."""
    return NUM_CUS * 8 * 256 // lmf_instantiation(C)[0]


# lmf_rows_kernel takes a second grid-stride step when the rows of 1 .. 512 entries outnumber the groups in flight:
# (rows, C, entries per row).  32 768 groups at G = 16, 16 384 at G = 32, 8 192 at G = 64.  The third is the shape
# test_half_sweeps_match_float64 already runs at C = 130 (the user side of its 24 000-user class matrix), stated as such.
LMF_ROUND_SHAPES = [(33000, 5, (1, 3)), (24000, 130, (1, 3)), (8300, 257, (1, 2))]


def lmf_round_matrix(rows, entries, items=40, seed=0):
    """`rows` rows of entries[0] .. entries[1] nonzeros over `items` columns, every 1000th row empty."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(entries[0], entries[1] + 1, rows)
    lens[::1000] = 0
    cols = np.concatenate([np.sort(rng.choice(items, n, replace=False)) for n in lens.tolist()]).astype(np.int32)
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    return csr_matrix((rng.uniform(0.5, 4.0, len(cols)).astype(np.float32), cols, indptr), shape=(rows, items))


def lmf_schedule_order(m):
    """The rows lmf_rows_kernel takes, in its order (csr_schedule.h: `order`, row ids by descending length, ascending id
    within a length; the kernel's range is the rows of 1 .. 512 entries)."""
    lens = np.diff(m.indptr)
    order = np.lexsort((np.arange(len(lens)), -lens))
    return order[(lens[order] >= 1) & (lens[order] <= 512)]


# ---- 5. ranking metrics -------------------------------------------------------------------------------------------------------
EVAL_BLOCK, EVAL_MAX_GRID = 256, 1024  # evaluation.hip kEvalBlock, kEvalMaxGrid


def eval_launch(n, K):
    """evaluation.hip imp_eval_add: `while (G < e->k && G < 64) G <<= 1;  tiles = (n + 256 / G - 1) / (256 / G);
    grid = min(tiles, kEvalMaxGrid)`.  Returns (G, tiles, slots): one workspace slot per workgroup."""
    G = 1
    while G < K and G < 64:
        G <<= 1
    tiles = (n + EVAL_BLOCK // G - 1) // (EVAL_BLOCK // G)
    return G, tiles, min(tiles, EVAL_MAX_GRID)


# (n, K): what the shape is for.  Tiles and slots are eval_launch's (independent of the CU count):
#   (1029, 64)    G 64,  258 tiles,  258 slots: eval_fold_kernel's `j += 256` takes a second step (slots 256, 257)
#   (4101, 64)    G 64, 1026 tiles, 1024 slots: workgroups 0 and 1 take a second tile, `run` is carried across tiles
#   (4101, 130)   G 64, 1026 tiles, 1024 slots: the same with three 64-wide chunks per row
#   (16391, 10)   G 16, 1025 tiles, 1024 slots
#   (262147, 1)   G 1,  1025 tiles, 1024 slots (host function only: the numpy restatement loops over rows in Python)
EVAL_ROUND_SHAPES = [(1029, 64), (4101, 64), (4101, 130), (16391, 10), (262147, 1)]
EVAL_NEW_K = [2, 5, 8, 17, 32, 128, 129, 200]
