"""The inputs of tests/test_gpu_serving.py as pure functions of seeds, shared with the margin census of
tests/test_serving_host.py (which proves on the host that the float64 answers of these very cases hold few near-ties).
Numpy and scipy only: nothing of the package under test is imported here."""
import functools

import numpy as np
import scipy.sparse as sp

import serving_reference as ref

USERS, ITEMS, SMALL_ITEMS = 400, 1000, 300
REG = 0.05

# name -> (model class, stored width, storage dtype, items, seed); bpr / lmf store factors + 1 / factors + 2 columns
MODELS = {
    "als32": ("als", 32, np.float32, ITEMS, 1),
    "als64": ("als", 64, np.float32, ITEMS, 2),
    "als128": ("als", 128, np.float32, ITEMS, 3),
    "als64h": ("als", 64, np.float16, ITEMS, 4),
    "bpr33": ("bpr", 33, np.float32, ITEMS, 5),
    "lmf34": ("lmf", 34, np.float32, ITEMS, 6),
    "als32s": ("als", 32, np.float32, SMALL_ITEMS, 7),
}

# planted rows, all below SMALL_ITEMS so that every model has them
DUP_ITEMS = ((17, 150, 290), (250, 251))  # identical item rows
ZERO_ITEM = 77
LEAD_USER = 131       # 3 x item row 17: the duplicates lead its list
ZERO_USER = 259
DUP_USERS = (40, 333)
LIKES_ALL, LIKES_NONE = 100, 101
PLANTED_ITEMS = frozenset(i for g in DUP_ITEMS for i in g) | {ZERO_ITEM}
PLANTED_USERS = frozenset(DUP_USERS) | {ZERO_USER}


@functools.lru_cache(maxsize=None)
def factors(name):
    """(X, Y) in the model's storage dtype: seeded standard_normal * 0.1 with the planted rows."""
    _, width, dtype, items, seed = MODELS[name]
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((USERS, width)) * 0.1).astype(np.float32)
    Y = (rng.standard_normal((items, width)) * 0.1).astype(np.float32)
    for group in DUP_ITEMS:
        Y[list(group[1:])] = Y[group[0]]
    Y[ZERO_ITEM] = 0
    X[LEAD_USER] = 3 * Y[DUP_ITEMS[0][0]]
    X[ZERO_USER] = 0
    X[DUP_USERS[1]] = X[DUP_USERS[0]]
    X, Y = X.astype(dtype), Y.astype(dtype)
    X.setflags(write=False), Y.setflags(write=False)
    return X, Y


def _pattern(rows, cols, per_row, everything, nothing, seed):
    """CSR from its three arrays: rows in shuffled (unsorted) order, every fifth stored value an explicit zero."""
    rng = np.random.default_rng(seed)
    indptr, indices = [0], []
    for r in range(rows):
        n = cols if r == everything else 0 if r in nothing else int(rng.integers(1, per_row))
        indices.append(rng.permutation(cols)[:n])
        indptr.append(indptr[-1] + n)
    indices = np.concatenate(indices).astype(np.int32)
    data = rng.integers(1, 5, len(indices)).astype(np.float32)
    data[::5] = 0
    return sp.csr_matrix((data, indices, np.array(indptr, dtype=np.int32)), shape=(rows, cols))


@functools.lru_cache(maxsize=None)
def liked(items=ITEMS):
    """users x items; LIKES_ALL likes every item, LIKES_NONE and user 200 nothing."""
    return _pattern(USERS, items, 60, LIKES_ALL, (LIKES_NONE, 200), 11)


@functools.lru_cache(maxsize=None)
def likers():
    """items x users, the rows recalculate_item / partial_fit_items are fed."""
    return _pattern(ITEMS, USERS, 40, -1, (5,), 12)


def rows_of(m, ids):
    return m[int(ids)] if np.isscalar(ids) else m[np.asarray(ids)]


# ---- recommend ----------------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(99)
VIEW = np.arange(77, 300)                       # crosses rows 128 and 256, holds LIKES_ALL, LIKES_NONE, LEAD_USER, ZERO_USER
UNSORTED = _rng.permutation(USERS)[:150]
REPEATED = np.array([5, 5, 6, 129, 5, LEAD_USER, 6, LIKES_ALL])
SUBSET = [int(i) for i in _rng.permutation(ITEMS)[:120]] + [17, 150, 77]          # unsorted, with two duplicates
SMALL_SUBSET = [int(i) for i in _rng.permutation(SMALL_ITEMS)[:60]] + [17, 150, 77]
LIKED7 = [int(i) for i in liked()[7].indices]                                       # stored zeros included
NOT_LIKED7 = [i for i in range(ITEMS - 1, -1, -3) if i not in LIKED7]


def _rec(name, userid, model="als32", N=10, filter_liked=True, filter_items=None, items=None):
    return dict(call="recommend", name=name, model=model, userid=userid, N=N, filter_liked=filter_liked,
                filter_items=filter_items, items=items)


def _recommend_cases():
    c = [
        _rec("int", 7), _rec("int-likes-all", LIKES_ALL), _rec("int-likes-nothing", LIKES_NONE),
        _rec("int-duplicates-lead-N1", LEAD_USER, N=1), _rec("int-duplicates-lead-N2", LEAD_USER, N=2),
        _rec("int-duplicates-lead", LEAD_USER, filter_liked=False),
        _rec("int64-scalar", np.int64(300)), _rec("one-element", np.array([130])),
        _rec("run-from-0", np.arange(200)), _rec("view", VIEW), _rec("view-as-list", [int(u) for u in VIEW]),
        _rec("unsorted", UNSORTED), _rec("repeated", REPEATED),
        _rec("int32", np.arange(120, 140, dtype=np.int32)), _rec("int64", np.arange(250, 262, dtype=np.int64)),
    ]
    for N in (1, 37, 300, ITEMS, ITEMS + 200):
        for filter_liked in (True, False):
            c.append(_rec(f"view-N{N}-{'liked' if filter_liked else 'all'}", VIEW, N=N, filter_liked=filter_liked))
    for N in (SMALL_ITEMS, SMALL_ITEMS + 100):
        for filter_liked in (True, False):
            c.append(_rec(f"small-N{N}-{'liked' if filter_liked else 'all'}", VIEW, model="als32s", N=N, filter_liked=filter_liked))
    c += [
        _rec("filter-list", VIEW, filter_items=[3, 17, 999]), _rec("filter-ndarray", VIEW, filter_items=np.array([3, 17, 999])),
        _rec("filter-duplicates", UNSORTED, filter_items=[3, 3, 17, 3, 999], filter_liked=False),
        _rec("filter-empty", VIEW, filter_items=[]), _rec("filter-scalar-user", 7, filter_items=[3, 17, 999]),
        _rec("items", VIEW, items=SUBSET), _rec("items-all", VIEW, items=SUBSET, filter_liked=False),
        _rec("items-ndarray", UNSORTED, items=np.array(SUBSET)),
        _rec("items-N-above", VIEW, items=SUBSET, N=len(SUBSET) + 80), _rec("items-N-above-all", REPEATED, items=SUBSET, N=500, filter_liked=False),
        _rec("items-scalar", 7, items=SUBSET), _rec("items-none-liked", 7, items=NOT_LIKED7),
        _rec("items-only-liked", 7, items=LIKED7), _rec("items-only-liked-all", 7, items=LIKED7, filter_liked=False),
        _rec("items-duplicates-lead", LEAD_USER, items=SUBSET, N=2, filter_liked=False),
    ]
    for model in ("als64", "als128", "als64h", "bpr33", "lmf34", "als32s"):
        sub = SMALL_SUBSET if model == "als32s" else SUBSET
        c += [
            _rec("view", VIEW, model=model), _rec("view-as-list", [int(u) for u in VIEW], model=model),
            _rec("unsorted-N37-all", UNSORTED, model=model, N=37, filter_liked=False),
            _rec("items", REPEATED, model=model, items=sub), _rec("int-duplicates-lead", LEAD_USER, model=model, N=3, filter_liked=False),
            _rec("filter-list", np.arange(120, 140), model=model, filter_items=[3, 17, 250]),
        ]
    return c


# ---- similar_items / similar_users -------------------------------------------------------------------------------------
ITEM_BATCH = np.array([17, 250, ZERO_ITEM, 290] + [int(i) for i in _rng.permutation(SMALL_ITEMS)[:30]])
USER_BATCH = np.array([ZERO_USER, LEAD_USER, 40, 333] + [int(i) for i in _rng.permutation(USERS)[:30]])
ITEM_SUBSET = [int(i) for i in _rng.permutation(ITEMS)[:90]] + [17, ZERO_ITEM, 251]
USER_SUBSET = [int(i) for i in _rng.permutation(USERS)[:70]] + [ZERO_USER, 40]


def _sim(call, name, qid, model="als32", N=10, filter_ids=None, subset=None):
    return dict(call=call, name=name, model=model, qid=qid, N=N, filter_ids=filter_ids, subset=subset)


def _similar_cases():
    c = []
    for call, batch, sub, zero, count in (("similar_items", ITEM_BATCH, ITEM_SUBSET, ZERO_ITEM, ITEMS),
                                          ("similar_users", USER_BATCH, USER_SUBSET, ZERO_USER, USERS)):
        c += [
            _sim(call, "scalar", 8), _sim(call, "scalar-duplicate-N1", int(batch[0]), N=1), _sim(call, "scalar-duplicate", int(batch[0])),
            _sim(call, "scalar-zero-query", zero), _sim(call, "int64-scalar", np.int64(12)),
            _sim(call, "batch", batch), _sim(call, "batch-as-list", [int(i) for i in batch]), _sim(call, "batch-N37", batch, N=37),
            _sim(call, "N-catalogue", batch[:6], N=count), _sim(call, "N-above", batch[:6], N=count + 50),
            _sim(call, "filter", batch, filter_ids=[int(batch[0]), 3, zero]), _sim(call, "filter-ndarray", 8, filter_ids=np.array([8, 3])),
            _sim(call, "filter-empty", batch, filter_ids=[]), _sim(call, "filter-zero-query", zero, filter_ids=[1, 2]),
            _sim(call, "subset", batch, subset=sub), _sim(call, "subset-scalar", int(batch[1]), subset=sub),
            _sim(call, "subset-N-above", batch[:6], subset=sub, N=len(sub) + 20),
        ]
        for model in ("als64", "als128", "als64h", "bpr33", "lmf34", "als32s"):
            c += [_sim(call, "batch", batch, model=model), _sim(call, "scalar-duplicate", int(batch[0]), model=model, N=4),
                  _sim(call, "subset", batch[:8], model=model, subset=SMALL_SUBSET if call == "similar_items" else USER_SUBSET)]
    return c


CASES = _recommend_cases() + _similar_cases()


def case_id(case):
    return f"{case['model']}-{case['call']}-{case['name']}"


def width(case):
    return MODELS[case["model"]][1]


def expected(case, extra=0):
    """The restatement's (ids, scores) for a case; extra: ask for N + extra (the census looks one past the end)."""
    X, Y = factors(case["model"])
    N = case["N"] + extra
    if case["call"] == "recommend":
        return ref.recommend(X, Y, case["userid"], rows_of(liked(len(Y)), case["userid"]), N, case["filter_liked"],
                             case["filter_items"], case["items"])
    return ref.similar(Y if case["call"] == "similar_items" else X, case["qid"], N, case["subset"], case["filter_ids"])


def census(case):
    """(close, compared positions): near-ties among the float64 scores this case compares, the score after the last
    position included; compared positions = rows x written columns."""
    ids, scores = (np.atleast_2d(a) for a in expected(case, extra=1))
    X, Y = factors(case["model"])
    if case["call"] == "recommend":
        candidates = len(Y) if case["items"] is None else len(case["items"])
        planted, queries, zero_queries = PLANTED_ITEMS, np.atleast_1d(case["userid"]), (ZERO_USER,)
    else:
        item_side = case["call"] == "similar_items"
        candidates = len(case["subset"]) if case["subset"] is not None else len(Y if item_side else X)
        planted = PLANTED_ITEMS if item_side else PLANTED_USERS
        queries, zero_queries = np.atleast_1d(case["qid"]), ((ZERO_ITEM,) if item_side else (ZERO_USER,))
    written = min(scores.shape[1], candidates)
    rows = ~np.isin(queries, zero_queries)  # a zero query scores 0 everywhere: its order is the id rule alone
    close, _ = ref.near_ties(ids[rows, :written], scores[rows, :written], width(case), planted)
    return close, len(queries) * min(case["N"], candidates)
