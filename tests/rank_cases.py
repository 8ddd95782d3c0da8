"""The inputs of tests/test_gpu_rank.py and tests/test_rank_host.py as pure functions of seeds.  Numpy and scipy only: nothing
of the package under test is imported here."""
import functools

import numpy as np
import scipy.sparse as sp

USERS, ITEMS = 48, 6000
REG = 0.05

# name -> (model class, stored width, storage dtype, seed); bpr / lmf store factors + 1 / factors + 2 columns
MODELS = {
    "als32": ("als", 32, np.float32, 1),
    "als64": ("als", 64, np.float32, 2),
    "als128": ("als", 128, np.float32, 3),
    "als256": ("als", 256, np.float32, 4),
    "als64h": ("als", 64, np.float16, 5),
    "bpr33": ("bpr", 33, np.float32, 6),
    "lmf34": ("lmf", 34, np.float32, 7),
    "als100": ("als", 100, np.float32, 8),
}

# every length at which the kernel takes another step: the unroll (4), a wavefront's share, the block (512), the powers of two of
# the sort, the LDS / select split at 4096 and its n limit of 1024, and every item
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5000, 6000)
REPEAT_LENGTHS = (64, 257, 4096, 5000)  # lists in which one id occurs three times

DUP_ITEMS = ((17, 150, 290), (250, 251))  # identical item rows
ZERO_ITEM = 77
PLANTED_ITEMS = tuple(i for g in DUP_ITEMS for i in g) + (ZERO_ITEM,)
ZERO_USER = 31           # list of 4097
DUP_USERS = (13, 30)     # lists of 4096
LIKES_ALL, LIKES_NONE = 16, 15  # lists of 6000 and 5000


def length_of(user):
    return LENGTHS[user % len(LENGTHS)]


@functools.lru_cache(maxsize=None)
def factors(name):
    """(X, Y) in the model's storage dtype: seeded standard_normal * 0.1 with the planted rows."""
    _, width, dtype, seed = MODELS[name]
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((USERS, width)) * 0.1).astype(np.float32)
    Y = (rng.standard_normal((ITEMS, width)) * 0.1).astype(np.float32)
    for group in DUP_ITEMS:
        Y[list(group[1:])] = Y[group[0]]
    Y[ZERO_ITEM] = 0
    X[ZERO_USER] = 0
    X[DUP_USERS[1]] = X[DUP_USERS[0]]
    X, Y = X.astype(dtype), Y.astype(dtype)
    X.setflags(write=False), Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def lists():
    """One unsorted list per user, user u's of length_of(u); lists of >= 63 entries hold every planted item, those of
    REPEAT_LENGTHS one id three times."""
    rng = np.random.default_rng(21)
    plain = np.setdiff1d(np.arange(ITEMS), PLANTED_ITEMS)
    out = []
    for u in range(USERS):
        n = length_of(u)
        if n >= 63:
            ids = np.concatenate([rng.permutation(plain)[:n - len(PLANTED_ITEMS)], PLANTED_ITEMS])
            ids = rng.permutation(ids)
        else:
            ids = rng.permutation(plain)[:n]
        if n in REPEAT_LENGTHS:
            ids[n // 2] = ids[n - 1] = ids[0]
        ids = ids.astype(np.int32)
        ids.setflags(write=False)
        out.append(ids)
    return tuple(out)


def lists_of(userids):
    return [lists()[int(u)] for u in np.atleast_1d(userids)]


PAD_WIDTH = ITEMS + 100


def padded(userids):
    """The same lists as a 2-d array: every row's entries in order at random columns, -1 (and -7) everywhere else."""
    rng = np.random.default_rng(22)
    userids = np.atleast_1d(userids)
    out = np.full((len(userids), PAD_WIDTH), -1, dtype=np.int32)
    out[:, ::3] = -7
    for r, ids in enumerate(lists_of(userids)):
        cols = np.sort(rng.choice(PAD_WIDTH, size=len(ids), replace=False))
        out[r, cols] = ids
    return out


@functools.lru_cache(maxsize=None)
def liked():
    """users x items from its three arrays: indices in shuffled (unsorted) order inside a row, every fifth stored value an
    explicit zero; LIKES_ALL likes every item, LIKES_NONE and user 3 nothing."""
    rng = np.random.default_rng(23)
    indptr, indices = [0], []
    for u in range(USERS):
        n = ITEMS if u == LIKES_ALL else 0 if u in (LIKES_NONE, 3) else int(rng.integers(1, 1500))
        indices.append(rng.permutation(ITEMS)[:n])
        indptr.append(indptr[-1] + n)
    indices = np.concatenate(indices).astype(np.int32)
    data = rng.integers(1, 5, len(indices)).astype(np.float32)
    data[::5] = 0
    return sp.csr_matrix((data, indices, np.array(indptr, dtype=np.int32)), shape=(USERS, ITEMS))


def rows_of(m, ids):
    return m[int(ids)] if np.isscalar(ids) else m[np.asarray(ids)]


# user id forms, as tests/serving_cases.py has them
_rng = np.random.default_rng(99)
ALL = np.arange(USERS)
VIEW = np.arange(5, 40)
UNSORTED = _rng.permutation(USERS)[:20]
REPEATED = np.array([5, 5, 6, 29, 5, ZERO_USER, 6, LIKES_ALL])
SHORT_USERS = np.array([u for u in range(USERS) if length_of(u) <= 4096])  # a batch with no list over 4096
