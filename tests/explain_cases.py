"""Inputs shared by tests/test_explain_host.py and tests/test_gpu_explain.py, with their float64 (and float32) restatement
results computed once per process (explain_reference.py).

ACCURACY: synthetic_csr(300, 400, 12000, seed=5, neg_frac=0.05), one explained item per user, item factors uniform in
+-0.05 from default_rng(1), regularization 0.01, at every factor count the kernels treat differently (4: one block; 16; 64:
one wavefront's width; 100: not a multiple of 4 x 4 blocks x wavefronts; 128; 256: the LDS limit, three rounds of register
blocks) and once with alpha = 40.

EDGES: one hand-made batch over 2500 items with N = 10 in mind: rows of 0, 1, 9, 10, 11, 63, 64, 65 and 700 entries, rows
of 2048 and 2049 (the last that keeps its contributions in the LDS and the first that spills them to the workspace), a row
of negative entries only, a row that likes the explained item and the same row explaining an item it does not like, the
last item id as explained and as liked item, the same user twice, and two liked items with identical factor rows and equal
confidence (the tie).
"""
import functools

import numpy as np
import scipy.sparse as sp

import explain_reference as ref
from implicit_amd.synthetic import synthetic_csr

REG = 0.01
ACCURACY = [(4, 1.0), (16, 1.0), (64, 1.0), (100, 1.0), (128, 1.0), (256, 1.0), (64, 40.0)]  # (factors, alpha)
ITEMS = 400
EDGE_ITEMS = 2500
EDGE_LENGTHS = [0, 1, 9, 10, 11, 63, 64, 65, 700, 2048, 2049]
TIE = (17, 905)  # identical factor rows


@functools.lru_cache(maxsize=None)
def accuracy_matrix():
    return synthetic_csr(300, ITEMS, 12000, seed=5, neg_frac=0.05)


@functools.lru_cache(maxsize=None)
def accuracy_items():
    return np.random.default_rng(2).integers(0, ITEMS, size=(300, 1)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def factors(f, items=ITEMS):
    Y = np.random.default_rng(1).uniform(-0.05, 0.05, size=(items, f)).astype(np.float32)
    if items == EDGE_ITEMS:
        Y[TIE[1]] = Y[TIE[0]]
    return Y


@functools.lru_cache(maxsize=None)
def accuracy_reference(f, alpha, dtype=np.float64, N=10):
    return ref.explain_batch(factors(f), accuracy_matrix(), accuracy_items(), REG, N, alpha=alpha, dtype=dtype)


@functools.lru_cache(maxsize=None)
def edge_matrix():
    """(user_items, names): one row per entry of `names`."""
    rng = np.random.default_rng(11)
    rows, names = [], []

    def add(name, cols, data):
        rows.append((np.asarray(cols, dtype=np.int32), np.asarray(data, dtype=np.float32)))
        names.append(name)

    for n in EDGE_LENGTHS:
        cols = np.sort(rng.choice(EDGE_ITEMS - 1, size=n, replace=False))  # never the last id
        data = 1.0 + 4.0 * rng.random(n)
        if n >= 63:
            data[rng.random(n) < 0.05] *= -1
        add(f"len{n}", cols, data)
    add("all_negative", [3, 50, 51, 1200, 2400], [-1.0, -2.5, -3.0, -1.5, -4.0])
    liked = [5, 40, 41, 300, 2000, EDGE_ITEMS - 1]           # likes item 40 and the last id
    add("likes_40", liked, [2.0, 3.0, 1.5, 4.0, 2.5, 3.5])
    add("likes_40_again", liked, [2.0, 3.0, 1.5, 4.0, 2.5, 3.5])  # the same user twice
    add("tie", [2, TIE[0], 400, TIE[1], 1999], [1.5, 3.0, 2.0, 3.0, 4.5])
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    m = sp.csr_matrix((np.concatenate([d for _, d in rows]), np.concatenate([c for c, _ in rows]), indptr),
                      shape=(len(rows), EDGE_ITEMS))
    return m, tuple(names)


@functools.lru_cache(maxsize=None)
def edge_items(M):
    """[B, M] explained items: column 0 is item 40 (liked by `likes_40`, not by the others' design) except that
    `likes_40_again` and `len1` explain the LAST id; further columns are random."""
    m, names = edge_matrix()
    ids = np.random.default_rng(12).integers(0, EDGE_ITEMS, size=(m.shape[0], M)).astype(np.int32)
    ids[:, 0] = 40
    ids[names.index("len1"), 0] = EDGE_ITEMS - 1
    ids[names.index("tie"), 0] = 7
    if M > 1:
        ids[names.index("likes_40"), 1] = 41 + 1   # an item this user does not like
        ids[names.index("likes_40_again"), 1] = EDGE_ITEMS - 1
    return ids


@functools.lru_cache(maxsize=None)
def edge_reference(f, M, N, dtype=np.float64):
    return ref.explain_batch(factors(f, EDGE_ITEMS), edge_matrix()[0], edge_items(M), REG, N, dtype=dtype)
