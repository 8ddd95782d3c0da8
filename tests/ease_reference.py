"""Host restatement of EASE (numpy only) and the inputs the CPU and the GPU suites share.

    G = X^T X + lambda I,  P = G^-1,  B[i, j] = -P[i, j] / P[j, j] (i != j),  B[j, j] = 0,  score(u, .) = X[u, :] B

gram64 / ease64 are the float64 closed form; weights32, scores32 and topk_order restate, operation for operation, what
imp_ease_weights and imp_ease_topk promise bit for bit (include/implicit_hip.h)."""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from implicit_amd.synthetic import synthetic_csr  # noqa: E402

FLT_MAX = np.finfo(np.float32).max
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ease_golden.npz")


# ---- the float64 closed form ----------------------------------------------------------------------------------------------
def gram64(X, reg):
    """X^T X + reg I in float64 from a scipy sparse or dense users x items matrix."""
    D = np.asarray(X.todense() if sp.issparse(X) else X, dtype=np.float64)
    return D.T @ D + float(reg) * np.eye(D.shape[1])


def weights64(P):
    B = -P / np.diag(P)[None, :]
    np.fill_diagonal(B, 0.0)
    return B


def ease64(X, reg):
    return weights64(np.linalg.inv(gram64(X, reg)))


# ---- the bitwise rules ----------------------------------------------------------------------------------------------------
def weights32(P):
    """B[i, j] = -(P[i, j] / P[j, j]): one IEEE float32 division and a sign flip; zero diagonal."""
    P = np.asarray(P, dtype=np.float32)
    B = -(P / np.diag(P)[None, :])
    np.fill_diagonal(B, np.float32(0.0))
    return B.astype(np.float32)


def scores32(B, indices, data):
    """((0 + x_1 B[i_1, :]) + x_2 B[i_2, :]) + ...: every product and every sum a separately rounded float32 operation."""
    B = np.asarray(B, dtype=np.float32)
    s = np.zeros(B.shape[1], dtype=np.float32)
    for i, x in zip(indices, np.asarray(data, dtype=np.float32)):
        s = s + x * B[i]  # float32 * float32 -> float32, then float32 + float32 -> float32
    return s


def topk_order(scores, k):
    """(ids, scores) of the k best under the project's total order: score descending, id descending, -0.0 as +0.0; padded
    with (-1, -FLT_MAX) past len(scores)."""
    s = np.asarray(scores, dtype=np.float32)
    key = np.where(s == 0, np.float32(0.0), s)  # -0.0 ranks, and is returned, as +0.0
    order = np.lexsort((-np.arange(len(s)), -key.astype(np.float64)))[:k]
    ids = np.full(k, -1, dtype=np.int32)
    out = np.full(k, -FLT_MAX, dtype=np.float32)
    ids[:len(order)] = order
    out[:len(order)] = key[order]
    return ids, out


def recommend32(B, rows, k, filter_liked=False, item_filter=None):
    """The restatement of imp_ease_topk for every row of the CSR matrix `rows`."""
    ids = np.empty((rows.shape[0], k), dtype=np.int32)
    out = np.empty((rows.shape[0], k), dtype=np.float32)
    for r in range(rows.shape[0]):
        lo, hi = rows.indptr[r], rows.indptr[r + 1]
        s = scores32(B, rows.indices[lo:hi], rows.data[lo:hi])
        if filter_liked:
            s[rows.indices[lo:hi]] = -FLT_MAX
        if item_filter is not None and len(item_filter):
            s[np.asarray(item_filter)] = -FLT_MAX
        ids[r], out[r] = topk_order(s, k)
    return ids, out


# ---- yardstick of the inverse ---------------------------------------------------------------------------------------------
def lapack32_inverse(G32):
    """LAPACK's float32 Cholesky inverse (spotrf + spotri) of the lower triangle, mirrored."""
    from scipy.linalg import lapack

    c, info = lapack.spotrf(np.asarray(G32, dtype=np.float32), lower=1)
    assert info == 0
    p, info = lapack.spotri(c, lower=1)
    assert info == 0
    return np.tril(p) + np.tril(p, -1).T


def rel_distance(P, P64):
    return float(np.linalg.norm(np.asarray(P, dtype=np.float64) - P64) / np.linalg.norm(P64))


# ---- cases ----------------------------------------------------------------------------------------------------------------
SPD_BLOCK = 128  # the block size spd_inverse.hip chose
SPD_SIZES = sorted({1, 2, 31, 64, 65, 127, 129, 200, 257, 300,
                    SPD_BLOCK - 1, SPD_BLOCK, SPD_BLOCK + 1, 2 * SPD_BLOCK + 1, 4 * SPD_BLOCK + 3})
_spd_cache = {}


def spd_case(n):
    """float32 SPD matrix of order n: X^T X + 10 I of synthetic_csr(4n, n, 48n, seed=n); for n <= 2, M^T M + 3 I with M 5 x n
    uniform.  Returns (G32, P64) with P64 the float64 inverse of the float32 matrix."""
    if n not in _spd_cache:
        if n <= 2:
            M = np.random.default_rng(n).random((5, n))
            G = M.T @ M + 3.0 * np.eye(n)
        else:
            G = gram64(synthetic_csr(4 * n, n, 48 * n, seed=n), 10.0)
        G32 = np.ascontiguousarray(G, dtype=np.float32)
        P64 = np.linalg.inv(G32.astype(np.float64))
        G32.setflags(write=False)
        P64.setflags(write=False)
        _spd_cache[n] = (G32, P64)
    return _spd_cache[n]


GRAM_EXACT_ITEMS = (1, 2, 63, 64, 65, 70, 257)
GRAM_REG = 3.0


def gram_exact_case(items):
    """users ~ 4 x items, integer values 1..3: an empty user row (user 1), an item nobody has (the last but one, when
    2 < items < 257), one item held by every other user (item 0: the long chain) and, at items = 257, a user row holding every
    item (257 entries: longer than one 256-thread step of the kernel)."""
    rng = np.random.default_rng(1000 + items)
    users = 4 * items + 3
    D = np.zeros((users, items), dtype=np.float32)
    dens = min(0.3, 8.0 / items + 0.05)
    mask = rng.random((users, items)) < dens
    D[mask] = rng.integers(1, 4, size=int(mask.sum()))
    D[:, 0] = rng.integers(1, 4, size=users)  # the long chain
    if items == 257:
        D[2, :] = rng.integers(1, 4, size=items)  # a user row longer than one workgroup step
    if 2 < items < 257:
        D[:, items - 2] = 0  # an item nobody has
    D[1, :] = 0  # an empty user row
    m = sp.csr_matrix(D)
    m.sort_indices()
    return m


def max_partial_sum(X):
    """The largest value any partial sum of a Gram entry (the regularised diagonal included) can reach."""
    D = np.abs(np.asarray(X.todense(), dtype=np.float64))
    return float((D.T @ D).max() + GRAM_REG)


def topk_case(items, seed=0):
    """(B, rows): a random float32 B with two identical columns (exact ties) and zeros of both signs, and query rows: empty,
    one entry, every item, 300 entries (or every item when items < 300), mixed signs."""
    rng = np.random.default_rng(items * 7 + seed)
    B = (rng.random((items, items), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    B[rng.random((items, items)) < 0.05] = np.float32(0.0)
    B[rng.random((items, items)) < 0.05] = np.float32(-0.0)
    if items >= 5:
        B[:, 3] = B[:, 1]  # duplicated score bits
    np.fill_diagonal(B, 0.0)
    rows = [np.zeros(0, np.int64), np.array([items // 2]), np.arange(items),
            np.sort(rng.choice(items, size=min(300, items), replace=False)),
            np.sort(rng.choice(items, size=min(7, items), replace=False))]
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    data = ((rng.random(len(indices), dtype=np.float32) - np.float32(0.5)) * np.float32(4.0)).astype(np.float32)
    data[:1] = np.float32(1.0)
    m = sp.csr_matrix((data, indices, indptr), shape=(len(rows), items))
    return B, m


TOPK_ITEMS = (1, 5, 70, 257, 5000)


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
