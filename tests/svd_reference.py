"""Numpy restatements of the contracts behind PureSVD (include/implicit_hip.h on imp_csr_spmm and
imp_matrix_multiply_small; implicit_amd.gpu.randomized_svd) and the inputs the tests share.  Host arrays in, host arrays out;
nothing of the package under test is imported except the synthetic-matrix generator.

spmm32
    out[r][c] of A D for a row of at most SEGMENT stored entries is ((0 + a_1 D[j_1][c]) + a_2 D[j_2][c]) + ... in stored
    order, every product and sum one float32 operation.  A longer row is cut into runs of SEGMENT entries from its start; each
    run is summed that way from 0 and the runs' sums are added in order, starting from the first run's.  One answer, compared
    with assert_array_equal.

multiply_bound
    (l + 1) 2^-24 sum_i |y_i w_ij|: whatever the order of the l exact products' sum, its error stays below gamma_l <= that for
    l <= 1024.

rsvd
    The driver's algorithm with every large product in `dtype` (float64: the yardstick; float32: what any fp32 implementation
    may lose) and the l x l eigenproblems in float64, as the driver has them.
"""
import numpy as np
import scipy.sparse as sp

from implicit_amd.synthetic import synthetic_csr

SEGMENT = 1024
RANK_TOLERANCE = 2.0**-16
FLOOR = 2.0**-20


# ---- the sparse product -------------------------------------------------------------------------------------------------
def spmm32(A, D):
    """(float32 result in the stated order, float64 product) of the scipy CSR matrix A (stored order and duplicates kept as
    they are) and the dense D."""
    D32 = np.ascontiguousarray(D, dtype=np.float32)
    indptr, indices = np.asarray(A.indptr, dtype=np.int64), np.asarray(A.indices, dtype=np.int64)
    data = np.asarray(A.data, dtype=np.float32)
    rows, l = A.shape[0], D32.shape[1]
    seg_row, seg_begin, seg_end = [], [], []
    for r in range(rows):
        for b in range(indptr[r], indptr[r + 1], SEGMENT):
            seg_row.append(r), seg_begin.append(b), seg_end.append(min(indptr[r + 1], b + SEGMENT))
    seg_begin, seg_end = np.array(seg_begin, dtype=np.int64), np.array(seg_end, dtype=np.int64)
    partial = np.zeros((len(seg_row), l), dtype=np.float32)
    for t in range(int((seg_end - seg_begin).max()) if len(seg_row) else 0):
        live = np.flatnonzero(seg_begin + t < seg_end)
        p = seg_begin[live] + t
        partial[live] = partial[live] + data[p][:, None] * D32[indices[p]]  # float32 product, then float32 sum
    out = np.zeros((rows, l), dtype=np.float32)
    seen = np.zeros(rows, dtype=bool)
    for s, r in enumerate(seg_row):  # segment order
        out[r] = out[r] + partial[s] if seen[r] else partial[s]
        seen[r] = True
    exact = np.zeros((rows, l))
    D64 = D32.astype(np.float64)
    for r in range(rows):
        lo, hi = indptr[r], indptr[r + 1]
        exact[r] = data[lo:hi].astype(np.float64) @ D64[indices[lo:hi]]
    return out, exact


SPMM_ROWS, SPMM_COLS = 40, 300
SPMM_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000)
SPMM_WIDTHS = (1, 3, 24, 64, 65, 130, 264, 1024)


def spmm_case(integer=False, seed=11):
    """The 40 x 300 CSR matrix of the SpMM tests: every length of SPMM_LENGTHS, empty rows between the long ones, the rest short;
    columns are drawn with replacement (they repeat inside the long rows and across rows), values in [-2, 2] (integer: in
    {-2 .. 2}).  Not canonical on purpose: the contract is about stored order."""
    rng = np.random.default_rng(seed)
    lengths = [5000, 0, 2049, 0, 2048, 2047, 0, 1025, 1024, 1023, 257, 256, 255, 65, 64, 63, 2, 1, 0]
    assert set(SPMM_LENGTHS) <= set(lengths)
    lengths += [int(x) for x in rng.integers(1, 200, size=SPMM_ROWS - len(lengths))]
    lengths = np.array(lengths, dtype=np.int64)[rng.permutation(SPMM_ROWS)]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = rng.integers(0, SPMM_COLS, size=indptr[-1]).astype(np.int32)
    if integer:
        data = rng.integers(-2, 3, size=indptr[-1]).astype(np.float32)
    else:
        data = rng.uniform(-2, 2, size=indptr[-1]).astype(np.float32)
    return sp.csr_matrix((data, indices, indptr), shape=(SPMM_ROWS, SPMM_COLS))


def transpose_keeping_entries(A):
    """A^T as CSR with every stored entry kept (no duplicate is summed): 300 short rows."""
    coo = A.copy().tocoo()
    order = np.argsort(coo.col, kind="stable")
    counts = np.bincount(coo.col, minlength=A.shape[1])
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return sp.csr_matrix((coo.data[order].astype(np.float32), coo.row[order].astype(np.int32), indptr), shape=(A.shape[1], A.shape[0]))


def dense_case(rows, cols, integer=False, seed=5):
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    if integer:
        return rng.integers(-3, 4, size=(rows, cols)).astype(np.float32)
    return rng.standard_normal((rows, cols)).astype(np.float32)


# ---- the dense product --------------------------------------------------------------------------------------------------
MULTIPLY_ROWS = (0, 1, 63, 64, 65, 1000)
MULTIPLY_SHAPES = ((1, 1), (24, 16), (33, 32), (130, 128), (264, 256), (1024, 8))


def multiply_bound(Y, W):
    """(float64 product, per-entry bound) of Y W."""
    Y64, W64 = np.asarray(Y, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return Y64 @ W64, (Y64.shape[1] + 1) * 2.0**-24 * (np.abs(Y64) @ np.abs(W64))


# ---- the driver ---------------------------------------------------------------------------------------------------------
def _gram_eigh(Y):
    g = (Y.T @ Y).astype(np.float64)
    lam, W = np.linalg.eigh(0.5 * (g + g.T))
    return lam[::-1], W[:, ::-1]


def _kept(lam, tol):
    return (lam > tol * lam[0]) & (lam > 0)


def _orth(Y, tol):
    for _ in range(2):
        lam, W = _gram_eigh(Y)
        keep = _kept(lam, tol)
        T = np.zeros_like(W)
        T[:, keep] = W[:, keep] / np.sqrt(lam[keep])
        Y = Y @ T.astype(Y.dtype)
    return Y


def rsvd(A, k, p, q, omega, dtype, rank_tolerance=RANK_TOLERANCE):
    """(U users x k, sigma[k] float64, V items x k) of the scipy CSR matrix A by the driver's algorithm: sketch k + p, q power
    iterations, the test matrix `omega` (items x (k + p)); products in `dtype`."""
    A = A.copy().astype(dtype)  # scipy may sum duplicates in place: never on the caller's matrix
    At = A.T.tocsr()
    Q = _orth(A @ np.asarray(omega, dtype=dtype), rank_tolerance)
    for _ in range(q):
        Z = _orth(At @ Q, rank_tolerance)
        Q = _orth(A @ Z, rank_tolerance)
    B = At @ Q
    s2, W = _gram_eigh(B)
    keep = _kept(s2, rank_tolerance)[:k]
    sigma = np.zeros(k)
    sigma[keep] = np.sqrt(s2[:k][keep])
    Wu, Wv = np.zeros((k + p, k)), np.zeros((k + p, k))
    Wu[:, keep] = W[:, :k][:, keep]
    Wv[:, keep] = W[:, :k][:, keep] / sigma[keep]
    return Q @ Wu.astype(dtype), sigma, B @ Wv.astype(dtype)


def metrics(U, sigma, V, U64, sigma64, V64):
    """(m1, m2, m3, m4): max |sigma - sigma64| / sigma_1; the relative Frobenius distance of the two reconstructions; the
    orthonormality defects of V and of U over the non-zero triplets."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    want = (U64 * sigma64) @ V64.T
    live = sigma > 0
    n = int(live.sum())
    return (float(np.abs(sigma - sigma64).max() / sigma64[0]),
            float(np.linalg.norm((U * sigma) @ V.T - want) / np.linalg.norm(want)),
            float(np.abs(V[:, live].T @ V[:, live] - np.eye(n)).max()),
            float(np.abs(U[:, live].T @ U[:, live] - np.eye(n)).max()))


def rank12_case(seed=12):
    """300 users in 12 groups, every group one random set of 8 .. 29 of 200 items, binary values: rank 12."""
    rng = np.random.default_rng(seed)
    group = rng.permutation(np.arange(300) % 12)
    sets = [np.sort(rng.choice(200, size=int(rng.integers(8, 30)), replace=False)) for _ in range(12)]
    indptr = np.concatenate([[0], np.cumsum([len(sets[g]) for g in group])]).astype(np.int32)
    indices = np.concatenate([sets[g] for g in group]).astype(np.int32)
    return sp.csr_matrix((np.ones(len(indices), dtype=np.float32), indices, indptr), shape=(300, 200))


def long_row_case():
    """synthetic_csr(300, 200, 3000, seed=7) with one more user of 1500 stored entries: more than the 200 items, so its
    columns repeat (the matrix is not canonical; as a linear map the repeats add up) and the row takes the long-row path."""
    base = synthetic_csr(300, 200, 3000, seed=7)
    rng = np.random.default_rng(70)
    cols = rng.integers(0, 200, size=1500).astype(np.int32)
    vals = rng.uniform(0.0, 0.25, size=1500).astype(np.float32)
    indptr = np.concatenate([base.indptr, [base.indptr[-1] + 1500]]).astype(np.int32)
    return sp.csr_matrix((np.concatenate([base.data, vals]), np.concatenate([base.indices, cols]), indptr), shape=(301, 200))


# name -> (matrix, k, p, q)
def driver_cases():
    return {
        "rank12": (rank12_case(), 16, 8, 1),
        "generic300": (synthetic_csr(300, 200, 3000, seed=7), 16, 8, 2),
        "generic500": (synthetic_csr(500, 130, 6000, seed=3), 32, 8, 2),
        "longrow": (long_row_case(), 16, 8, 2),
    }


def omega_for(A, k, p, seed=99):
    return np.random.default_rng(seed).standard_normal((A.shape[1], k + p)).astype(np.float32)
