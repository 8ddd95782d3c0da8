"""Float64 numpy restatement of the sparse x sparse top-k contract (include/implicit_hip.h imp_sparse_topk_product,
csrc/knn.hip) and of the similarity structure the item-item models build from it.  Test code only.

product_topk(A, B, k, zero_own): for every row r of A the touched columns of A[r].B, every column's sum taken as
((0.0 + B[u1,j]*A[r,u1]) + B[u2,j]*A[r,u2]) + ... in A[r]'s stored order (np.add.at applies its updates in index order),
then the k best under (score, column) descending."""
import numpy as np
import scipy.sparse as sp


def product_topk(A, B, k, zero_own=False, chunk_pairs=1 << 24):
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    R, C = A.shape[0], B.shape[1]
    ids = np.full((R, k), -1, dtype=np.int32)
    scores = np.full((R, k), -np.inf)
    counts = np.zeros(R, dtype=np.int32)
    blen = np.diff(B.indptr)
    # pairs per row, for the chunking alone (prefix sums: reduceat rejects the offsets of trailing empty rows)
    work = np.diff(np.concatenate([[0], np.cumsum(blen[A.indices], dtype=np.int64)])[A.indptr])
    r0 = 0
    while r0 < R:
        r1, acc = r0, 0
        while r1 < R and (r1 == r0 or acc + work[r1] <= chunk_pairs) and (r1 - r0) * C < (1 << 26):
            acc += work[r1]
            r1 += 1
        _chunk(A, B, k, zero_own, r0, r1, ids, scores, counts)
        r0 = r1
    return ids, scores, counts


def _chunk(A, B, k, zero_own, r0, r1, ids, scores, counts):
    C = B.shape[1]
    p0, p1 = A.indptr[r0], A.indptr[r1]
    u = A.indices[p0:p1]
    a = A.data[p0:p1].astype(np.float64)
    prow = np.repeat(np.arange(r0, r1), np.diff(A.indptr[r0:r1 + 1]))
    L = B.indptr[u + 1] - B.indptr[u]
    start = np.repeat(B.indptr[u], L)
    offs = np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)
    q = start + offs
    flat = (np.repeat(prow, L) - r0) * C + B.indices[q]
    sums = np.zeros((r1 - r0) * C)
    np.add.at(sums, flat, B.data[q].astype(np.float64) * np.repeat(a, L))
    touched = np.zeros((r1 - r0) * C, dtype=bool)
    touched[flat] = True
    if zero_own:
        own = (prow - r0) * C + u
        own = own[touched[own]]
        sums[own] = 0.0
    rr, cc = np.divmod(np.flatnonzero(touched), C)
    ss = sums[rr * C + cc]
    order = np.lexsort((-cc, -ss, rr))
    rr, cc, ss = rr[order], cc[order], ss[order]
    first = np.searchsorted(rr, np.arange(r1 - r0))
    rank = np.arange(len(rr)) - first[rr]
    keep = rank < k
    ids[rr[keep] + r0, rank[keep]] = cc[keep]
    scores[rr[keep] + r0, rank[keep]] = ss[keep]
    counts[r0:r1] = np.minimum(np.bincount(rr, minlength=r1 - r0), k)


def similarity_csr(ids, scores, counts, K):
    """The items x items CSR the reference's model stores: K slots per row (unused ones (0, 0, 0.0)), then .tocsr()."""
    n = len(counts)
    keep = np.arange(K)[None, :] < counts[:, None]
    rows = np.where(keep, np.arange(n)[:, None], 0).ravel()
    cols = np.where(keep, ids[:, :K], 0).ravel()
    vals = np.where(keep, scores[:, :K], 0.0).ravel()
    return sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()


def fit_similarity(weighted, K):
    """similarity of a model fitted on the weighted users x items matrix `weighted`."""
    users = sp.csr_matrix(weighted)
    items = users.T.tocsr()
    return similarity_csr(*product_topk(items, users, K), K)


def tie_tolerant_equal(ids_a, sc_a, ids_b, sc_b, rtol=1e-12):
    """Two ranked lists of one row agree: same length, scores within rtol of the row's largest magnitude, and ids equal
    except inside a run of items whose scores tie the last kept score (the reference keeps tied items by visit order)."""
    if len(ids_a) != len(ids_b):
        return False
    if not len(ids_a):
        return True
    scale = max(np.abs(sc_a).max(), np.abs(sc_b).max(), 1e-300)
    if not np.all(np.abs(sc_a - sc_b) <= rtol * scale):
        return False
    diff = set(ids_a.tolist()) ^ set(ids_b.tolist())
    if not diff:
        return True
    kth = min(sc_a[-1], sc_b[-1])
    score_of = dict(zip(ids_a.tolist(), sc_a.tolist()))
    score_of.update(zip(ids_b.tolist(), sc_b.tolist()))
    return all(abs(score_of[i] - kth) <= rtol * scale for i in diff)
