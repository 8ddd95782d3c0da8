"""Float64 numpy restatement of the IVF-Flat index, written from its specification: spherical
k-means from given initial rows, the inverted lists, and the probed search.  Orders are total: (score desc, id desc).
The exact_* functions at the end restate the `iterations = 0` build and the search in integers, for inputs that have one answer."""
import numpy as np


def order_desc(scores):
    """Indices of a 1-d score array under (score desc, index desc)."""
    n = len(scores)
    return np.lexsort((-np.arange(n), -np.asarray(scores, dtype=np.float64)))


def argmax_rows(scores):
    """Per row the column of the largest score, ties to the larger column."""
    n = scores.shape[1]
    return n - 1 - np.argmax(scores[:, ::-1], axis=1)


def normalise_rows(x):
    """Unit rows; a zero row stays zero."""
    x = np.asarray(x, dtype=np.float64)
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)


def build_lists(assign, nlist):
    """(offsets[nlist + 1], ids[n]): list l = ids[offsets[l]:offsets[l + 1]], ascending."""
    assign = np.asarray(assign)
    ids = np.argsort(assign, kind="stable").astype(np.int32)
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    np.cumsum(np.bincount(assign, minlength=nlist), out=offsets[1:])
    return offsets, ids


def assign_margin(scores):
    """Per row: best minus second-best score (inf with one column)."""
    if scores.shape[1] < 2:
        return np.full(scores.shape[0], np.inf)
    part = np.partition(scores, scores.shape[1] - 2, axis=1)
    return part[:, -1] - part[:, -2]


def kmeans(vectors, init_rows, iterations, history=None):
    """Returns (centroids float64 [nlist x f], assign [n]): `iterations` rounds of (assign, mean of each list in ascending
    id, normalise; an empty list or a zero mean keeps its centroid), then the assignment against the final centroids.
    history (a list): receives every round's (assign, margin) including the last."""
    v = np.asarray(vectors, dtype=np.float64)
    cent = normalise_rows(v[np.asarray(init_rows)])
    nlist = len(cent)
    for it in range(iterations + 1):
        scores = v @ cent.T
        assign = argmax_rows(scores)
        if history is not None:
            history.append((assign.copy(), assign_margin(scores)))
        if it == iterations:
            return cent, assign
        sums = np.zeros_like(cent)
        np.add.at(sums, assign, v)  # unbuffered, in ascending vector id
        counts = np.bincount(assign, minlength=nlist)
        for l in range(nlist):
            if counts[l] == 0:
                continue
            mean = sums[l] / counts[l]
            norm = np.sqrt(mean @ mean)
            if norm > 0:
                cent[l] = mean / norm


def topk_candidates(scores, ids, k):
    """The k best of (scores, ids) under (score desc, id desc), padded with (-1, -FLT_MAX)."""
    out_ids = np.full(k, -1, dtype=np.int64)
    out_scores = np.full(k, -np.finfo(np.float32).max, dtype=np.float64)
    order = np.lexsort((-np.asarray(ids, dtype=np.int64), -np.asarray(scores, dtype=np.float64)))[:k]
    out_ids[:len(order)] = np.asarray(ids)[order]
    out_scores[:len(order)] = np.asarray(scores)[order]
    return out_ids, out_scores


def search(centroids, offsets, ids, vectors, queries, k, nprobe, probes=None):
    """(probes [q x P], top ids [q x k], top scores [q x k]) with P = min(nprobe, nlist): per query the P centroids of
    largest inner product, then the k best vectors of those lists.  `probes` given: scan those lists instead."""
    cent = np.asarray(centroids, dtype=np.float64)
    v = np.asarray(vectors, dtype=np.float64)
    q = np.asarray(queries, dtype=np.float64)
    P = min(nprobe, len(cent))
    if probes is None:
        coarse = q @ cent.T
        probes = np.stack([order_desc(row)[:P] for row in coarse]) if len(q) else np.zeros((0, P), dtype=np.int64)
    out_ids = np.empty((len(q), k), dtype=np.int64)
    out_scores = np.empty((len(q), k), dtype=np.float64)
    for r in range(len(q)):
        members = np.concatenate([ids[offsets[l]:offsets[l + 1]] for l in probes[r]]) if P else np.zeros(0, dtype=np.int64)
        out_ids[r], out_scores[r] = topk_candidates(v[members] @ q[r], members, k)
    return np.asarray(probes), out_ids, out_scores


def brute_force(vectors, queries, k):
    v = np.asarray(vectors, dtype=np.float64)
    q = np.asarray(queries, dtype=np.float64)
    everyone = np.arange(len(v))
    out = [topk_candidates(v @ row, everyone, k) for row in q]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def audit(got_ids, want_ids, want_scores, score_of, f):
    """The near-tie rule of smoke(): where an id differs from the float64 result, the float64 score of the id that was
    returned (score_of(row, id)) must equal the expected score at that position within 4 f 2^-23 relative.  Returns the
    number of such exceptions; raises AssertionError for anything else."""
    got_ids, want_ids = np.asarray(got_ids), np.asarray(want_ids)
    assert got_ids.shape == want_ids.shape
    tol = 4 * f * float(np.finfo(np.float32).eps)
    exceptions = 0
    for pos in zip(*np.nonzero(got_ids != want_ids)):
        r = pos[0]
        assert got_ids[pos] >= 0 and want_ids[pos] >= 0, f"row {r}: a filled position against an empty one at {pos}"
        exact = score_of(r, got_ids[pos])
        want = want_scores[pos]
        assert abs(exact - want) <= tol * max(abs(want), 1e-30), f"id at {pos} differs and is not a near-tie ({exact} vs {want})"
        exceptions += 1
    return exceptions


# ---- exact restatements ------------------------------------------------------------------------------------------------
# Integer-valued vectors and queries whose scores stay below 2^24 have one possible fp32 score in any summation order, and
# an `iterations = 0` build whose initial rows are zero or +-2^m e_j has the centroids 0 / +-e_j exactly (the sum of squares
# 4^m, its square root and the division are exact).  Everything below is integer arithmetic on such inputs: one answer,
# compared with array_equal.
def exact_centroids(vectors, init_rows):
    """(coord[nlist], sign[nlist]): centroid c is sign[c] * e_coord[c] (sign 0: the zero centroid of a zero row)."""
    rows = np.asarray(vectors)[np.asarray(init_rows)].astype(np.int64)
    assert ((rows != 0).sum(axis=1) <= 1).all(), "an initial row is not one-hot"
    coord = np.abs(rows).argmax(axis=1)
    value = rows[np.arange(len(rows)), coord]
    mag = np.abs(value)
    assert ((mag & (mag - 1)) == 0).all(), "an initial row's entry is not a power of two"
    return coord, np.sign(value)


def exact_centroid_matrix(coord, sign, f):
    cent = np.zeros((len(coord), f), dtype=np.float32)
    cent[np.arange(len(coord)), coord] = sign
    return cent


def exact_build(vectors, init_rows):
    """(coord, sign, assign[n], offsets[nlist + 1], ids[n]) of the iterations = 0 build: a vector's score against list c is
    sign[c] * v[coord[c]], ties go to the larger list id, ids ascend inside a list."""
    v = np.asarray(vectors).astype(np.int64)
    coord, sign = exact_centroids(v, init_rows)
    assign = argmax_rows(v[:, coord] * sign)
    offsets, ids = build_lists(assign, len(coord))
    return coord, sign, assign, offsets, ids


def exact_scores(vectors, queries):
    """queries x vectors int64 inner products.  The product runs in float64, where sums of integers below 2^53 are exact in
    any order; the result is checked to be integral and below 2^24 (exact in fp32 too)."""
    s = np.asarray(queries, dtype=np.float64) @ np.asarray(vectors, dtype=np.float64).T
    assert (s == np.rint(s)).all() and (np.abs(s) < 2.0 ** 24).all()
    return s.astype(np.int64)


def exact_probes(coord, sign, queries, nprobe):
    """queries x min(nprobe, nlist) list ids under (coarse score desc, list id desc); the coarse score is sign * q[coord]."""
    q = np.asarray(queries).astype(np.int64)
    nlist = len(coord)
    key = q[:, coord] * sign * nlist + np.arange(nlist)  # distinct per row: one order
    return np.argsort(-key, axis=1, kind="stable")[:, :min(nprobe, nlist)]


def exact_search(coord, sign, assign, vectors, queries, k, nprobe, probes=None):
    """(probes, ids [q x k] int64, scores [q x k] float64): the k best vectors of the probed lists under (score desc, id
    desc), holes (-1, -FLT_MAX).  Vectorised over the queries.  `probes` given: scan those lists."""
    v = np.asarray(vectors)
    n, nlist, nq = len(v), len(coord), len(queries)
    if probes is None:
        probes = exact_probes(coord, sign, queries, nprobe)
    probes = np.asarray(probes)
    probed = np.zeros((nq, nlist), dtype=bool)
    np.put_along_axis(probed, probes.astype(np.int64), True, axis=1)
    hole = -(1 << 62)  # below every key: |score * n + id| < 2^24 * 2^31
    key = np.where(probed[:, np.asarray(assign)], exact_scores(v, queries) * n + np.arange(n), hole)
    kk = min(k, n)
    if kk < n:  # the kk largest keys of every row, then only those sorted
        key = np.take_along_axis(key, np.argpartition(-key, kk - 1, axis=1)[:, :kk], axis=1)
    pkey = -np.sort(-key, axis=1)
    out_ids = np.full((nq, k), -1, dtype=np.int64)
    out_scores = np.full((nq, k), -float(np.finfo(np.float32).max))
    filled = pkey != hole
    out_ids[:, :kk][filled] = (pkey % n)[filled]
    out_scores[:, :kk][filled] = (pkey // n)[filled]
    return probes, out_ids, out_scores
