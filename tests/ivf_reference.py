"""Float64 numpy restatement of the IVF-Flat index, written from its specification: spherical
k-means from given initial rows, the inverted lists, and the probed search.  Orders are total: (score desc, id desc)."""
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
