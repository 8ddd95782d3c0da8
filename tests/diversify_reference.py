"""Restatement of KnnQuery.diversify, written from the contract (include/implicit_hip.h on imp_knn_diversify): the greedy DPP
MAP inference as column-pivoted Gram-Schmidt, and maximal marginal relevance, one list at a time in numpy at a chosen dtype."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def greedy(Y, ids, quality, n, rule, param=0.5, min_gain=1e-6, dtype=np.float64):
    """(picked ids, gains, gaps[k] = relative distance of pick k's best value from the second best); ties: larger id, later position."""
    T = np.dtype(dtype).type
    ids = np.asarray(ids)
    y, q = Y[ids].astype(T), np.asarray(quality).astype(T)
    M, w = y.shape
    norm = np.sqrt((y * y).sum(axis=1))[:, None]
    unit = np.divide(y, norm, out=np.zeros_like(y), where=norm > 0)
    alive, pos = np.ones(M, dtype=bool), np.arange(M)
    picks, gains, gaps = [], [], []
    if rule == "dpp":
        B = q[:, None] * unit
        value, U = (B * B).sum(axis=1), np.zeros((0, w), dtype=T)
    else:
        lam, most = T(param), np.zeros(M, dtype=T)
    for k in range(min(n, M)):
        if rule == "mmr":
            value = lam * q - (T(1) - lam) * most
        order = np.lexsort((pos, ids, np.where(alive, value, -np.inf)))
        j = order[-1]
        a, b = float(value[j]), float(value[order[-2]]) if alive.sum() > 1 else -np.inf
        gap = (a - b) / max(abs(a), abs(b), 1e-300) if alive.sum() > 1 else np.inf
        if rule == "dpp":
            if len(U) == w:
                break
            r = B[j].copy()
            for _ in range(2):
                r = r - (U @ r) @ U
            g = (r * r).sum()
            if g <= T(min_gain) * q[j] * q[j]:
                break
            U = np.vstack([U, r / np.sqrt(g)])
            e = B @ U[-1]
            value = value - e * e
        else:
            g = value[j]
            e = unit @ unit[j]
            most = e if k == 0 else np.maximum(most, e)
        alive[j] = False
        picks.append(int(ids[j]))
        gains.append(float(g))
        gaps.append(gap)
    return picks, gains, gaps


def batch(Y, lists, qualities, n, rule, dtype=np.float64, **kw):
    """greedy() per list, shaped as KnnQuery.diversify returns: (ids [B, n], gains [B, n] float64, counts [B], smallest gap)."""
    ids = np.full((len(lists), n), -1, dtype=np.int32)
    gains = np.full((len(lists), n), -FLT_MAX, dtype=np.float64)
    counts, closest = np.zeros(len(lists), dtype=np.int32), np.inf
    for r, (l, q) in enumerate(zip(lists, qualities)):
        p, g, gaps = greedy(Y, l, q, n, rule, dtype=dtype, **kw)
        ids[r, :len(p)], gains[r, :len(p)], counts[r] = p, g, len(p)
        closest = min([closest] + gaps)
    return ids, gains, counts, closest
