"""Host restatements of the WARP contract (csrc/warp.hip), written from its equations, for the WARP tests.

positives: the (u, i) of a call's samples.  candidates: the items a sample draws, in trial order.  weight: the rank
estimate's weight L.  step64: one sample in float64.  serial_epochs: the whole serial SGD over the device's draws (and its closest margin).
"""
import math

import numpy as np

from bpr_reference import coo_ids, philox4x32_10

_TAG_WARP = 4


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def positions(seed, nnz, samples, first=0):
    """lp of samples first .. first + samples - 1 of a call with this seed."""
    s = np.arange(first, first + samples, dtype=np.uint64)
    r = philox4x32_10(s & np.uint64(0xFFFFFFFF), s >> np.uint64(32), 0, _TAG_WARP, *_key(seed))
    return ((r[0].astype(np.uint64) * np.uint64(nnz)) >> np.uint64(32)).astype(np.int64)


def positives(m, seed, samples=None):
    userids, itemids = coo_ids(m)
    lp = positions(seed, m.nnz, m.nnz if samples is None else samples)
    return userids[lp], itemids[lp]


def candidates(seed, s, items, max_sampled):
    """The items sample s draws in trials 1 .. max_sampled (int64 array)."""
    blocks = (max_sampled + 3) // 4
    r = philox4x32_10(int(s) & 0xFFFFFFFF, int(s) >> 32, 1 + np.arange(blocks, dtype=np.uint64), _TAG_WARP, *_key(seed))
    words = np.stack(r, axis=1).ravel()[:max_sampled]  # word (t-1) & 3 of block (t-1) >> 2
    return ((words.astype(np.uint64) * np.uint64(items)) >> np.uint64(32)).astype(np.int64)


def weight(items, t):
    return min(10.0, math.log(max(1, (items - 1) // t)))


def step64(X, Y, row, u, i, cand, lr, reg):
    """One sample applied in float64 to float64 copies X, Y (in place).  `row`: the set of items user u liked, `cand`: the
    sample's candidates.  Returns (t of the violating trial or None, trials consumed, the closest margin |sn - sp + 1| over the
    examined trials, inf when none was examined).  The examined candidates are those of cand[:trials] outside `row`."""
    x, p = X[u].copy(), Y[i].copy()
    sp = float(x @ p)
    scores = (Y[cand] @ x).tolist()
    closest = math.inf
    for t, j in enumerate(cand.tolist(), start=1):
        if j in row:
            continue
        sn = scores[t - 1]
        closest = min(closest, abs(sn - sp + 1.0))
        if sn > sp - 1.0:
            q = Y[j].copy()
            L = weight(Y.shape[0], t)
            f = X.shape[1] - 1
            X[u, :f] = x[:f] + lr * (L * (p[:f] - q[:f]) - reg * x[:f])
            Y[i, :f] = p[:f] + lr * (L * x[:f] - reg * p[:f])
            Y[j, :f] = q[:f] + lr * (-L * x[:f] - reg * q[:f])
            Y[i, f] = p[f] + lr * (L - reg * p[f])
            Y[j, f] = q[f] + lr * (-L - reg * q[f])
            return t, t, closest
    return None, len(cand), closest


def liked_sets(m):
    return [set(m.indices[m.indptr[u]:m.indptr[u + 1]].tolist()) for u in range(m.shape[0])]


def serial_epochs(m, X0, Y0, seeds, lr, reg, max_sampled, with_margin=False):
    """The serial SGD over the device's draws, float64; returns X, Y and the per-epoch (satisfied, trials), and with
    `with_margin` also the closest margin |sn - sp + 1| over every examined trial of every epoch."""
    X, Y = X0.astype(np.float64), Y0.astype(np.float64)
    rows = liked_sets(m)
    items = m.shape[1]
    counts, closest = [], math.inf
    blocks = (max_sampled + 3) // 4
    for seed in seeds:
        us, iis = positives(m, seed)
        # every sample's candidates at once: block b of sample s is Philox(counter (s, 0, 1 + b, 4))
        s = np.arange(m.nnz, dtype=np.uint64)
        words = np.stack([w for b in range(blocks) for w in philox4x32_10(s, 0, 1 + b, _TAG_WARP, *_key(seed))], axis=1)
        cands = ((words[:, :max_sampled].astype(np.uint64) * np.uint64(items)) >> np.uint64(32)).astype(np.int64)
        satisfied = trials = 0
        for k, (u, i) in enumerate(zip(us.tolist(), iis.tolist())):
            t, used, margin = step64(X, Y, rows[u], u, i, cands[k], lr, reg)
            satisfied += t is None
            trials += used
            closest = min(closest, margin)
        counts.append((satisfied, trials))
    return (X, Y, counts, closest) if with_margin else (X, Y, counts)
