"""Host restatements of the BPR contract (csrc/bpr.hip), written from its equations, for the BPR tests.

philox4x32_10: vectorised numpy Philox4x32-10.  sample_ids: the (u, i, j) triples of a call.  predicted_skipped: its
skipped count.  step64: one sample in float64.  serial_epochs: the whole serial SGD (the reference CPU loop's order with
the device's draws).  init_factors: the initial factors of implicit/gpu/bpr.py:99-128.
"""
import numpy as np

_MASK = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_TAG_BPR = 2


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Random123's philox4x32 with 10 rounds; arguments are uint32 scalars or arrays, returns four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def sample_positions(seed, nnz, samples, first=0):
    """(lp, dp) of samples first .. first + samples - 1 of a call with this seed."""
    s = np.arange(first, first + samples, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10(s & _MASK, s >> np.uint64(32), 0, _TAG_BPR, seed & 0xFFFFFFFF, seed >> 32)
    n = np.uint64(nnz)
    lp = (r[0].astype(np.uint64) * n) >> np.uint64(32)
    dp = (r[1].astype(np.uint64) * n) >> np.uint64(32)
    return lp.astype(np.int64), dp.astype(np.int64)


def coo_ids(m):
    """userids, itemids (int32) of a CSR matrix, in storage order."""
    return np.repeat(np.arange(m.shape[0], dtype=np.int32), np.diff(m.indptr)), np.asarray(m.indices, dtype=np.int32)


def sample_ids(m, seed, samples=None):
    userids, itemids = coo_ids(m)
    lp, dp = sample_positions(seed, m.nnz, m.nnz if samples is None else samples)
    return userids[lp], itemids[lp], itemids[dp]


def liked(m, u, j):
    """Vectorised membership of item j in row u (rows of m sorted)."""
    items = m.shape[1]
    keys = np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(m.indptr)) * items + m.indices
    q = np.asarray(u, dtype=np.int64) * items + np.asarray(j, dtype=np.int64)
    pos = np.minimum(np.searchsorted(keys, q), max(len(keys) - 1, 0))
    return (keys[pos] == q) if len(keys) else np.zeros(len(q), dtype=bool)


def predicted_skipped(m, seed, verify, samples=None):
    if not verify:
        return 0
    u, _, j = sample_ids(m, seed, samples)
    return int(liked(m, u, j).sum())


def step64(X, Y, u, i, j, lr, reg):
    """One sample applied in float64 to float64 copies X, Y (in place); returns the score."""
    C = X.shape[1]
    x, p, q = X[u].copy(), Y[i].copy(), Y[j].copy()
    score = float(x @ (p - q))
    z = 1.0 / (1.0 + np.exp(score))
    f = C - 1
    X[u, :f] = x[:f] + lr * (z * (p[:f] - q[:f]) - reg * x[:f])
    Y[i, :f] = p[:f] + lr * (z * x[:f] - reg * p[:f])
    Y[i, f] = p[f] + lr * (z - reg * p[f])
    qb = Y[j].copy()  # the value the i update produced when i == j
    Y[j, :f] = qb[:f] + lr * (-z * x[:f] - reg * qb[:f])
    Y[j, f] = qb[f] + lr * (-z - reg * qb[f])
    return score


def serial_epochs(m, X0, Y0, seeds, lr, reg, verify):
    """The serial SGD over the device's draws, float64; returns X, Y and the per-epoch (correct, skipped)."""
    X, Y = X0.astype(np.float64), Y0.astype(np.float64)
    userids, itemids = coo_ids(m)
    counts = []
    for seed in seeds:
        lp, dp = sample_positions(seed, m.nnz, m.nnz)
        us, iis, js = userids[lp], itemids[lp], itemids[dp]
        skip = liked(m, us, js) if verify else np.zeros(len(us), dtype=bool)
        correct = 0
        for u, i, j, sk in zip(us.tolist(), iis.tolist(), js.tolist(), skip.tolist()):
            if sk:
                continue
            correct += step64(X, Y, u, i, j, lr, reg) > 0
        counts.append((correct, int(skip.sum())))
    return X, Y, counts


def init_factors(m, factors, random_state):
    """implicit/gpu/bpr.py:99-128 with a numpy Generator: items first, then users; returns (X, Y, rng after the draws)."""
    rs = np.random.default_rng(random_state)
    users, items = m.shape
    Y = rs.random((items, factors + 1), "float32") - 0.5
    Y /= factors
    Y[np.bincount(m.indices, minlength=items) == 0] = np.zeros(factors + 1)
    X = rs.random((users, factors + 1), "float32") - 0.5
    X /= factors
    X[np.diff(m.indptr) == 0] = np.zeros(factors + 1)
    X[:, factors] = 1.0
    return X, Y, rs
