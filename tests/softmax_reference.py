"""Host restatement of the sampled-softmax contract (csrc/softmax_mf.hip), written from its equations.  positives: the (u, i)
of a call's samples.  negatives: the items batch b shares.  serial: the serial mini-batch SGD over the device's draws, in
float64 or, for the tests' tolerances, in float32."""
import numpy as np

from bpr_reference import coo_ids, philox4x32_10

_TAG = 6
BATCH = 64


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def positives(m, seed, samples):
    userids, itemids = coo_ids(m)
    s = np.arange(samples, dtype=np.uint64)
    r = philox4x32_10(s & np.uint64(0xFFFFFFFF), s >> np.uint64(32), 0, _TAG, *_key(seed))
    lp = ((r[0].astype(np.uint64) * np.uint64(m.nnz)) >> np.uint64(32)).astype(np.int64)
    return userids[lp], itemids[lp]


def negatives(seed, b, items, N):
    r = philox4x32_10(int(b) & 0xFFFFFFFF, int(b) >> 32, 1 + np.arange(N // 4, dtype=np.uint64), _TAG, *_key(seed))
    words = np.stack(r, axis=1).ravel()
    return ((words.astype(np.uint64) * np.uint64(items)) >> np.uint64(32)).astype(np.int64)


def serial(m, X0, Y0, seed, lr, reg, N, samples=None, dtype=np.float64):
    """One call applied batch after batch to copies of X0, Y0 in `dtype`.  Returns X, Y, correct, masked and the smallest
    |z_r - max unmasked z_rn| met (inf when every row masked everything)."""
    X, Y = X0.astype(dtype), Y0.astype(dtype)
    liked = m.toarray() != 0
    f = X.shape[1] - 1
    samples = m.nnz if samples is None else samples
    all_us, all_is = positives(m, seed, samples)
    correct, masked, closest = 0, 0, np.inf
    for b in range((samples + BATCH - 1) // BATCH):
        us, iis = all_us[b * BATCH:(b + 1) * BATCH], all_is[b * BATCH:(b + 1) * BATCH]
        js = negatives(seed, b, m.shape[1], N)
        M = liked[us[:, None], js[None, :]]
        U, Q, V = X[us], Y[iis], Y[js]
        z = (U * Q).sum(axis=1)
        Z = np.where(M, -np.inf, U @ V.T)
        top = Z.max(axis=1)
        mx = np.maximum(z, top)
        e, ez = np.exp(Z - mx[:, None]), np.exp(z - mx)
        total = ez + e.sum(axis=1)
        P, g = e / total[:, None], 1 - ez / total
        correct, masked, closest = correct + int((z > top).sum()), masked + int(M.sum()), min(closest, float(np.abs(z - top).min()))
        dX = lr * (g[:, None] * Q - P @ V - reg * U)
        dX[:, f] = 0
        dQ = lr * (g[:, None] * U - reg * Q)
        dQ[:, f] = lr * (g - reg * Q[:, f])
        dV = lr * (-(P.T @ U) - reg * V)
        dV[:, f] = lr * (-P.sum(axis=0) - reg * V[:, f])
        for A, rows, d in ((X, us, dX), (Y, iis, dQ), (Y, js, dV)):
            np.add.at(A, rows, d)
    return X, Y, correct, masked, closest
