"""Float64 restatement of the hybrid WARP contract (csrc/hybrid_warp.hip), written from its equations, for the hybrid tests.

represent: a row's representation.  step64: one sample, with the scatters in the contract's order -- the user's, the
positive's, then the negative's ON WHAT THE POSITIVE'S LEFT, so a feature both items share receives both steps.  positives /
candidates: warp_reference's draws under Philox tag 5.  serial_epochs: the whole serial SGD over the device's draws.
"""
import contextlib
import math

import numpy as np

import warp_reference as wref

TAG = 5


@contextlib.contextmanager
def _tagged():
    old, wref._TAG_WARP = wref._TAG_WARP, TAG
    try:
        yield
    finally:
        wref._TAG_WARP = old


def positives(m, seed, samples=None):
    with _tagged():
        return wref.positives(m, seed, samples)


def candidates(seed, s, items, max_sampled):
    with _tagged():
        return wref.candidates(seed, s, items, max_sampled)


def feature_row(F, r):
    """(ids, float64 weights) of row r of a CSR feature matrix."""
    a, b = F.indptr[r], F.indptr[r + 1]
    return F.indices[a:b], F.data[a:b].astype(np.float64)


def represent(F, E, r):
    ids, w = feature_row(F, r)
    return w @ E[ids]  # zeros for an empty row


def _scatter(E, ids, w, g, cols, lr, reg):
    E[ids, :cols] += lr * (np.outer(w, g[:cols]) - reg * E[ids, :cols])  # no repeated id within a row


def step64(EU, EI, UF, IF, row, u, i, cand, lr, reg):
    """One sample applied in float64 to float64 EU, EI (in place).  Returns what warp_reference.step64 returns: (t of the
    violating trial or None, trials consumed, the closest margin over the examined trials)."""
    C = EI.shape[1]
    x = represent(UF, EU, u)
    x[C - 1] = 1.0
    p = represent(IF, EI, i)
    sp, closest = float(x @ p), math.inf
    for t, j in enumerate(cand.tolist(), start=1):
        if j in row:
            continue
        q = represent(IF, EI, j)
        sn = float(x @ q)
        closest = min(closest, abs(sn - sp + 1.0))
        if sn > sp - 1.0:
            L = wref.weight(IF.shape[0], t)
            _scatter(EU, *feature_row(UF, u), L * (p - q), C - 1, lr, reg)
            _scatter(EI, *feature_row(IF, i), L * x, C, lr, reg)
            _scatter(EI, *feature_row(IF, j), -L * x, C, lr, reg)  # after the positive's, re-reading the rows it updates
            return t, t, closest
    return None, len(cand), closest


def serial_epochs(m, UF, IF, EU0, EI0, seeds, lr, reg, max_sampled):
    """The serial SGD over the device's draws, float64; returns EU, EI and the per-epoch (satisfied, trials)."""
    EU, EI = EU0.astype(np.float64), EI0.astype(np.float64)
    rows, counts = wref.liked_sets(m), []
    for seed in seeds:
        us, iis = positives(m, seed)
        satisfied = trials = 0
        for s, (u, i) in enumerate(zip(us.tolist(), iis.tolist())):
            t, used, _ = step64(EU, EI, UF, IF, rows[u], u, i, candidates(seed, s, m.shape[1], max_sampled), lr, reg)
            satisfied, trials = satisfied + (t is None), trials + used
        counts.append((satisfied, trials))
    return EU, EI, counts
