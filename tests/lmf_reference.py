"""Host restatements of the LMF contract (csrc/lmf.hip), written from its equations, for the LMF tests.

negative_count: K per row.  negative_positions: the Philox positions of a row's negatives.  half_sweep64: one half-sweep
in float64, with an element-wise bound on what an fp32 evaluation may differ by.  serial_fit: the whole fit in float64
over the device's draws.  init_factors: the initial factors of implicit/cpu/lmf.pyx's fit.
"""
import numpy as np

from bpr_reference import philox4x32_10

_TAG_LMF = 3
EPS32 = float(np.finfo(np.float32).eps)


def negative_count(n, C, neg_prop):
    """K = min(C, n * neg_prop): the reference caps with item_vectors.shape[1], the column count."""
    return np.minimum(np.int64(C), np.asarray(n, dtype=np.int64) * np.int64(neg_prop))


def negative_positions(seed, nnz, rows, ks):
    """Positions in [0, nnz) of negatives ks of rows (arrays of equal length): word (k mod 4) of Philox4x32-10 at counter
    (k / 4, row, 0, 3), key (seed_lo, seed_hi), scaled as (w * nnz) >> 32."""
    ks = np.asarray(ks, dtype=np.uint64)
    rows = np.asarray(rows, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = np.stack(philox4x32_10(ks >> np.uint64(2), rows, 0, _TAG_LMF, seed & 0xFFFFFFFF, seed >> 32))
    w = words[(ks & np.uint64(3)).astype(np.int64), np.arange(len(ks))].astype(np.uint64)
    return ((w * np.uint64(nnz)) >> np.uint64(32)).astype(np.int64)


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    pos = x >= 0
    out[pos] = 1.0 / (1.0 + np.exp(-x[pos]))
    z = np.exp(x[~pos])
    out[~pos] = z / (1.0 + z)
    return out


def _entries(m, neg_prop, seed, C):
    """(row, col, weight, is_negative) of every term of a half-sweep over the CSR m."""
    n = np.diff(m.indptr).astype(np.int64)
    prow = np.repeat(np.arange(m.shape[0], dtype=np.int64), n)
    K = negative_count(n, C, neg_prop) * (n > 0)
    nrow = np.repeat(np.arange(m.shape[0], dtype=np.int64), K)
    ks = np.arange(K.sum(), dtype=np.int64) - np.repeat(np.cumsum(K) - K, K)
    ncol = np.asarray(m.indices, dtype=np.int64)[negative_positions(seed, m.nnz, nrow, ks)] if len(nrow) else nrow
    rows = np.concatenate([prow, nrow])
    cols = np.concatenate([np.asarray(m.indices, dtype=np.int64), ncol])
    w = np.concatenate([np.asarray(m.data, dtype=np.float64), np.ones(len(nrow))])
    neg = np.concatenate([np.zeros(len(prow), bool), np.ones(len(nrow), bool)])
    return rows, cols, w, neg, n, K


def half_sweep64(m, X, Y, G, lr, reg, neg_prop, seed, one_col=-1):
    """One half-sweep in float64 from (X, Y, G) (not modified); returns (X1, G1, bound_X, bound_G): the bounds are what an
    fp32 evaluation in any summation order may differ from X1 / G1 by, element-wise, built from the fp32 summation bound of
    d (|terms| summed) and the Adagrad step's sensitivity to d."""
    X, Y, G = (np.asarray(a, dtype=np.float64) for a in (X, Y, G))
    rows_n, C = X.shape
    rows, cols, w, neg, n, K = _entries(m, neg_prop, seed, C)
    s = np.einsum("ij,ij->i", X[rows], Y[cols])
    dot_abs = np.einsum("ij,ij->i", np.abs(X[rows]), np.abs(Y[cols]))
    coef = np.where(neg, -sigmoid(s), w * sigmoid(-s))
    terms = coef[:, None] * Y[cols]
    d = np.zeros((rows_n, C))
    np.add.at(d, rows, terms)
    d -= reg * X
    # fp32 error of d: the summation (depth <= n + K + 1 terms per row) over sum |terms|, plus each coefficient's error
    # (sigma moves by at most a quarter of the dot product's error, C eps sum |x y|, and a few eps of its own)
    S = np.zeros((rows_n, C))
    np.add.at(S, rows, np.abs(terms))
    S += np.abs(reg * X)
    coef_err = np.abs(w) * (0.25 * C * dot_abs + 4.0) * EPS32
    T = np.zeros((rows_n, C))
    np.add.at(T, rows, coef_err[:, None] * np.abs(Y[cols]))
    err_d = EPS32 * (n + K + 2)[:, None] * S + T

    touched = n > 0
    G1 = G.copy()
    G1[touched] += d[touched] ** 2
    a = 1e-6 + G[touched]
    X1 = X.copy()
    X1[touched] += lr * d[touched] / np.sqrt(a + d[touched] ** 2)
    if one_col >= 0:
        X1[:, one_col] = 1.0
    # the step lr d / sqrt(a + d^2) has slope lr a / (a + d^2)^1.5, largest where |d| is smallest
    dmin = np.maximum(np.abs(d[touched]) - err_d[touched], 0.0)
    bound_X = np.zeros_like(X1)
    bound_X[touched] = lr * a / (a + dmin**2) ** 1.5 * err_d[touched] + 4 * EPS32 * (np.abs(X[touched]) + abs(lr))
    bound_G = np.zeros_like(G1)
    bound_G[touched] = (2 * np.abs(d[touched]) + err_d[touched]) * err_d[touched] + 2 * EPS32 * G1[touched]
    return X1, G1, bound_X, bound_G


def within(got, want, bound, factor=2.0):
    """Element-wise |got - want| <= factor * bound (+ a denormal floor); returns the worst ratio for the message."""
    diff = np.abs(np.asarray(got, dtype=np.float64) - want)
    lim = factor * bound + 1e-30
    return bool((diff <= lim).all()), float((diff / lim).max()) if diff.size else 0.0


def serial_fit(m, X0, Y0, seeds, lr, reg, neg_prop):
    """The fit in float64 over the device's draws: per epoch the user half (seeds[2e], one_col C-2), then the item half
    (seeds[2e + 1], one_col C-1), accumulators from zero; returns X, Y."""
    from scipy.sparse import csr_matrix

    m = csr_matrix(m, dtype=np.float32)
    m.sort_indices()
    mt = m.T.tocsr()
    mt.sort_indices()
    X, Y = X0.astype(np.float64), Y0.astype(np.float64)
    C = X.shape[1]
    GX, GY = np.zeros_like(X), np.zeros_like(Y)
    for e in range(len(seeds) // 2):
        X, GX, _, _ = half_sweep64(m, X, Y, GX, lr, reg, neg_prop, seeds[2 * e], C - 2)
        Y, GY, _, _ = half_sweep64(mt, Y, X, GY, lr, reg, neg_prop, seeds[2 * e + 1], C - 1)
    return X, Y


def init_factors(m, factors, random_state):
    """implicit/cpu/lmf.pyx fit with a numpy Generator: items first, then users; returns (X, Y, rng after the draws)."""
    rs = np.random.default_rng(random_state)
    users, items = m.shape
    C = factors + 2
    Y = rs.standard_normal(size=(items, C), dtype=np.float32)
    Y[:, -1] = 1.0
    Y[np.bincount(m.indices, minlength=items) == 0] = np.zeros(C)
    X = rs.standard_normal(size=(users, C), dtype=np.float32)
    X[:, -2] = 1.0
    X[np.diff(m.indptr) == 0] = np.zeros(C)
    return X, Y, rs
