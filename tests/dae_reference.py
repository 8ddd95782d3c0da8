"""Host restatement of the Mult-DAE contract (csrc/mult_dae.hip), written from its equations with dense matrices.  dtype is
float64, or float32 for the tests' tolerances: then every operand and every intermediate is float32 and every product is the
chain the contract documents -- one accumulator per entry, the inner index ascending (the k-ordered chain of the matrix
instruction; stored order in the encoder) -- instead of numpy's blocked matmul."""
import numpy as np

from bpr_reference import philox4x32_10

_TAG = 7


def keep_mask(m, seed, dropout):
    """The Bernoulli(1 - dropout) keep mask of every stored entry, by CSR position."""
    if dropout <= 0:
        return np.ones(m.nnz, dtype=bool)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10(np.arange(m.nnz, dtype=np.uint64), 0, 0, _TAG, seed & 0xFFFFFFFF, seed >> 32)
    return (r[0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0**-24) >= np.float32(dropout)


def _mm(A, B):
    """A @ B; in float32 as one sequential chain over the inner index."""
    if A.dtype == np.float64:
        return A @ B
    out = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k in range(A.shape[1]):
        out += A[:, k:k + 1] * B[k:k + 1]
    return out


def _inputs(m, rows, seed, dropout, dtype):
    """Dense X (the undropped rows) and X~ (kept entries, scaled) of a batch; row id -1 is an empty row."""
    B, items = len(rows), m.shape[1]
    X, Xs = np.zeros((B, items), dtype=dtype), np.zeros((B, items), dtype=dtype)
    keep = keep_mask(m, seed, dropout)
    for r, u in enumerate(rows):
        if u < 0 or m.indptr[u] == m.indptr[u + 1]:
            continue
        lo, hi = m.indptr[u], m.indptr[u + 1]
        s = dtype(1) / (dtype(1 - dtype(dropout)) * np.sqrt(dtype(hi - lo)))
        X[r, m.indices[lo:hi]] = 1
        Xs[r, m.indices[lo:hi]] = np.where(keep[lo:hi], s, dtype(0))
    return X, Xs


def encode(m, rows, W_in, b_in, dtype=np.float64):
    """[h, 1] of the rows, without dropout."""
    Xs = _inputs(m, rows, 0, 0.0, dtype)[1]
    h = np.tanh(b_in.astype(dtype) + _mm(Xs, W_in.astype(dtype)))
    return np.concatenate([h, np.ones((len(rows), 1), dtype=dtype)], axis=1)


def gradients(m, rows, W_in, b_in, W_out, dropout=0.0, seed=0, dtype=np.float64):
    """dict of loss, dW_in, db_in, dW_out, dh, dz, and the logits and g of the batch."""
    W_in, b_in, W_out = (a.astype(dtype) for a in (W_in, b_in, W_out))
    B, H = len(rows), W_in.shape[1]
    X, Xs = _inputs(m, rows, seed, dropout, dtype)
    h = np.tanh(b_in + _mm(Xs, W_in))
    logits = _mm(h, np.ascontiguousarray(W_out[:, :H].T)) + W_out[:, H]
    top = logits.max(axis=1, keepdims=True)
    lse = top + np.log(np.exp(logits - top).sum(axis=1, keepdims=True))
    n = X.sum(axis=1, keepdims=True)
    per_row = n * lse - _mm(X * logits, np.ones((X.shape[1], 1), dtype=dtype))  # the contract's order: row by row, then the rows
    loss = _mm(np.ones((1, B), dtype=dtype), per_row)[0, 0] / dtype(B)
    g = (n * np.exp(logits - lse) - X) / dtype(B)
    dh = _mm(g, W_out[:, :H])
    dz = dh * (1 - h * h)
    dW_out = np.concatenate([_mm(g.T, h), _mm(g.T, np.ones((B, 1), dtype=dtype))], axis=1)
    return dict(loss=loss, dW_in=_mm(Xs.T, dz), db_in=_mm(np.ones((1, B), dtype=dtype), dz), dW_out=dW_out, dh=dh, dz=dz, logits=logits, g=g)


def adam_step(m, rows, params, moments, dropout, seed, lr, step, reg=0.0, b1=0.9, b2=0.999, eps=1e-8, dtype=np.float64):
    """One step on params = (W_in, b_in, W_out), moments = (m, v) per parameter in that order; returns (loss, params, moments)."""
    params, moments = [p.astype(dtype) for p in params], [a.astype(dtype) for a in moments]
    H = params[0].shape[1]
    out = gradients(m, rows, *params, dropout, seed, dtype)
    c1, c2 = dtype(1 / (1 - float(b1) ** step)), dtype(1 / (1 - float(b2) ** step))
    lr, b1, b2, eps, reg = (dtype(x) for x in (lr, b1, b2, eps, reg))
    for i, name in enumerate(("dW_in", "db_in", "dW_out")):
        g = out[name].copy()
        if name != "db_in":
            g[:, :H] += reg * params[i][:, :H]
        moments[2 * i] = b1 * moments[2 * i] + (1 - b1) * g
        moments[2 * i + 1] = b2 * moments[2 * i + 1] + (1 - b2) * (g * g)
        params[i] = params[i] - lr * (moments[2 * i] * c1) / (np.sqrt(moments[2 * i + 1] * c2) + eps)
    return out["loss"], params, moments
