"""Host restatement of the Mult-VAE contract (csrc/mult_vae.hip), written from its equations with dense matrices, in the
manner of dae_reference.py whose input stage and chained product it shares.  dtype is float64, or float32 for the tests'
tolerances: then every operand and intermediate is float32 and every product one chain over the ascending inner index.
params = (W_in, b_in, W_lat, b_lat, W_dec, b_dec, W_out) everywhere."""
import numpy as np

from bpr_reference import philox4x32_10
from dae_reference import _inputs, _mm

NAMES = ("dW_in", "db_in", "dW_lat", "db_lat", "dW_dec", "db_dec", "dW_out")
_TAG = 8


def draws(B, L, seed):
    """eps [B x L] in float64 by the contract's rule: u1 and u2 are formed in float32 as written, the rest is exact."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r, l = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(L, dtype=np.uint64), indexing="ij")
    R = philox4x32_10(r, l, 0, _TAG, seed & 0xFFFFFFFF, seed >> 32)
    u1 = ((R[0] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0**-24)
    u2 = (R[1] >> np.uint32(8)).astype(np.float32) * np.float32(2.0**-24)
    return np.sqrt(-2 * np.log(u1.astype(np.float64))) * np.cos(2 * np.pi * u2.astype(np.float64))


def _forward(m, rows, params, dropout, seed, eps, dtype):
    W_in, b_in, W_lat, b_lat, W_dec, b_dec = params[:6]
    L = W_dec.shape[0]
    X, Xs = _inputs(m, rows, seed, dropout, dtype)
    h1 = np.tanh(b_in + _mm(Xs, W_in))
    a = _mm(h1, W_lat) + b_lat
    mu, lv = a[:, :L], a[:, L:]
    sd = np.exp(dtype(0.5) * lv)
    z = mu + eps * sd if eps is not None else mu
    return X, Xs, h1, mu, lv, sd, z, np.tanh(_mm(z, W_dec) + b_dec)


def encode(m, rows, params, dtype=np.float64):
    """[h2, 1] of the rows at z = mu, without dropout."""
    h2 = _forward(m, rows, [p.astype(dtype) for p in params[:6]], 0.0, 0, None, dtype)[-1]
    return np.concatenate([h2, np.ones((len(rows), 1), dtype=dtype)], axis=1)


def gradients(m, rows, params, dropout=0.0, seed=0, beta=0.0, eps=None, dtype=np.float64):
    """dict of nll, kl, the seven gradients, mu_lv and dh2 for the given eps [B x L] (None: sample = 0)."""
    params = [p.astype(dtype) for p in params]
    W_lat, W_dec, W_out = params[2], params[4], params[6]
    B, H = len(rows), W_dec.shape[1]
    eps = None if eps is None else eps.astype(dtype)
    ones = np.ones((1, B), dtype=dtype)
    X, Xs, h1, mu, lv, sd, z, h2 = _forward(m, rows, params, dropout, seed, eps, dtype)
    logits = _mm(h2, np.ascontiguousarray(W_out[:, :H].T)) + W_out[:, H]
    top = logits.max(axis=1, keepdims=True)
    lse = top + np.log(np.exp(logits - top).sum(axis=1, keepdims=True))
    n = X.sum(axis=1, keepdims=True)
    nll = _mm(ones, n * lse - _mm(X * logits, np.ones((X.shape[1], 1), dtype=dtype)))[0, 0] / dtype(B)
    live = n > 0
    terms = np.where(live, dtype(0.5) * (((np.exp(lv) + mu * mu) - 1) - lv), dtype(0))
    kl = _mm(ones, _mm(terms, np.ones((terms.shape[1], 1), dtype=dtype)))[0, 0] / dtype(B)
    g = (n * np.exp(logits - lse) - X) / dtype(B)
    dh2 = _mm(g, W_out[:, :H])
    dz2 = dh2 * (1 - h2 * h2)
    dzl = _mm(dz2, np.ascontiguousarray(W_dec.T))
    scale = dtype(beta) / dtype(B)
    dmu = dzl + scale * mu
    dlv = (dtype(0.5) * scale) * (np.exp(lv) - 1)
    if eps is not None:
        dlv = ((dtype(0.5) * dzl) * eps) * sd + dlv
    da = np.where(live, np.concatenate([dmu, dlv], axis=1), dtype(0))
    dz1 = _mm(da, np.ascontiguousarray(W_lat.T)) * (1 - h1 * h1)
    return dict(nll=nll, kl=kl, dW_in=_mm(Xs.T, dz1), db_in=_mm(ones, dz1), dW_lat=_mm(h1.T, da), db_lat=_mm(ones, da),
                dW_dec=_mm(z.T, dz2), db_dec=_mm(ones, dz2),
                dW_out=np.concatenate([_mm(g.T, h2), _mm(g.T, ones.T)], axis=1), mu_lv=np.concatenate([mu, lv], axis=1), dh2=dh2)


def random_params(rng, items, H, L, scale=0.3):
    """The seven parameters as float32; a sixth of b_lat's log-variance entries sit near +8 and a sixth near -8."""
    shapes = [(items, H), (1, H), (H, 2 * L), (1, 2 * L), (L, H), (1, H), (items, H + 1)]
    params = [rng.standard_normal(s) * (scale if s[0] > 1 else 0.1) for s in shapes]
    params[2] *= np.sqrt(32.0 / H)  # mu and lv spread alike at every H
    params[3][0, L:] += rng.choice([8.0, -8.0, 0.0], size=L, p=[1 / 6, 1 / 6, 2 / 3])
    return [p.astype(np.float32) for p in params]


def top_n(U, W_out, liked, N):
    """float64 top-N ids per row after the liked-item filter, the smallest gap between rank N and N + 1, the scores."""
    scores = U @ W_out.astype(np.float64).T
    ranked = -np.sort(-np.where(liked, -np.inf, scores), axis=1)
    return np.argsort(-np.where(liked, -np.inf, scores), axis=1)[:, :N], float((ranked[:, N - 1] - ranked[:, N]).min()), scores


def serving_case(N=10):
    """Random weights (hidden 32, latent 32, 500 items), 64 known users and 20 unseen rows, and for both sets (rows, want ids,
    gap, scores) in float64."""
    from implicit_amd.synthetic import synthetic_csr

    params = random_params(np.random.default_rng(11), 500, 32, 32)
    sets = []
    for rows in (synthetic_csr(300, 500, 6000, seed=3)[:64], synthetic_csr(20, 500, 400, seed=8)):
        rows = rows.tocsr()
        rows.sum_duplicates()
        sets.append((rows,) + top_n(encode(rows, np.arange(rows.shape[0]), params), params[6], rows.toarray() != 0, N))
    return params, sets


def adam_step(m, rows, params, moments, dropout, seed, beta, eps, lr, step, reg=0.0, b1=0.9, b2=0.999, eps_adam=1e-8, dtype=np.float64):
    """One step; moments = (m, v) per parameter in order.  Returns (nll, kl, params, moments)."""
    params, moments = [p.astype(dtype) for p in params], [a.astype(dtype) for a in moments]
    H = params[0].shape[1]
    out = gradients(m, rows, params, dropout, seed, beta, eps, dtype)
    c1, c2 = dtype(1 / (1 - float(b1) ** step)), dtype(1 / (1 - float(b2) ** step))
    lr, b1, b2, eps_adam, reg = (dtype(x) for x in (lr, b1, b2, eps_adam, reg))
    for i, name in enumerate(NAMES):
        g = out[name].copy()
        if i % 2 == 0:  # the weight matrices; W_out's last column is its bias
            cols = H if i == 6 else g.shape[1]
            g[:, :cols] += reg * params[i][:, :cols]
        moments[2 * i] = b1 * moments[2 * i] + (1 - b1) * g
        moments[2 * i + 1] = b2 * moments[2 * i + 1] + (1 - b2) * (g * g)
        params[i] = params[i] - lr * (moments[2 * i] * c1) / (np.sqrt(moments[2 * i + 1] * c2) + eps_adam)
    return out["nll"], out["kl"], params, moments
