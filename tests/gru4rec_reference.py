"""Host restatement of the GRU4Rec contract (csrc/gru4rec.hip), written from its equations with dense matrices.  dtype is
float64, or float32 for the tests' tolerances: then every operand and intermediate is float32 and every product one sequential
chain over the inner index (dae_reference._mm)."""
import numpy as np

from dae_reference import _mm


def _sigmoid(x):
    with np.errstate(over="ignore"):  # exp(+big) = inf gives the limit 0
        return 1 / (1 + np.exp(-x))


def forward(W_x, W_h, b, h, inputs, reset):
    """(h1, r, z, c, h0) of one step; the rows of idle slots hold h, 0, 0, 0, 0."""
    H, act = W_h.shape[0], inputs >= 0
    h0 = np.where((act & (reset == 0))[:, None], h, 0).astype(h.dtype)
    wx = np.where(act[:, None], W_x[np.maximum(inputs, 0)], 0).astype(h.dtype)
    r = _sigmoid((wx[:, :H] + b[:, :H]) + _mm(h0, W_h[:, :H]))
    z = _sigmoid((wx[:, H:2 * H] + b[:, H:2 * H]) + _mm(h0, W_h[:, H:2 * H]))
    c = np.tanh((wx[:, 2 * H:] + b[:, 2 * H:]) + _mm(r * h0, W_h[:, 2 * H:]))
    h1 = np.where(act[:, None], (1 - z) * h0 + z * c, h)
    r, z, c = (np.where(act[:, None], a, 0).astype(h.dtype) for a in (r, z, c))
    return h1.astype(h.dtype), r, z, c, h0


def loss_and_g(scores, targets, cols, loss, bpreg):
    """The step's loss and g = dL/dscores [B x S]; targets -1: an idle row; cols -1: a column that takes part nowhere."""
    dtype = scores.dtype.type
    B, S = scores.shape
    own = np.zeros((B, S), dtype=bool)
    own[np.arange(B), np.arange(B)] = True
    valid = (cols >= 0)[None, :] & (targets >= 0)[:, None] & (own | (cols[None, :] != targets[:, None]))
    A = int((targets >= 0).sum())
    g, total = np.zeros((B, S), dtype=dtype), dtype(0)
    for r in np.nonzero(targets >= 0)[0]:
        s, srr = scores[r], scores[r, r]
        use = valid[r] if loss == "cross-entropy" else valid[r] & ~own[r]
        if not use.any():
            continue
        top = s[use].max()
        e = np.where(use, np.exp(np.where(use, s - top, 0)), 0).astype(dtype)
        p = e / e.sum()
        if loss == "cross-entropy":
            total += (top + np.log(e.sum())) - srr
            g[r] = p - own[r]
        else:
            sg = _sigmoid(srr - s)
            P, R = (p * sg).sum(), (p * s * s).sum()
            total += bpreg * R - np.log(P + dtype(1e-24))
            g[r] = bpreg * (p * ((s * s + 2 * s) - R)) - (p * (sg * sg - P)) / (P + dtype(1e-24))
            g[r, r] = -(p * sg * (1 - sg)).sum() / (P + dtype(1e-24))
    if A == 0:
        return dtype(0), g
    return total / dtype(A), g / dtype(A)


def gradients(params, h, inputs, targets, reset, negatives, loss="bpr-max", bpreg=1.0, dtype=np.float64):
    """dict of loss, h1, da, dcol, dh1, dW_h, db, and the scores, g and column items of the step."""
    W_x, W_h, b, W_out = (a.astype(dtype) for a in params)
    inputs, targets, reset, negatives = (np.asarray(a, dtype=np.int64) for a in (inputs, targets, reset, negatives))
    H, act = W_h.shape[0], inputs >= 0
    h1, r, z, c, h0 = forward(W_x, W_h, b, h.astype(dtype), inputs, reset)
    rows = np.where(act, targets, -1)
    cols = np.concatenate([rows, negatives])
    Wc = np.where((cols >= 0)[:, None], W_out[np.maximum(cols, 0)], 0).astype(dtype)
    scores = _mm(h1, np.ascontiguousarray(Wc[:, :H].T)) + Wc[:, H]
    value, g = loss_and_g(scores, rows, cols, loss, dtype(bpreg))
    ones = np.ones((len(inputs), 1), dtype=dtype)
    dcol = _mm(np.ascontiguousarray(g.T), np.concatenate([h1, ones], axis=1))
    dh1 = _mm(g, Wc[:, :H])
    dz = (dh1 * (c - h0)) * (z * (1 - z))
    dc = (dh1 * z) * (1 - c * c)
    dr = (_mm(dc, np.ascontiguousarray(W_h[:, 2 * H:].T)) * h0) * (r * (1 - r))
    da = np.concatenate([dr, dz, dc], axis=1)
    dW_h = np.concatenate([_mm(np.ascontiguousarray(h0.T), da[:, :2 * H]), _mm(np.ascontiguousarray((r * h0).T), dc)], axis=1)
    return dict(loss=value, h1=h1, da=da, dcol=dcol, dh1=dh1, dW_h=dW_h, db=_mm(ones.T, da), scores=scores, g=g, cols=cols)


def adagrad_step(params, accs, h, inputs, targets, reset, negatives, loss, bpreg, lr, dtype=np.float64):
    """One training step; returns (loss, params, accs, h).  A row that occurs several times receives the sum of its
    occurrences, in ascending position, once."""
    params, accs = [p.astype(dtype).copy() for p in params], [a.astype(dtype).copy() for a in accs]
    inputs = np.asarray(inputs)
    if not (inputs >= 0).any():
        return dtype(0), params, accs, h.astype(dtype)
    out = gradients(params, h, inputs, targets, reset, negatives, loss, bpreg, dtype)

    def apply(i, rows, G):
        accs[i][rows] = accs[i][rows] + G * G
        params[i][rows] = params[i][rows] - (dtype(lr) * G) / np.sqrt(accs[i][rows] + dtype(1e-6))

    for i, ids, per in ((0, inputs, out["da"]), (3, out["cols"], out["dcol"])):
        for row in np.unique(ids[ids >= 0]):
            G = np.zeros(per.shape[1], dtype=dtype)
            for at in np.nonzero(ids == row)[0]:
                G = G + per[at]
            apply(i, row, G)
    apply(1, slice(None), out["dW_h"])
    apply(2, slice(None), out["db"])
    return out["loss"], params, accs, out["h1"]


def encode(sessions, W_x, W_h, b, dtype=np.float64):
    """[h after the session's last item | 1], one row per session."""
    W_x, W_h, b = (a.astype(dtype) for a in (W_x, W_h, b))
    h = np.zeros((len(sessions), W_h.shape[0]), dtype=dtype)
    for t in range(max([len(s) for s in sessions], default=0)):
        inputs = np.array([s[t] if t < len(s) else -1 for s in sessions], dtype=np.int64)
        h = forward(W_x, W_h, b, h, inputs, np.zeros(len(sessions), dtype=np.int64) + (t == 0))[0]
    return np.concatenate([h, np.ones((len(sessions), 1), dtype=dtype)], axis=1)


def planted(seed, items=40, train=400, held=200, length=8, follow=0.97):
    """Sessions in which the next item is (i + 1) mod items with probability `follow`, otherwise uniform: (train, held-out)."""
    rng = np.random.default_rng(1000 + seed)
    sessions = []
    for _ in range(train + held):
        s = [int(rng.integers(items))]
        for _ in range(length - 1):
            s.append((s[-1] + 1) % items if rng.random() < follow else int(rng.integers(items)))
        sessions.append(np.array(s, dtype=np.int32))
    return sessions[:train], sessions[train:]


def fit(sessions, n_items, seed, hidden, loss, n_sample, sample_alpha, bpreg, learning_rate, batch_size, iterations, dtype=np.float64):
    """The model's fit (implicit_amd/gpu/gru4rec.py) restated: the same draws in the same order, every step by adagrad_step.
    Returns (params, the last epoch's mean loss)."""
    from implicit_amd.gpu.gru4rec import as_sessions, session_parallel_schedule

    rs, H = np.random.default_rng(seed), hidden
    indptr, items = as_sessions(sessions)

    def uniform(rows, cols):
        bound = np.sqrt(6.0 / (rows + cols))
        return rs.uniform(-bound, bound, size=(rows, cols)).astype(np.float32)

    params = [uniform(n_items, 3 * H), uniform(H, 3 * H), np.zeros((1, 3 * H), dtype=np.float32), uniform(n_items, H + 1)]
    params[3][:, H] = 0.0
    accs = [np.zeros(p.shape) for p in params]
    trainable = np.nonzero(np.diff(indptr) >= 2)[0]
    support = np.bincount(np.concatenate([sessions[s] for s in trainable]), minlength=n_items).astype(np.float64) ** sample_alpha
    for _ in range(iterations):
        inputs, targets, reset = session_parallel_schedule(indptr, items, trainable[rs.permutation(len(trainable))], batch_size)
        negatives = np.zeros((len(inputs), n_sample), dtype=np.int32)
        if n_sample:
            negatives = rs.choice(n_items, size=(len(inputs), n_sample), p=support / support.sum()).astype(np.int32)
        h, losses = np.zeros((batch_size, H), dtype=dtype), []
        for t in range(len(inputs)):
            value, params, accs, h = adagrad_step(params, accs, h, inputs[t], targets[t], reset[t], negatives[t], loss, bpreg, learning_rate, dtype)
            losses.append(value)
    return params, float(np.mean(losses))


def hit_rate(held, W_x, W_h, b, W_out, dtype=np.float64):
    """hit rate@1 of the held-out sessions' last item from the items before it."""
    scores = encode([s[:-1] for s in held], W_x, W_h, b, dtype) @ W_out.astype(dtype).T
    return float((scores.argmax(axis=1) == np.array([s[-1] for s in held])).mean())
