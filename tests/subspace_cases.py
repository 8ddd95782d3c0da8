"""The inputs of the block-subspace half sweep's tests (tests/test_gpu_subspace.py) and the two restatements they are judged by.
tests/test_subspace_cases_host.py proves on the CPU that the restatements and the problems are what they claim to be.  Test
infrastructure only; nothing here touches a GPU.

The contract (include/implicit_hip.h, imp_solver_least_squares_subspace), in the notation of cholesky_cases._normal_parts: for a
row with stored entries (j, c_j), w_j = |c_j| - 1, c+_j = max(c_j, 0), A = G + reg I + sum_j w_j y_j y_j^T, b = sum_j c+_j y_j.
A sweep starts from the stored x: p_j = x . y_j; then for the blocks S = [0, k), [k, 2k), ... (the last possibly shorter)
    g = (G x)_S + reg x_S + sum_j (w_j p_j - c+_j) y_j[S],   H = G_SS + reg I + sum_j w_j y_j[S] y_j[S]^T,
    delta = -H^-1 g,   x_S += delta,   p_j += delta . y_j[S];
further sweeps repeat the block loop without recomputing p.  Empty rows become zero; a row with a non-positive pivot fails.

sweep_f64: the contract in float64 from the fp32 inputs.
sweep_f32: the same steps in float32 with every sum -- over a row's entries, over the factors, inside the k x k factorisation --
accumulated left to right in stored order by elementwise operations: no pairwise summation, no BLAS.  It is the yardstick of
the GPU tests: a kernel whose reductions are trees of the same length errs by the same order, not more."""
import functools
from types import SimpleNamespace

import numpy as np

import cholesky_cases as cc

# the kernel's cuts (csrc/als_subspace.hip): 8 nonzeros per gather trip and 64 per chunk of the wave kernel; rows of more than
# 1024 nonzeros leave the one-wavefront kernel for the segment kernels; segments hold 1024 nonzeros.  Predictions always live in
# the workspace: there is no LDS / workspace cut.
WAVE_CUT, SEGMENT = 1024, 1024
CUT_LENGTHS = [7, 8, 9, 63, WAVE_CUT - 1, WAVE_CUT, WAVE_CUT + 1, 2 * SEGMENT - 1, 2 * SEGMENT, 2 * SEGMENT + 1]
LENGTHS = cc.LENGTHS + [5000] + CUT_LENGTHS
COLS, REG, EXTRA_ROWS = 6000, 0.01, 3
GRID = [(8, 8), (16, 4), (20, 8), (20, 1), (32, 32), (64, 16), (96, 32), (130, 32), (256, 32), (520, 32)]
SWEEPS = (1, 3)
FAILING_SETS = cc.FAILING_SETS
POISON_CONFIDENCE, POISON_SCALE = 0.25, 3.0


def _ordered_sum(a):
    """Sum over axis 0, strictly left to right in the array's dtype: numpy reduces a leading (slow) axis by adding one slice
    after the other (pairwise summation is only used along the contiguous axis, which axis 0 is for a single column; the
    host tests check both shapes against a loop)."""
    a = np.ascontiguousarray(a)
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:], a.dtype)
    if a[0].size == 1:  # one column: axis 0 is the contiguous axis, which numpy would sum pairwise; a running sum is sequential
        return np.add.accumulate(a, axis=0)[-1]
    return np.add.reduce(a, axis=0)


def _ordered_gram(u, y, chunk=256):
    """sum_j u_j y_j^T, one rank-one term after the other (chunks only bound the temporary: the running sum leads every chunk)."""
    acc = np.zeros((u.shape[1], y.shape[1]), u.dtype)
    for lo in range(0, len(u), chunk):
        terms = u[lo:lo + chunk, :, None] * y[lo:lo + chunk, None, :]
        acc = _ordered_sum(np.concatenate([acc[None], terms]))
    return acc


def _newton(H, g):
    """(-H^-1 g, bad) for a batch of k x k systems by a right-looking Cholesky factorisation and two substitutions written
    with elementwise operations only (the batch's dtype throughout); bad marks the systems that met a non-positive pivot."""
    L, z = H.copy(), g.copy()
    k = z.shape[1]
    bad = np.zeros(len(z), bool)
    one = L.dtype.type(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(k):
            d = L[:, c, c]
            bad |= ~(d > 0)
            sd = np.sqrt(np.where(bad, one, d))
            col = L[:, c + 1:, c] / sd[:, None]
            L[:, c + 1:, c] = col
            L[:, c, c] = sd
            z[:, c] = z[:, c] / sd
            z[:, c + 1:] -= col * z[:, c:c + 1]
            L[:, c + 1:, c + 1:] -= col[:, :, None] * col[:, None, :]
        for c in reversed(range(k)):
            z[:, c] = z[:, c] / L[:, c, c]
            z[:, :c] -= L[:, c, :c] * z[:, c:c + 1]
    return -z, bad


def _sweeps(C, X0, Y, gram, reg, k, sweeps, dt, ordered):
    dt = np.dtype(dt)
    n, f = C.shape[0], Y.shape[1]
    Yd, G, lam = np.asarray(Y, np.float32).astype(dt), np.asarray(gram).astype(dt), dt.type(reg)
    X = np.asarray(X0, np.float32)[:n].astype(dt)
    lens = np.diff(C.indptr)
    X[lens == 0] = 0
    rows = [u for u in range(n) if lens[u]]
    ys, w, cp, p = {}, {}, {}, {}
    for u in rows:
        lo, hi = C.indptr[u], C.indptr[u + 1]
        c = C.data[lo:hi].astype(dt)
        ys[u], w[u], cp[u] = Yd[C.indices[lo:hi]], np.abs(c) - dt.type(1), np.maximum(c, dt.type(0))
        p[u] = _ordered_sum((ys[u] * X[u]).T) if ordered else ys[u] @ X[u]
    failed, out = set(), []
    for _ in range(sweeps):
        for s0 in range(0, f, k):
            S = slice(s0, min(s0 + k, f))
            kb = S.stop - S.start
            live = [u for u in rows if u not in failed]
            H, g = np.empty((len(live), kb, kb), dt), np.empty((len(live), kb), dt)
            for i, u in enumerate(live):
                yS = np.ascontiguousarray(ys[u][:, S])
                coef = w[u] * p[u] - cp[u]
                if ordered:
                    gx, gs = _ordered_sum((G[S] * X[u]).T), _ordered_sum(coef[:, None] * yS)
                    Hs = _ordered_gram(w[u][:, None] * yS, yS)
                else:
                    gx, gs, Hs = G[S] @ X[u], coef @ yS, (yS.T * w[u]) @ yS
                g[i] = (gs + gx) + lam * X[u, S]
                H[i] = Hs + G[S, S] + lam * np.eye(kb, dtype=dt)
            delta, bad = _newton(H, g)
            for i, u in enumerate(live):
                if bad[i]:
                    failed.add(u)
                    continue
                X[u, S] += delta[i]
                yS = ys[u][:, S]
                p[u] = p[u] + (_ordered_sum((yS * delta[i]).T) if ordered else yS @ delta[i])
        out.append(X.copy())
    return out, sorted(failed)


def sweep_f64(C, X0, Y, gram, reg, k, sweeps=1):
    """([X after sweep 1, ..., X after sweep `sweeps`], failing rows): the contract in float64 from the fp32 inputs.  Rows of X0
    beyond the matrix are dropped; a failing row's contents are unspecified."""
    return _sweeps(C, X0, Y, gram, reg, k, sweeps, np.float64, False)


def sweep_f32(C, X0, Y, gram, reg, k, sweeps=1):
    """The same steps in float32, every sum accumulated left to right in stored order."""
    return _sweeps(C, X0, Y, gram, reg, k, sweeps, np.float32, True)


def row_energy(C, X, Y, gram, reg):
    """{row: x^T A x / 2 - b^T x} in float64 for every non-empty row."""
    return {u: float(0.5 * X[u] @ A @ X[u] - b @ X[u]) for u, A, b in cc._normal_parts(C, Y, gram, reg)}


def block_spectra(C, Y, gram, reg, k):
    """{row: [lambda_min of every block's H]} in float64 for every non-empty row."""
    f = Y.shape[1]
    return {u: [float(np.linalg.eigvalsh(A[s0:s0 + k, s0:s0 + k])[0]) for s0 in range(0, f, k)]
            for u, A, _ in cc._normal_parts(C, Y, gram, reg)}


def _confidences(rng, n):
    c = (1 + 39 * rng.random(n)).astype(np.float32)
    c[rng.random(n) < 0.1] *= -1
    c[::37] = 1.0  # weight 0
    return c


def _rows(rng, lengths, cols):
    return [(np.sort(rng.choice(cols, size=n, replace=False)), _confidences(rng, n)) for n in lengths]


@functools.lru_cache(maxsize=None)
def routes_problem(f):
    """A row of every length in LENGTHS over 6000 columns, confidences uniform in [1, 40] with about 10 % negated and every
    37th equal to 1 (weight 0), Y uniform in +-0.15, X0 (three rows more than C) uniform in [0, 0.01), the genuine gramian
    in float32 from a float64 sum, reg 0.01."""
    rng = np.random.default_rng(4000 + f)
    Y = ((rng.random((COLS, f), dtype=np.float32) - np.float32(0.5)) * np.float32(0.3)).astype(np.float32)
    X0 = rng.random((len(LENGTHS) + EXTRA_ROWS, f), dtype=np.float32) * np.float32(0.01)
    Y64 = Y.astype(np.float64)
    p = SimpleNamespace(name=f"routes-f{f}", f=f, C=cc._csr(_rows(rng, LENGTHS, COLS), COLS), Y=Y, X0=X0,
                        gram=(Y64.T @ Y64).astype(np.float32), reg=REG, failing=())
    for a in (p.Y, p.X0, p.gram):
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def failing_problem(f, failing):
    """cholesky_cases.LENGTHS over 2400 columns and one more, the poison item 3 e_0; the identity as gramian, reg 0; every row
    of `failing` holds the poison item with confidence 0.25 (weight -0.75): its first block's H has an eigenvalue near
    1 - 0.75 * 9.  Small item rows (+-0.02) and integer confidences of magnitude 1 .. 5, about 10 % negated, keep the other
    entries' part of that eigenvalue below 1."""
    failing = tuple(failing)
    assert all(cc.LENGTHS[r] >= 2 for r in failing)
    rng = np.random.default_rng(5000 + f)
    cols = cc.COLS
    Y = np.zeros((cols + 1, f), np.float32)
    Y[:cols] = (rng.random((cols, f), dtype=np.float32) - np.float32(0.5)) * np.float32(0.04)
    Y[cols, 0] = POISON_SCALE
    rows = []
    for n in cc.LENGTHS:
        c = rng.integers(1, 6, size=n).astype(np.float32)
        c[rng.random(n) < 0.1] *= -1
        rows.append((np.sort(rng.choice(cols, size=n, replace=False)), c))
    for r in failing:
        ids, c = rows[r]
        ids[-1], c[-1] = cols, POISON_CONFIDENCE  # the largest column id: still sorted
    X0 = rng.random((len(cc.LENGTHS) + EXTRA_ROWS, f), dtype=np.float32) * np.float32(0.01)
    return SimpleNamespace(name=f"failing-f{f}-" + "_".join(map(str, failing)), f=f, C=cc._csr(rows, cols + 1), Y=Y, X0=X0,
                           gram=np.eye(f, dtype=np.float32), reg=0.0, failing=failing)


@functools.lru_cache(maxsize=None)
def reference(name, f, k, sweeps, failing=()):
    """(X64 per sweep, X32 per sweep, failing rows) of a problem ("routes" or "failing"), computed once and read-only."""
    p = routes_problem(f) if name == "routes" else failing_problem(f, failing)
    x64, bad64 = sweep_f64(p.C, p.X0, p.Y, p.gram, p.reg, k, sweeps)
    x32, bad32 = sweep_f32(p.C, p.X0, p.Y, p.gram, p.reg, k, sweeps)
    assert bad64 == bad32 == sorted(p.failing)
    for a in x64 + x32:
        a.setflags(write=False)
    return x64, x32, bad64


def distance(got, want, rows=None):
    """Relative Frobenius distance over `rows` (all by default)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if rows is not None:
        got, want = got[rows], want[rows]
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def alternate(sweep, Cui, X0, Y0, reg, k, iterations, sweeps=1):
    """`iterations` of the model's fit on the host with `sweep` (sweep_f64 or sweep_f32): users from items, then items from the
    new users.  The factors are float32 after every half sweep, as on the device.  The gramian of the other side's factors is
    exact (float64) for sweep_f64 and a float32 sum, one row after the other, for sweep_f32."""
    Ciu = Cui.T.tocsr()
    Ciu.sort_indices()
    X, Y = np.array(X0, np.float32), np.array(Y0, np.float32)

    def gram(M):
        return _ordered_gram(M, M) if sweep is sweep_f32 else M.astype(np.float64).T @ M.astype(np.float64)

    for _ in range(iterations):
        for C, own in ((Cui, "X"), (Ciu, "Y")):
            mine, other = (X, Y) if own == "X" else (Y, X)
            out, bad = sweep(C, mine, other, gram(other), reg, k, sweeps)
            assert not bad
            mine[:] = out[-1].astype(np.float32)
    return X, Y
