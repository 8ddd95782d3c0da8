"""The last CG step of the tile kernels forms only the scalar p.Ap = p.(A0 p) + sum_k (|c_k|-1) (y_k.p)^2 instead of the
vector Ap.  A numpy fp32 restatement of the oracle's CG (implicit/cpu/_als.pyx:152-248) with the last step
in both forms shows what that re-association costs: nothing beyond rounding.

Bar: |x_scalar - x_vector| / |x_f64| < 1e-5, five times the 1.9e-6 this restatement measured as its worst case (2e-7
typical) when the change was proposed; both forms are equally far from the fp64 solution, and the project's parity bar is
1e-4.
"""
import numpy as np
import pytest

F = 128
ITEMS = 3000
ROWS = 40
BAR = 1e-5


def _cg(A0, Yu, c, x, steps, scalar_last, dt):
    A0, Yu, c, x = A0.astype(dt), Yu.astype(dt), c.astype(dt), x.astype(dt).copy()
    cm1, cp = np.abs(c) - 1, np.maximum(c, 0)
    r = -(A0 @ x) + Yu.T @ (cp - cm1 * (Yu @ x))
    p = r.copy()
    rsold = r @ r
    if rsold < 1e-20:
        return x
    for it in range(steps):
        last = it == steps - 1
        d = Yu @ p
        if last and scalar_last:
            pAp = p @ (A0 @ p) + dt(np.sum((cm1 * d * d).astype(dt), dtype=dt))
        else:
            Ap = A0 @ p + Yu.T @ (cm1 * d)
            pAp = p @ Ap
        x = x + dt(rsold / pAp) * p
        if last:
            break
        r = r - dt(rsold / pAp) * Ap
        rsnew = r @ r
        if rsnew < 1e-20:
            break
        p = r + dt(rsnew / rsold) * p
        rsold = rsnew
    return x


def _factors(kind):
    rng = np.random.default_rng(0 if kind == "warm" else 1)
    u = rng.random((ITEMS, F))
    Y = ((u - 0.5) * 0.2 if kind == "warm" else u * 0.01).astype(np.float32)
    A0 = (Y.T.astype(np.float64) @ Y + 0.05 * np.eye(F)).astype(np.float32)
    return Y, A0


_FACTORS = {kind: _factors(kind) for kind in ("warm", "cold")}


@pytest.mark.parametrize("kind", ["warm", "cold"])
@pytest.mark.parametrize("n", [1, 5, 16, 32, 45, 100, 300, 512])
def test_scalar_last_step_is_within_rounding_of_the_vector_form(kind, n):
    Y, A0 = _FACTORS[kind]
    rng = np.random.default_rng(1000 + n)
    worst = {"vector-vs-f64": 0.0, "scalar-vs-f64": 0.0, "scalar-vs-vector": 0.0}
    for _ in range(ROWS):
        cols = rng.choice(ITEMS, n, replace=False)
        c = 1 + 4 * rng.random(n)
        c[rng.random(n) < 0.1] *= -1
        u = rng.random(F)
        x0 = ((u - 0.5) * 0.2 if kind == "warm" else u * 0.01).astype(np.float32)
        for steps in (1, 3):
            exact = _cg(A0, Y[cols], c, x0, steps, False, np.float64)
            vec = _cg(A0, Y[cols], c, x0, steps, False, np.float32)
            sca = _cg(A0, Y[cols], c, x0, steps, True, np.float32)
            assert vec.dtype == np.float32 and sca.dtype == np.float32
            nrm = np.linalg.norm(exact)
            worst["vector-vs-f64"] = max(worst["vector-vs-f64"], np.linalg.norm(vec - exact) / nrm)
            worst["scalar-vs-f64"] = max(worst["scalar-vs-f64"], np.linalg.norm(sca - exact) / nrm)
            worst["scalar-vs-vector"] = max(worst["scalar-vs-vector"], np.linalg.norm(sca.astype(np.float64) - vec) / nrm)
    print(kind, "n", n, " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["scalar-vs-vector"] < BAR
