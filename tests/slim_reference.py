"""Host restatement of the SLIM solver (numpy only) and the inputs the CPU and the GPU suites share.

With A = X^T X + l2 I, column j minimises  1/2 w^T A w - sum_i A[j, i] w_i + l1 sum_i |w_i|  subject to w_j = 0 (and w >= 0
when `positive`) by cyclic coordinate descent.  solve32 restates, operation for operation, what imp_slim_solve promises bit for
bit (include/implicit_hip.h); solve64 is the same rule in float64; chunked32 models the kernel's evaluate / first-changed /
apply / re-evaluate loop and has to equal solve32 bit for bit (tests/test_slim_host.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ease_reference import gram64  # noqa: E402
from implicit_amd.synthetic import synthetic_csr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slim_golden.npz")
CHUNK = 1024  # the chunk width slim.hip chose: one coordinate per thread of a 1024-thread workgroup
MAX_ITEMS = 40000  # IMP_SLIM_MAX_ITEMS


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def _solve(A, j, l1, positive, max_sweeps, tol, dtype):
    A = np.asarray(A, dtype=dtype)
    n = A.shape[0]
    l1, tol, zero = dtype(l1), dtype(tol), dtype(0.0)
    w = np.zeros(n, dtype=dtype)
    r = np.zeros(n, dtype=dtype)
    diag = [dtype(x) for x in np.diag(A)]
    target = [dtype(x) for x in A[j]]
    sweeps = 0
    for s in range(1, max_sweeps + 1):
        sweeps = s
        dmax = zero
        for i in range(n):
            if i == j:
                continue
            a = diag[i]
            wi = w[i]
            rho = (target[i] - r[i]) + a * wi  # every operation rounds to `dtype`
            if positive:
                t = rho - l1
                new = t / a if t > 0 else zero
            elif rho > l1:
                new = (rho - l1) / a
            elif rho < -l1:
                new = (rho + l1) / a
            else:
                new = zero
            d = new - wi
            if d != 0:
                w[i] = new
                r = r + d * A[i]  # the only vectorised step: product and sum rounded separately, element by element
                dmax = max(dmax, abs(d))
        wmax = np.max(np.abs(w)) if n else zero
        if dmax <= tol * wmax:
            break
    return w, sweeps


def solve32(A, j, l1, positive, max_sweeps, tol):
    """(w float32, sweeps): column j by the rule of imp_slim_solve with np.float32 scalars."""
    return _solve(A, j, l1, positive, max_sweeps, tol, np.float32)


def solve64(A, j, l1, positive, max_sweeps, tol):
    return _solve(A, j, l1, positive, max_sweeps, tol, np.float64)


def chunked32(A, j, l1, positive, max_sweeps, tol, chunk):
    """The kernel's loop: a chunk of coordinates is evaluated against the current r at once, the lowest one with d != 0 is
    applied, and only the coordinates after it are evaluated again."""
    A = np.asarray(A, dtype=np.float32)
    n = A.shape[0]
    l1, tol, zero = np.float32(l1), np.float32(tol), np.float32(0.0)
    w = np.zeros(n, dtype=np.float32)
    r = np.zeros(n, dtype=np.float32)
    diag = np.diag(A).copy()
    target = A[j].copy()
    sweeps = 0
    for s in range(1, max_sweeps + 1):
        sweeps = s
        dmax = zero
        for c0 in range(0, n, chunk):
            lo, hi = c0, min(n, c0 + chunk)
            while lo < hi:
                a, wi = diag[lo:hi], w[lo:hi]
                rho = (target[lo:hi] - r[lo:hi]) + a * wi
                if positive:
                    t = rho - l1
                    new = np.where(t > 0, t / a, zero)
                else:
                    new = np.where(rho > l1, (rho - l1) / a, np.where(rho < -l1, (rho + l1) / a, zero))
                d = (new - wi).astype(np.float32)
                if lo <= j < hi:
                    d[j - lo] = zero
                moved = np.flatnonzero(d != 0)
                if not len(moved):
                    break
                f = moved[0]
                w[lo + f] = new[f]
                r = r + d[f] * A[lo + f]
                dmax = max(dmax, abs(d[f]))
                lo += f + 1
        wmax = np.max(np.abs(w)) if n else zero
        if dmax <= tol * wmax:
            break
    return w, sweeps


# ---- cases ------------------------------------------------------------------------------------------------------------------
L1, L2 = 4.0, 10.0
SIZES = sorted({1, 2, 63, 64, 65, 257, 1025, CHUNK - 1, CHUNK, CHUNK + 1})  # the kernel changes path at the chunk width only
SETTINGS = ((1, 1e-4), (2, 1e-4), (5, 0.0), (100, 1e-4))  # (max_sweeps, tol)
_cases = {}


def case(n, l2=L2):
    """(A float32 n x n, empty item or None, twins (a, b) or None): X^T X + l2 I of synthetic_csr(4n, n, 48n, seed=n) with one
    item nobody has (n - 2) and two identical item columns (1 and 3) planted where n >= 5."""
    if (n, l2) not in _cases:
        D = np.asarray(synthetic_csr(4 * n, n, 48 * n, seed=n).todense(), dtype=np.float64)
        empty = twins = None
        if n >= 5:
            empty, twins = n - 2, (1, 3)
            D[:, 3] = D[:, 1]
            D[:, empty] = 0.0
        A = np.ascontiguousarray(gram64(D, l2), dtype=np.float32)
        A.setflags(write=False)
        _cases[(n, l2)] = (A, empty, twins)
    return _cases[(n, l2)]


def columns(n, A, empty, twins):
    """Every column when n <= 65; otherwise 16: 0, 1, n - 1, the largest diagonal, the empty item's, a twin and ten seeded."""
    if n <= 65:
        return list(range(n))
    cols = [0, 1, n - 1, int(np.argmax(np.diag(A))), empty, twins[1]]
    rng = np.random.default_rng(n)
    for c in rng.permutation(n):
        if len(cols) == 16:
            break
        if int(c) not in cols:
            cols.append(int(c))
    return cols


_expected = {}


def expected(n, j, l1, positive, max_sweeps, tol, l2=L2):
    """solve32 of column j of case(n), computed once per process."""
    key = (n, j, float(l1), bool(positive), max_sweeps, float(tol), l2)
    if key not in _expected:
        _expected[key] = solve32(case(n, l2)[0], j, l1, positive, max_sweeps, tol)
    return _expected[key]


# max_j ||solve32_j - w_sklearn_j|| / ||w_sklearn_j|| over the columns of the golden X at max_sweeps = 100, tol = 1e-6, measured on
# the host, keyed by (setting, positive); the supports came out identical in all four.  The tests assert twice the figure: the
# float32 rule is deterministic, the factor only absorbs another numpy or BLAS in gram64.
GOLDEN_MAX_SWEEPS, GOLDEN_TOL = 100, 1e-6
GOLDEN_DISTANCE = {(0, False): 8.346167e-06, (0, True): 9.259431e-06, (1, False): 5.894835e-06, (1, True): 3.767768e-06}


def column_distance(W, W_ref):
    """(max_j ||W[:, j] - W_ref[:, j]|| / ||W_ref[:, j]|| over the columns with a nonzero reference, largest support difference)."""
    W = np.asarray(W, dtype=np.float64)
    worst, support = 0.0, 0
    for j in range(W_ref.shape[1]):
        norm = np.linalg.norm(W_ref[:, j])
        support = max(support, int(((W[:, j] != 0) != (W_ref[:, j] != 0)).sum()))
        if norm > 0:
            worst = max(worst, float(np.linalg.norm(W[:, j] - W_ref[:, j]) / norm))
    return worst, support


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
