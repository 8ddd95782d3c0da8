"""Randomized truncated SVD of a sparse matrix on the device: Python over spmm, multiply_small and the gramian kernel, the way
EASE.fit is Python over its primitives.  Only the l x l eigenproblems run on the host."""
import numpy as np

from ._cuda import CSRMatrix, LeastSquaresSolver, Matrix, RandomState, multiply_small, spmm

MAX_SKETCH = 1024  # columns spmm and multiply_small accept


def _gram_eigh(solver, Y, G):
    """(eigenvalues descending, eigenvectors) in float64 of the symmetrised fp32 gramian Y^T Y (G: an l x l scratch Matrix)."""
    solver.calculate_yty(Y, G, 0.0)
    g = G.to_numpy().astype(np.float64)
    lam, W = np.linalg.eigh(0.5 * (g + g.T))
    return lam[::-1], W[:, ::-1]


def _kept(lam, rank_tolerance):
    """The eigenvalues that count: larger than rank_tolerance times the largest (none of a zero matrix)."""
    top = lam[0] if len(lam) else 0.0
    return (lam > rank_tolerance * top) & (lam > 0)


def _orth(solver, Y, spare, G, rank_tolerance):
    """Y with orthonormal columns spanning the same space, columns of directions below the cut zeroed: twice
    Y <- Y (W diag(lam)^-1/2) from the eigen-decomposition of Y^T Y.  Returns (the result, the other buffer)."""
    for _ in range(2):
        lam, W = _gram_eigh(solver, Y, G)
        keep = _kept(lam, rank_tolerance)
        T = np.zeros_like(W)
        T[:, keep] = W[:, keep] / np.sqrt(lam[keep])
        multiply_small(Y, Matrix(T.astype(np.float32)), out=spare)
        Y, spare = spare, Y
    return Y, spare


def randomized_svd(user_items, item_users, k, oversample=10, power_iterations=2, omega=None, random_state=None,
                   rank_tolerance=2.0**-16):
    """The k leading singular triplets of A = user_items by randomized subspace iteration (Halko, Martinsson, Tropp 2011,
    algorithms 4.4 and 5.1) with l = k + oversample <= 1024 sketch columns:

        Q = orth(A Omega)                            Omega: items x l, N(0, 1) from a RandomState unless `omega` is given
        power_iterations times:  Z = orth(A^T Q);  Q = orth(A Z)
        B = A^T Q;  B^T B = W S^2 W^T                float64 eigh of the symmetrised l x l gramian, descending
        V = B W S^-1,  U = Q W,  sigma = S           the first k columns

    user_items / item_users: the two orientations of A as CSRMatrix handles.  omega: a float32 items x l Matrix.  random_state:
    a gpu.RandomState, or what check_random_state makes one from.  orth(Y) is applied twice through the eigen-decomposition
    of Y^T Y; wherever an eigenvalue is at most rank_tolerance times the largest the column is zeroed, in the last step
    sigma = 0, u = 0, v = 0: a rank-deficient matrix yields fewer non-zero triplets instead of noise.  The cut acts on squared
    singular values, so with the default 2^-16 directions below 2^-8 of sigma_1 are given up.

    Returns (U: Matrix users x k, sigma: float64 ndarray of length k, V: Matrix items x k).  Nothing of size users or items
    crosses the bus."""
    if not isinstance(user_items, CSRMatrix) or not isinstance(item_users, CSRMatrix):
        raise TypeError("randomized_svd: user_items and item_users must be implicit_amd.gpu.CSRMatrix")
    users, items = user_items.shape
    if tuple(item_users.shape) != (items, users) or item_users.nnz != user_items.nnz:
        raise ValueError("randomized_svd: item_users and user_items must be the two orientations of one matrix")
    k, oversample, power_iterations = int(k), int(oversample), int(power_iterations)
    if k < 1 or oversample < 0 or power_iterations < 0:
        raise ValueError("randomized_svd: k must be >= 1, oversample and power_iterations >= 0")
    sketch = k + oversample
    if sketch > MAX_SKETCH:
        raise ValueError(f"randomized_svd: k + oversample = {sketch} exceeds {MAX_SKETCH}")
    if omega is None:
        if not isinstance(random_state, RandomState):
            from .matrix_factorization_base import check_random_state  # imports this package

            random_state = check_random_state(random_state)
        omega = random_state.randn(items, sketch)
    elif not isinstance(omega, Matrix) or tuple(omega.shape) != (items, sketch) or omega.itemsize != 4:
        raise ValueError(f"randomized_svd: omega must be a float32 Matrix of shape ({items}, {sketch})")

    solver = LeastSquaresSolver()
    G = Matrix.zeros(sketch, sketch)
    Q, q_spare = Matrix.zeros(users, sketch), Matrix.zeros(users, sketch)
    Z, z_spare = Matrix.zeros(items, sketch), Matrix.zeros(items, sketch)
    spmm(user_items, omega, out=Q)
    Q, q_spare = _orth(solver, Q, q_spare, G, rank_tolerance)
    for _ in range(power_iterations):
        spmm(item_users, Q, out=Z)
        Z, z_spare = _orth(solver, Z, z_spare, G, rank_tolerance)
        spmm(user_items, Z, out=Q)
        Q, q_spare = _orth(solver, Q, q_spare, G, rank_tolerance)
    spmm(item_users, Q, out=Z)  # B
    s2, W = _gram_eigh(solver, Z, G)
    keep = _kept(s2, rank_tolerance)[:k]
    sigma = np.zeros(k)
    sigma[keep] = np.sqrt(s2[:k][keep])
    Wu, Wv = np.zeros((sketch, k)), np.zeros((sketch, k))
    Wu[:, keep] = W[:, :k][:, keep]
    Wv[:, keep] = W[:, :k][:, keep] / sigma[keep]
    U = multiply_small(Q, Matrix(Wu.astype(np.float32)))
    V = multiply_small(Z, Matrix(Wv.astype(np.float32)))
    return U, sigma, V
