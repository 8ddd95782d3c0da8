"""Writes tests/golden/slim_golden.npz: a 60 x 40 integer-valued matrix X and, for positive in (True, False) at two (l1, l2)
settings, the float64 SLIM weights from scikit-learn's coordinate descent run to tol = 1e-12.

    python tests/golden/make_slim_golden.py

X has an empty user (row 1), an item nobody has (column 38) and two identical item columns (4 and 5).  Column j of W is

    ElasticNet(alpha=(l1 + l2) / users, l1_ratio=l1 / (l1 + l2), positive=positive, fit_intercept=False, tol=1e-12,
               max_iter=100000).fit(X with column j zeroed, X[:, j]).coef_

scikit-learn minimises 1/(2 users) ||y - Z w||^2 + alpha l1_ratio ||w||_1 + alpha (1 - l1_ratio)/2 ||w||^2, which times `users` is
the Gram form of the solver's contract with A = X^T X + l2 I.  This is the only file that imports scikit-learn."""
import os

import numpy as np
from sklearn.linear_model import ElasticNet

HERE = os.path.dirname(os.path.abspath(__file__))
USERS, ITEMS = 60, 40
SETTINGS = ((1.0, 10.0), (3.0, 20.0))  # (l1, l2)


def main():
    rng = np.random.default_rng(2011)
    X = np.where(rng.random((USERS, ITEMS)) < 0.25, rng.integers(1, 4, size=(USERS, ITEMS)), 0).astype(np.float64)
    X[1, :] = 0.0
    X[:, 5] = X[:, 4]
    X[:, 38] = 0.0
    W = np.zeros((len(SETTINGS), 2, ITEMS, ITEMS))  # [setting][positive][source i][target j]
    for s, (l1, l2) in enumerate(SETTINGS):
        for p in (0, 1):
            for j in range(ITEMS):
                Z = X.copy()
                Z[:, j] = 0.0
                model = ElasticNet(alpha=(l1 + l2) / USERS, l1_ratio=l1 / (l1 + l2), positive=bool(p), fit_intercept=False,
                                   tol=1e-12, max_iter=100000)
                model.fit(Z, X[:, j])
                W[s, p, :, j] = model.coef_
    path = os.path.join(HERE, "slim_golden.npz")
    np.savez_compressed(path, X=X.astype(np.float32), l1=np.array([a for a, _ in SETTINGS]), l2=np.array([b for _, b in SETTINGS]),
                        W=W)
    print(os.path.getsize(path), "bytes; nonzero share", float((W != 0).mean()))


if __name__ == "__main__":
    main()
