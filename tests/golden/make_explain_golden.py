#!/usr/bin/env python3
"""Generates tests/golden/explain_golden.npz from the REFERENCE ITSELF: AlternatingLeastSquares.explain of the CPU model
(implicit.cpu.als) of the package assembled by oracle/refsuite.py in build/refsuite.  Run in the build container only (the
reference tree is not on the GPU box):

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_explain_golden.py

Two models are fitted by the reference and their explanations recorded:

    m0  the 7 x 6 counts matrix of the reference's own explain test, transposed to 6 users x 7 items as there:
        factors 4, regularization 20, alpha 2, Cholesky, 100 iterations, random_state 23
    m1  synthetic_csr(60, 80, 700, seed=3, neg_frac=0.1) (a tenth of the entries disliked): factors 16, regularization 0.05,
        alpha 1.5, Cholesky, 5 iterations, random_state 7

Arrays per model k: m<k>_X, m<k>_Y (the fitted float32 factors), m<k>_indptr / _indices / _data (the users x items matrix
BEFORE alpha), m<k>_params = (regularization, alpha); `cases`, one JSON string per explained pair (model, user, item, N); and
c<i>_total, c<i>_ids, c<i>_scores, what the reference returned (float64 scores).  Fixed zip timestamps: the same reference
reproduces the file byte for byte.
"""
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "build", "refsuite"))
sys.path.insert(1, ROOT)

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    from implicit.cpu.als import AlternatingLeastSquares  # noqa: E402

from implicit_amd.synthetic import synthetic_csr  # noqa: E402  host-only numpy

counts = csr_matrix([[1, 1, 0, 1, 0, 0],
                     [0, 1, 1, 1, 0, 0],
                     [1, 4, 1, 0, 7, 0],
                     [1, 1, 0, 0, 0, 0],
                     [9, 0, 4, 1, 0, 1],
                     [0, 1, 0, 0, 0, 1],
                     [0, 0, 2, 0, 1, 1]], dtype=np.float32)

MODELS = [
    dict(user_items=counts.T.tocsr(), factors=4, regularization=20.0, alpha=2.0, iterations=100, random_state=23,
         pairs=[(0, None, 10), (0, 5, 10), (2, 3, 10), (4, 0, 2), (5, 6, 1), (1, 1, 10)]),
    dict(user_items=synthetic_csr(60, 80, 700, seed=3, neg_frac=0.1), factors=16, regularization=0.05, alpha=1.5, iterations=5,
         random_state=7, pairs=[(0, 3, 10), (7, 79, 10), (13, 0, 3), (21, 40, 10), (33, 12, 1), (59, 79, 25), (45, None, 10)]),
]

out, cases = {}, []
for k, spec in enumerate(MODELS):
    user_items = spec["user_items"]
    model = AlternatingLeastSquares(factors=spec["factors"], regularization=spec["regularization"], alpha=spec["alpha"],
                                    use_native=False, use_cg=False, iterations=spec["iterations"],
                                    random_state=spec["random_state"], num_threads=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit(user_items, show_progress=False)
    out[f"m{k}_X"], out[f"m{k}_Y"] = model.user_factors.astype(np.float32), model.item_factors.astype(np.float32)
    out[f"m{k}_indptr"], out[f"m{k}_indices"], out[f"m{k}_data"] = user_items.indptr, user_items.indices, user_items.data
    out[f"m{k}_params"] = np.array([spec["regularization"], spec["alpha"]], dtype=np.float64)
    for user, item, N in spec["pairs"]:
        if item is None:  # the reference test's own pair: the top recommendation with a recalculated user
            ids, _ = model.recommend(user, user_items[user], N=3, recalculate_user=True)
            item = int(ids[0])
        total, top, _ = model.explain(user, user_items, item, N=N)
        i = len(cases)
        cases.append(json.dumps(dict(model=k, user=user, item=item, N=N), sort_keys=True))
        out[f"c{i}_total"] = np.float64(total)
        out[f"c{i}_ids"] = np.array([t[0] for t in top], dtype=np.int64)
        out[f"c{i}_scores"] = np.array([t[1] for t in top], dtype=np.float64)
out["cases"] = np.array(cases)

path = os.path.join(HERE, "explain_golden.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
    for name in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[name]), allow_pickle=False)
        info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        z.writestr(info, buf.getvalue())
print("wrote", path, len(out), "arrays,", len(cases), "cases,", os.path.getsize(path), "bytes")
