#!/usr/bin/env python3
"""Generates tests/golden/lmf_golden.npz from the REFERENCE ITSELF: implicit.cpu.lmf.lmf_update, the compiled Cython module
of the reference package assembled by oracle/refsuite.py in build/refsuite.  Run in the build container only (the
reference tree is not on the GPU box):

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_lmf_golden.py

Two kinds of case:
  np0_*   neg_prop = 0 half-sweeps (no random draws: deterministic, the same for any thread count), two consecutive calls
          so that the second one starts from a non-zero Adagrad accumulator; rows without a nonzero and confidences other
          than 1.  Arrays: indptr / indices / data / shape, X0, Y, lr, reg, then X1, G1 (after the first call) and X2, G2
          (after the second).
  kprobe  the negative-count probe: all confidences 0, Y = 1, X = 0, reg = 0 -- then G[u] = (K/2)^2 for every column,
          whatever the draws.  Rows of 1, 5 and 20 nonzeros at C = 7 and neg_prop 1, 2, 30 (G_np<neg_prop>).
"""
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SUITE = os.path.join(ROOT, "build", "refsuite")
sys.path.insert(0, ROOT)
sys.path.insert(0, SUITE)

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    from implicit.cpu.lmf import RNGVector, lmf_update  # noqa: E402

out = {}


def put_csr(prefix, m):
    out[prefix + "_indptr"] = m.indptr.astype(np.int32)
    out[prefix + "_indices"] = m.indices.astype(np.int32)
    out[prefix + "_data"] = m.data.astype(np.float32)
    out[prefix + "_shape"] = np.array(m.shape, dtype=np.int64)


def ref_update(m, X, Y, G, lr, reg, neg_prop, seed=1):
    rng = RNGVector(1, max(m.nnz - 1, 0), np.array([seed], dtype="long"))
    lmf_update(rng, G, X, Y, m.indices.astype(np.int32), m.indptr.astype(np.int32), m.data.astype(np.float32),
               np.float32(lr), np.float32(reg), neg_prop, 1)


# ---- neg_prop = 0 half-sweeps: (name, rows, other, nnz, C, lr, reg) ----------------------------------------------------
cases = [("np0_c5", 50, 40, 500, 5, 1.0, 0.6), ("np0_c32", 80, 120, 1500, 32, 0.5, 0.1), ("np0_c66", 60, 70, 900, 66, 1.0, 0.6)]
rng = np.random.default_rng(2024)
for name, rows, other, nnz, C, lr, reg in cases:
    r = rng.integers(0, rows, nnz)
    c = rng.integers(0, other, nnz)
    keep = r % 7 != 3  # every seventh row empty
    m = sp.csr_matrix((rng.uniform(0.5, 3.0, keep.sum()).astype(np.float32), (r[keep], c[keep])), shape=(rows, other))
    m.sum_duplicates()
    m.sort_indices()
    X = (rng.standard_normal((rows, C)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((other, C)) * 0.5).astype(np.float32)
    put_csr(name, m)
    out[name + "_X0"], out[name + "_Y"] = X.copy(), Y
    out[name + "_lr"], out[name + "_reg"] = np.float32(lr), np.float32(reg)
    G = np.zeros_like(X)
    for step in (1, 2):
        ref_update(m, X, Y, G, lr, reg, 0)
        out[f"{name}_X{step}"], out[f"{name}_G{step}"] = X.copy(), G.copy()

# ---- the negative-count probe -------------------------------------------------------------------------------------------
C = 7
lens = [1, 5, 20]
indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
m = sp.csr_matrix((np.zeros(indptr[-1], np.float32), np.arange(indptr[-1], dtype=np.int32) % 30, indptr), shape=(3, 30))
put_csr("kprobe", m)
out["kprobe_C"] = np.int64(C)
for neg_prop in (1, 2, 30):
    X, Y, G = np.zeros((3, C), np.float32), np.ones((30, C), np.float32), np.zeros((3, C), np.float32)
    ref_update(m, X, Y, G, 1.0, 0.0, neg_prop, seed=5)
    out[f"kprobe_G_np{neg_prop}"] = G

np.savez_compressed(os.path.join(HERE, "lmf_golden.npz"), **out)
print("wrote", os.path.join(HERE, "lmf_golden.npz"), len(out), "arrays")
