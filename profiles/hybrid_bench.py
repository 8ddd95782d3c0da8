"""Hybrid WARP epoch throughput on the device (imp_hybrid_warp_update, csrc/hybrid_warp.hip), beside WARP's.

    python profiles/hybrid_bench.py [--out DIR] [--only shape,...] [--factors F]

Feature matrices are the identity plus k random tag features per row (weights 1.0, 1000 tags per side), k = 0, 4 and 16: at
k = 0 the model is WARP's, so the first row of every shape is the overhead of going through feature rows at all.  For every
shape (the lastfm360k and ml20m synthetic shapes) it trains three epochs per configuration from WARP's initial factors scaled
by 1 / (k + 1) (learning rate 0.02, regularization 0.01, max_sampled 10) and prints, for the first and the third epoch: ms
per epoch (host clock around the synchronous call), samples/s, mean trials per sample, and the HIP-event time of the update
kernel -- then the same for imp_warp_update in the same process.  Every epoch is timed on its own, after one untimed
single-sample call that loads the kernel.  Not a test; no speed is promised."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from scipy.sparse import csr_matrix  # noqa: E402

SHAPES = ("lastfm360k", "ml20m")
TAGS_PER_ROW = (0, 4, 16)
TAGS = 1000
LR, REG, MAX_SAMPLED, EPOCHS = 0.02, 0.01, 10, 3


def tagged_identity(rows, k, rng):
    """rows x (rows + TAGS): the row's own feature and k random tags, one from each of k equal blocks of the tags (distinct and
    sorted by construction), weights 1.0."""
    tags = rows + (np.arange(k) * (TAGS // max(k, 1)))[None, :] + rng.integers(0, TAGS // max(k, 1), (rows, k))
    cols = np.concatenate([np.arange(rows)[:, None], tags], axis=1).astype(np.int32)
    return csr_matrix((np.ones(cols.size, dtype=np.float32), cols.ravel(), (k + 1) * np.arange(rows + 1)), shape=(rows, rows + TAGS))


def _init(rows, factors, rng, scale, bias=None):
    E = (rng.random((rows, factors + 1), "float32") - 0.5) / factors * np.float32(scale)
    if bias is not None:
        E[:, factors] = bias
    return E


def _epochs(gpu, scope, results, row, nnz, call):
    gpu.Profiler.enable(True, only=scope)
    for e in range(EPOCHS):
        gpu.Profiler.reset()
        t0 = time.perf_counter()
        _, trials = call(1000 + e)
        wall = time.perf_counter() - t0
        if e in (0, EPOCHS - 1):
            r = dict(row, epoch=e + 1, nnz=nnz, ms_per_epoch=round(wall * 1e3, 3), samples_per_s=round(nnz / wall),
                     trials_per_sample=round(trials / nnz, 3), update_kernel_ms=round(gpu.Profiler.get(scope)[0], 3))
            results.append(r)
            print(json.dumps(r), flush=True)
    gpu.Profiler.enable(False)


def run(shapes, factors):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("hybrid_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.synthetic import named

    results = []
    for name in shapes:
        m = named(name)
        users, items = m.shape
        userids = np.repeat(np.arange(users, dtype=np.int32), np.diff(m.indptr))
        ids = gpu.IntVector(userids), gpu.IntVector(m.indices), gpu.IntVector(m.indptr.astype(np.int32))
        for k in TAGS_PER_ROW:
            rng = np.random.default_rng(7)
            UF, IF = gpu.CSRMatrix(tagged_identity(users, k, rng)), gpu.CSRMatrix(tagged_identity(items, k, rng))
            EI = gpu.Matrix(_init(items + TAGS, factors, rng, 1.0 / (k + 1)))
            EU = gpu.Matrix(_init(users + TAGS, factors, rng, 1.0 / (k + 1), bias=1.0))
            gpu.hybrid_warp_epoch(*ids, UF, IF, EU, EI, 0.0, 0.0, 0, MAX_SAMPLED, samples=1)  # loads the kernel; a zero step
            _epochs(gpu, "hybrid_warp_update", results, {"model": "hybrid", "shape": name, "factors": factors, "tags_per_row": k}, int(m.nnz),
                    lambda seed: gpu.hybrid_warp_epoch(*ids, UF, IF, EU, EI, LR, REG, seed, MAX_SAMPLED))
            del UF, IF, EU, EI
        rng = np.random.default_rng(7)
        Y, X = gpu.Matrix(_init(items, factors, rng, 1.0)), gpu.Matrix(_init(users, factors, rng, 1.0, bias=1.0))
        gpu.warp_epoch(*ids, X, Y, 0.0, 0.0, 0, MAX_SAMPLED, samples=1)
        _epochs(gpu, "warp_update", results, {"model": "warp", "shape": name, "factors": factors}, int(m.nnz),
                lambda seed: gpu.warp_epoch(*ids, X, Y, LR, REG, seed, MAX_SAMPLED))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "hybrid_bench"))
    ap.add_argument("--only", default=None, help="shape[,shape...]")
    ap.add_argument("--factors", type=int, default=64)
    a = ap.parse_args()
    results = run(a.only.split(",") if a.only else SHAPES, a.factors)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "hybrid_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
