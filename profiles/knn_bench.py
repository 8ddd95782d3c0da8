"""Item-item nearest-neighbour fit and recommend on the device (imp_sparse_topk_product, csrc/knn.hip).

    python profiles/knn_bench.py [--reps 3] [--out DIR] [--no-cpu] [--configs lastfm360k,ml20m]

Per dataset (the synthetic lastfm360k and ml20m shapes) and model (Cosine, BM25; K = 20), prints the fit time (host clock
around model.fit: weighting, transpose, upload, the product, the similarity CSR), the time of the device call alone, and
the achieved products/s against sum_r w_r (w_r = sum over A[r] of nnz(B[u]): every multiply-add of the product).  A
separate pass with the library profiler on gives the HIP-event time of each kernel class (knn_hash: every row in an LDS
table; knn_dense: the rows past the table's limit, dense accumulators in global memory).  recommend is timed at batches of 10 000 users, N = 10.  Where build/refsuite exists, the reference's CPU
all_pairs_knn at 16 threads is timed on the same weighted matrix (--no-cpu skips it)."""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = os.path.join(ROOT, "build", "refsuite")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

K = 20
KERNELS = ("knn_hash", "knn_dense")

_CPU_SCRIPT = r"""
import sys, time, warnings
from scipy.sparse import load_npz
warnings.simplefilter("ignore")
from implicit.nearest_neighbours import all_pairs_knn
w = load_npz(sys.argv[1]).tocsr()
t0 = time.perf_counter()
all_pairs_knn(w, int(sys.argv[2]), num_threads=16, show_progress=False)
print((time.perf_counter() - t0) * 1e3)
"""


def products(items, users):
    blen = np.diff(users.indptr).astype(np.int64)
    return int(blen[items.indices].sum())


def cpu_ms(w):
    import tempfile

    from scipy.sparse import save_npz

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "knn_w.npz")
        save_npz(path, w)
        env = dict(os.environ, PYTHONPATH=SUITE, OMP_NUM_THREADS="16")
        out = subprocess.run([sys.executable, "-c", _CPU_SCRIPT, path, str(K)], env=env, capture_output=True, text=True,
                             timeout=1800)
    return float(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--configs", default="lastfm360k,ml20m")
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
        from implicit_amd import nearest_neighbours as nn
        from implicit_amd import synthetic
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    results = []
    for name in a.configs.split(","):
        counts = synthetic.named(name).astype(np.float64)
        for kind, cls in (("cosine", nn.CosineRecommender), ("bm25", nn.BM25Recommender)):
            model = cls(K=K)
            w = (nn.normalize(counts.T).T if kind == "cosine" else nn.bm25_weight(counts.T, model.K1, model.B).T).tocsr()
            items = w.T.tocsr()
            prods = products(items, w)
            A, B = gpu.SpMat(items), gpu.SpMat(w)
            gpu.sparse_topk_product(A, B, K)  # warm-up: workspaces, code objects
            dev = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, _, counts_out = gpu.sparse_topk_product(A, B, K)
                dev.append((time.perf_counter() - t0) * 1e3)
            fits = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    model.fit(counts, show_progress=False)
                fits.append((time.perf_counter() - t0) * 1e3)
            gpu.Profiler.reset()
            gpu.Profiler.enable(True, only="knn")
            gpu.sparse_topk_product(A, B, K)
            gpu.Profiler.enable(False)
            per_kernel = {k: gpu.Profiler.get(k)[0] for k in KERNELS}
            # recommend: batches of 10 000 users, N = 10
            users = np.arange(min(10_000, counts.shape[0]))
            batch = counts[users]
            model.recommend(users, batch, N=10)
            t0 = time.perf_counter()
            for _ in range(a.reps):
                model.recommend(users, batch, N=10)
            rec_s = (time.perf_counter() - t0) / a.reps
            r = {"dataset": name, "model": kind, "K": K, "items": counts.shape[1], "products": prods,
                 "fit_ms": min(fits), "device_ms": min(dev), "products_per_s": prods / (min(dev) * 1e-3),
                 "kernel_ms": per_kernel, "rows_at_K": int((counts_out == K).sum()),
                 "recommend_users_per_s": len(users) / rec_s}
            if not a.no_cpu and os.path.isdir(SUITE):
                r["reference_cpu16_ms"] = cpu_ms(w)
            print(json.dumps(r), flush=True)
            results.append(r)
            del A, B
    if a.out:
        with open(os.path.join(a.out, "knn_bench.json"), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
