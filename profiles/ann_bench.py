"""IVF-Flat index (implicit_amd.gpu.IVFIndex, csrc/ivf.hip) against the exact scorer KnnQuery.topk on the same inputs.

    python profiles/ann_bench.py [--shapes lastfm360k,1m,4m] [--reps 5] [--batch 16384] [--out DIR]

Factors come from a short ALS fit (f = 128, 2 iterations) on a synthetic matrix of the shape: random factors have no
clusters.  Shapes: lastfm360k (BASELINE configs[2]: 358 868 users x 292 385 items), 1m (1 M users x 1 M items, 40 M
nonzeros: the item count of configs[3]) and 4m (1 M users x 4 M items, 60 M nonzeros).  Queries: the first --batch user
factors, k = 10, no filters.

Per shape: KnnQuery.topk's time on the batch (the yardstick; its code is not part of the index), and per nlist in
{400, 1024, 4096} the build time (10 k-means rounds, host clock around IVFIndex.build, factors already on the device) and
per nprobe the search time and recall@10 against KnnQuery.topk's ids.  Every time is a host clock around one synchronous
call with the results copied to host arrays, after one warm-up call; the median of --reps calls with the minimum and maximum
beside it.  One JSON line per measurement, a table at the end."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

K = 10
FACTORS = 128
SHAPES = {  # users, items, nonzeros, gamma
    "lastfm360k": (358_868, 292_385, 17_500_000, 3.0),
    "1m": (1_000_000, 1_000_000, 40_000_000, 2.0),
    "4m": (1_000_000, 4_000_000, 60_000_000, 2.0),
}
GRID = {400: (5, 20, 50), 1024: (8, 32, 64), 4096: (16, 64, 128)}


def timed(fn, reps):
    fn()  # warm-up: code objects, workspaces
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ms)), float(min(ms)), float(max(ms))


def recall(ids, exact):
    return float((ids[:, :, None] == exact[:, None, :]).any(axis=2).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="lastfm360k,1m,4m")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
        from implicit_amd.als import AlternatingLeastSquares
        from implicit_amd.synthetic import synthetic_csr
    if not gpu.HAS_CUDA:
        raise SystemExit("ann_bench: no usable device (there is nothing to measure without one)")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    results, lines = [], []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    for name in a.shapes.split(","):
        users, items, nnz, gamma = SHAPES[name]
        t0 = time.perf_counter()
        C = synthetic_csr(users, items, nnz, gamma=gamma, seed=42)
        model = AlternatingLeastSquares(factors=FACTORS, iterations=2, random_state=1, use_gpu=True)
        model.fit(C, show_progress=False)
        print(f"# {name}: matrix {C.shape}, nnz {C.nnz}, generated and fitted in {time.perf_counter() - t0:.1f} s", flush=True)
        Y = model.item_factors
        Q = model.user_factors[0:a.batch]
        zero_items = int((gpu.calculate_norms(Y).to_numpy() <= 1e-10).sum())
        del C
        knn = gpu.KnnQuery()
        (exact, _), ms, lo, hi = timed(lambda: knn.topk(Y, Q, K), a.reps)
        base = {"shape": name, "items": items, "factors": FACTORS, "batch": a.batch, "k": K, "zero_items": zero_items}
        emit(dict(base, what="KnnQuery.topk", ms=ms, ms_min=lo, ms_max=hi, queries_per_s=a.batch / (ms * 1e-3)))
        lines.append(f"{name}: {items} items, f = {FACTORS}, batch {a.batch}, k = {K}; {zero_items} items with a zero factor row")
        lines.append(f"  KnnQuery.topk (exact)              {ms:9.2f} ms [{lo:.2f} .. {hi:.2f}]  {a.batch / ms / 1e3:8.3f} M queries/s")
        exact_ms = ms
        for nlist, probes in GRID.items():
            init = np.random.default_rng(nlist).choice(items, size=nlist, replace=False)
            builds = []
            for _ in range(2):
                gpu.synchronize()
                t0 = time.perf_counter()
                ix = gpu.IVFIndex.build(Y, nlist, 10, init_rows=init)
                builds.append((time.perf_counter() - t0) * 1e3)
            sizes = np.diff(ix.list_offsets)
            emit(dict(base, what="build", nlist=nlist, build_ms=min(builds), build_ms_first=builds[0],
                      longest_list=int(sizes.max()), empty_lists=int((sizes == 0).sum())))
            lines.append(f"  nlist {nlist:5d}: build {min(builds):9.1f} ms (10 rounds), longest list {int(sizes.max())}, "
                         f"{int((sizes == 0).sum())} empty")
            for nprobe in probes:
                (ids, _), ms, lo, hi = timed(lambda: ix.search(Q, K, nprobe), a.reps)
                rec = recall(ids, exact)
                emit(dict(base, what="search", nlist=nlist, nprobe=nprobe, ms=ms, ms_min=lo, ms_max=hi,
                          queries_per_s=a.batch / (ms * 1e-3), recall_at_10=rec, speedup_vs_exact=exact_ms / ms))
                lines.append(f"    nprobe {nprobe:4d}                     {ms:9.2f} ms [{lo:.2f} .. {hi:.2f}]  {a.batch / ms / 1e3:8.3f} M queries/s"
                             f"  recall@10 {rec:.4f}  x{exact_ms / ms:.2f} of exact")
            del ix
        del model, Y, Q, knn
        gpu.release_workspaces()
    print("\n".join(lines), flush=True)
    if a.out:
        with open(os.path.join(a.out, "ann_bench.json"), "w") as f:
            json.dump(results, f, indent=1)
        with open(os.path.join(a.out, "ann_bench_table.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
