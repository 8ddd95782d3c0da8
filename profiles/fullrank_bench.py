"""Full-catalogue ranking metrics over a fitted model: implicit_amd.evaluation.full_ranking_metrics (csrc/target_ranks.hip)
beside ranking_metrics_at_k at K = 10, the only evaluation the package had before it.

    python profiles/fullrank_bench.py [--config lastfm360k] [--scale 1.0] [--reps 2] [--out profiles/fullrank_bench.txt]

The set-up is that of profiles/eval_bench.py: the synthetic matrix of the named shape split 80 / 20 (train_test_split, seed 7),
ALS (f = 64) for a few iterations on the train part, the host clock around the whole call (each returns only after its
results are on the host), best of --reps after a warm-up call.  Then one profiled call (HIP events around every launch,
Profiler) gives the per-kernel split, and the dense pass is set against its floor: 2 users items C flops at the 157.3
TFLOP/s of the fp32 matrix pipe (the pass reads Y once per tile of 32 users from the L2; at 16 flops per byte read it is
bound by the pipe, not by HBM).  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_TF = 157.3  # fp32 MFMA
KERNELS = ("target_filter_bits", "target_thresholds", "target_sort", "target_ranks_dense", "target_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="lastfm360k")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
        from implicit_amd import evaluation, synthetic
        from implicit_amd.gpu.als import AlternatingLeastSquares
    if not gpu.HAS_CUDA:
        raise SystemExit("fullrank_bench: no HIP device")
    lines = []

    def emit(r):
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    C = synthetic.named(a.config, scale=a.scale)
    train, test = evaluation.train_test_split(C, 0.8, random_state=7)
    train, test = train.astype(np.float32), test.astype(np.float32)
    model = AlternatingLeastSquares(factors=64, iterations=a.iterations, random_state=11)
    model.fit(train, show_progress=False)
    users = int((np.diff(test.indptr) > 0).sum())
    emit({"config": a.config, "users": C.shape[0], "items": C.shape[1], "train_nnz": int(train.nnz), "test_nnz": int(test.nnz),
          "evaluated_users": users, "factors": 64, "batch_size": evaluation.DEFAULT_BATCH_SIZE})

    def timed(fn):
        fn()  # warm-up: code objects, workspaces
        best, res = None, None
        for _ in range(a.reps):
            gpu.synchronize()
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, res

    Ks = (1, 10, 100)
    top_s, top = timed(lambda: evaluation.ranking_metrics_at_k(model, train, test, K=10, show_progress=False))
    emit({"path": "ranking_metrics_at_k, K = 10", "seconds": top_s, "users_per_s": users / top_s, **top})
    full_s, full = timed(lambda: evaluation.full_ranking_metrics(model, train, test, K=Ks, show_progress=False))
    emit({"path": f"full_ranking_metrics, K = {Ks}", "seconds": full_s, "users_per_s": users / full_s, "ratio_to_topk": full_s / top_s,
          **{k: (v if not isinstance(v, dict) else {str(kk): vv for kk, vv in v.items()}) for k, v in full.items()}})

    gpu.Profiler.enable(True, only="target_")
    gpu.Profiler.reset()
    evaluation.full_ranking_metrics(model, train, test, K=Ks, show_progress=False)
    split = {name: gpu.Profiler.get(name) for name in KERNELS}
    gpu.Profiler.enable(False)
    emit({"part": "per-kernel split of one call (HIP events)", **{k: {"ms": ms, "launches": n} for k, (ms, n) in split.items()}})
    flops = 2.0 * users * C.shape[1] * 64
    dense_s = split["target_ranks_dense"][0] / 1e3
    emit({"part": "dense pass against the fp32 matrix pipe", "flops": flops, "floor_seconds": flops / (PEAK_TF * 1e12),
          "dense_seconds": dense_s, "tflops": flops / dense_s / 1e12, "share_of_peak": flops / dense_s / (PEAK_TF * 1e12),
          "bound": "fp32 MFMA rate"})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
