"""AlternatingLeastSquares.explain_batch (csrc/explain.hip): explanations per second for a batch of users.

    python profiles/explain_bench.py [--factors 64,128] [--users 1024] [--items 10] [--reps 5] [--out DIR]

Model: a short ALS fit (2 iterations) on the BASELINE configs[2]-shaped synthetic matrix (358 868 users x 292 385 items,
17.5 M nonzeros).  Workload: the top --items recommendations (recommend, N = --items) of the first --users users, each explained
with N = 10 contributions: B x M (user, item) pairs in one explain_batch call.

Per factor count: explain_batch with a fresh factorisation (factor kernel + contribution kernel) and with the user_weights of
an earlier call passed back (contribution kernel only), and for scale recalculate_user for the same users (the Cholesky fold-in:
the same normal matrices, factorised and solved once per user).  Every time is a host clock around one synchronous call,
uploads of the rows and downloads of the results included, after one warm-up call; the median of --reps calls with the minimum
and maximum beside it.  One JSON line per measurement, a table at the end."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHAPE = (358_868, 292_385, 17_500_000, 3.0)  # users, items, nonzeros, gamma
N = 10


def timed(fn, reps):
    fn()  # warm-up: code objects, workspaces
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", default="64,128")
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--items", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
        from implicit_amd.als import AlternatingLeastSquares
        from implicit_amd.synthetic import synthetic_csr
    if not gpu.HAS_CUDA:
        raise SystemExit("explain_bench: no usable device (there is nothing to measure without one)")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    results, lines = [], []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    users, items, nnz, gamma = SHAPE
    t0 = time.perf_counter()
    C = synthetic_csr(users, items, nnz, gamma=gamma, seed=42)
    print(f"# matrix {C.shape}, nnz {C.nnz}, generated in {time.perf_counter() - t0:.1f} s", flush=True)
    userids = np.arange(a.users)
    rows = C[userids]
    lengths = np.diff(rows.indptr)
    pairs = a.users * a.items
    for f in (int(x) for x in a.factors.split(",")):
        model = AlternatingLeastSquares(factors=f, iterations=2, random_state=1, use_gpu=True)
        model.fit(C, show_progress=False)
        ids, _ = model.recommend(userids, rows, N=a.items)
        base = {"factors": f, "users": a.users, "items_per_user": a.items, "n": N, "row_nnz_mean": float(lengths.mean()),
                "row_nnz_max": int(lengths.max())}
        lines.append(f"f = {f}: {a.users} users x {a.items} items, N = {N}; rows of {lengths.mean():.1f} nonzeros on average, "
                     f"{int(lengths.max())} at most")
        (_, _, _, W), ms, lo, hi = timed(lambda: model.explain_batch(userids, rows, ids, N=N), a.reps)
        emit(dict(base, what="explain_batch", ms=ms, ms_min=lo, ms_max=hi, explanations_per_s=pairs / (ms * 1e-3)))
        lines.append(f"  explain_batch, fresh weights   {ms:9.2f} ms [{lo:.2f} .. {hi:.2f}]  {pairs / ms:9.1f} K explanations/s")
        _, ms, lo, hi = timed(lambda: model.explain_batch(userids, rows, ids, N=N, user_weights=W), a.reps)
        emit(dict(base, what="explain_batch_reused_weights", ms=ms, ms_min=lo, ms_max=hi, explanations_per_s=pairs / (ms * 1e-3)))
        lines.append(f"  explain_batch, reused weights  {ms:9.2f} ms [{lo:.2f} .. {hi:.2f}]  {pairs / ms:9.1f} K explanations/s")
        # the two kernels alone: HIP events around their launches (imp_prof), in a call of its own
        gpu.Profiler.enable(True)
        gpu.Profiler.reset()
        model.explain_batch(userids, rows, ids, N=N)
        k_factor, k_contrib = gpu.Profiler.get("explain_factor")[0], gpu.Profiler.get("explain_contributions")[0]
        gpu.Profiler.enable(False)
        emit(dict(base, what="kernels", explain_factor_ms=k_factor, explain_contributions_ms=k_contrib))
        lines.append(f"  kernels alone: factor {k_factor:.2f} ms, contributions {k_contrib:.2f} ms")
        _, ms, lo, hi = timed(lambda: model.recalculate_user(userids, rows).to_numpy(), a.reps)
        emit(dict(base, what="recalculate_user", ms=ms, ms_min=lo, ms_max=hi, users_per_s=a.users / (ms * 1e-3)))
        lines.append(f"  recalculate_user (for scale)   {ms:9.2f} ms [{lo:.2f} .. {hi:.2f}]  {a.users / ms:9.1f} K users/s")
        del model, W
        gpu.release_workspaces()
    print("\n".join(lines), flush=True)
    if a.out:
        with open(os.path.join(a.out, "explain_bench.json"), "w") as f:
            json.dump(results, f, indent=1)
        with open(os.path.join(a.out, "explain_bench_table.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
