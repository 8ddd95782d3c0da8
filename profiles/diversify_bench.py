"""diversify_items (csrc/diversify.hip) against the only route a user had before it: the same greedy in float32 numpy, one user
at a time.

    python profiles/diversify_bench.py [--users 16384] [--loop-users 256] [--reps 5] [--out DIR]

Item factors of the configs[2] shape (292 385 x 128, fp32, seeded standard_normal * 0.1), --users users, every user with its own
list of M random item ids as a [users, M] int32 array.  Cases: M in {100, 500, 2000} x N in {10, 50}, both rules.  M = 100 and
500 run on the resident path (rows in registers), M = 2000 on the streamed one.

Every time is a host clock around one synchronous diversify_items call (scores, qualities and the re-rank) with the results in
host arrays, after one warm-up call: the median of --reps calls with the minimum and maximum beside it.  The kernel alone is
timed by HIP events (imp_prof) in a call of its own.  The yardstick is tests/diversify_reference.greedy in float32 over the first
--loop-users users on the scores the model returns, ONE measurement, reported per user.  The floor is the gather alone at
6.3 TB/s: M * w * 4 bytes per user on the resident path, N times that on the streamed one.
One JSON line per case on stdout; the table goes to diversify_bench.txt in --out (default: this directory)."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

ITEMS, FACTORS = 292_385, 128
HBM_BYTES_PER_S = 6.3e12
RESIDENT = 512  # longest list kept in registers at w = 128
WEIGHT = 0.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=16384)
    ap.add_argument("--loop-users", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
        from implicit_amd.gpu.als import AlternatingLeastSquares
    import diversify_reference as ref
    if not gpu.HAS_CUDA:
        raise SystemExit("diversify_bench: no usable device (there is nothing to measure without one)")
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(7)
    Y = (rng.standard_normal((ITEMS, FACTORS)) * 0.1).astype(np.float32)
    model = AlternatingLeastSquares(factors=FACTORS)
    model.item_factors = gpu.Matrix(Y)
    model.user_factors = gpu.Matrix((rng.standard_normal((a.users, FACTORS)) * 0.1).astype(np.float32))
    users, n_loop = np.arange(a.users), min(a.loop_users, a.users)
    lines = [f"{ITEMS} items x {FACTORS} fp32, {a.users} users, lists of M random ids, relevance_weight {WEIGHT}; median of {a.reps} "
             "[min .. max], host clock;",
             "kernel: HIP events around the diversify kernel in a call of its own; floor: the gather at 6.3 TB/s (streamed: N gathers);",
             f"numpy: the float32 restatement, one user at a time over {n_loop} users, one measurement",
             f"{'case':24s} {'diversify_items, whole call':>36s} {'per user':>11s} {'kernel, per user':>17s} {'floor':>9s} "
             f"{'numpy, per user':>16s}"]
    for M in (100, 500, 2000):
        lists = rng.integers(0, ITEMS, size=(a.users, M), dtype=np.int32)
        scores = model.score_items(users[:n_loop], lists[:n_loop])
        for N in (10, 50):
            for rule in ("dpp", "mmr"):
                call = lambda: model.diversify_items(users, None, lists, N, rule=rule, relevance_weight=WEIGHT)  # noqa: E731
                call()  # warm-up: code objects, allocator free lists
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ids, _ = call()
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert ids.shape == (a.users, N)
                gpu.Profiler.enable(True)
                gpu.Profiler.reset()
                call()
                k_ms = gpu.Profiler.get("diversify")[0]
                gpu.Profiler.enable(False)
                t0 = time.perf_counter()
                for u in range(n_loop):
                    s = scores[u].astype(np.float64)
                    q = np.exp(WEIGHT / (2 * (1 - WEIGHT)) * (s - s.max())) if rule == "dpp" else s
                    ref.greedy(Y, lists[u], q, N, rule, param=WEIGHT, dtype=np.float32)
                loop_us = (time.perf_counter() - t0) * 1e6 / n_loop
                med, lo, hi = float(np.median(ms)), min(ms), max(ms)
                floor_us = M * FACTORS * 4 * (1 if M <= RESIDENT else N) / HBM_BYTES_PER_S * 1e6
                print(json.dumps(dict(users=a.users, M=M, N=N, rule=rule, call_ms=med, call_ms_min=lo, call_ms_max=hi,
                                      call_us_per_user=med * 1e3 / a.users, kernel_ms=k_ms, kernel_us_per_user=k_ms * 1e3 / a.users,
                                      floor_us_per_user=floor_us, loop_users=n_loop, numpy_us_per_user=loop_us)), flush=True)
                lines.append(f"{f'M {M}, N {N}, {rule}':24s} {med:11.3f} ms [{lo:.3f} .. {hi:.3f}] {med * 1e3 / a.users:8.2f} us "
                             f"{k_ms * 1e3 / a.users:14.3f} us {floor_us:6.3f} us {loop_us:13.1f} us")
        del lists
    print("\n".join(lines), flush=True)
    with open(os.path.join(a.out, "diversify_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
