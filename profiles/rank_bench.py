"""rank_items (csrc/rank.hip) against the only route the package had before it: one recommend(items=list) call per user.

    python profiles/rank_bench.py [--users 16384] [--loop-users 256] [--reps 5] [--out DIR]

Item factors of the configs[2] shape (292 385 x 128, fp32, seeded standard_normal * 0.1: scoring given candidates does not
depend on structure in the factors), --users users, every user with its own list of M random item ids, given as a [users, M]
int32 array.  Cases: M in {100, 500, 4096} at N = M, M = 20 000 at N = 100, and 1 user x 500.

Every time is a host clock around one synchronous call with the results in host arrays, after one warm-up call: the median of
--reps calls with the minimum and maximum beside it.  The yardstick is a loop of
recommend(u, None, N, filter_already_liked_items=False, items=list_u) over the first --loop-users users, timed the same way
as ONE measurement and reported per user.  The kernel alone is timed by HIP events (imp_prof) in a call of its own.  The floor
is the gather alone: M * w * 4 bytes per user at 6.3 TB/s.
One JSON line per case on stdout; the table goes to rank_bench.txt in --out (default: this directory)."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ITEMS, FACTORS = 292_385, 128
HBM_BYTES_PER_S = 6.3e12
CASES = ((100, 100), (500, 500), (4096, 4096), (20_000, 100))  # (M, N)


def timed(fn, reps):
    fn()  # warm-up: code objects, allocator free lists
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ms)), float(min(ms)), float(max(ms))


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
    if not gpu.HAS_CUDA:
        raise SystemExit("rank_bench: no usable device (there is nothing to measure without one)")
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(7)
    model = AlternatingLeastSquares(factors=FACTORS)
    model.item_factors = gpu.Matrix((rng.standard_normal((ITEMS, FACTORS)) * 0.1).astype(np.float32))
    model.user_factors = gpu.Matrix((rng.standard_normal((a.users, FACTORS)) * 0.1).astype(np.float32))
    users = np.arange(a.users)
    lines = [f"{ITEMS} items x {FACTORS} fp32, {a.users} users, lists of M random ids; median of {a.reps} [min .. max], host clock;",
             "kernel: HIP events around the rank kernel in a call of its own; floor: M * w * 4 bytes per user at 6.3 TB/s",
             f"{'case':28s} {'rank_items, whole call':>34s} {'per user':>11s} {'kernel, per user':>17s} {'floor':>9s} "
             f"{'recommend loop, per user':>32s}"]

    def kernel_ms(fn):
        """The rank kernel alone: HIP events around its launches (imp_prof), in a call of its own."""
        gpu.Profiler.enable(True)
        gpu.Profiler.reset()
        fn()
        ms = gpu.Profiler.get("rank")[0]
        gpu.Profiler.enable(False)
        return ms

    def case(label, n_users, M, N, rank, n_loop, loop):
        (ids, _), ms, lo, hi = timed(rank, a.reps)
        assert ids.shape[-1] == N
        k_ms = kernel_ms(rank)
        _, lms, llo, lhi = timed(loop, a.reps)
        floor_us = M * FACTORS * 4 / HBM_BYTES_PER_S * 1e6
        print(json.dumps(dict(users=n_users, M=M, N=N, rank_items_ms=ms, rank_items_ms_min=lo, rank_items_ms_max=hi,
                              rank_items_us_per_user=ms * 1e3 / n_users, kernel_ms=k_ms, kernel_us_per_user=k_ms * 1e3 / n_users,
                              gather_floor_us_per_user=floor_us, loop_users=n_loop, loop_ms=lms, loop_ms_min=llo, loop_ms_max=lhi,
                              loop_us_per_user=lms * 1e3 / n_loop)), flush=True)
        lines.append(f"{label:28s} {ms:11.3f} ms [{lo:.3f} .. {hi:.3f}] {ms * 1e3 / n_users:8.2f} us {k_ms * 1e3 / n_users:14.3f} us "
                     f"{floor_us:6.3f} us {lms * 1e3 / n_loop:10.1f} us [{llo * 1e3 / n_loop:.1f} .. {lhi * 1e3 / n_loop:.1f}]")

    def loop_of(n_users, lists, N):
        def run():
            for u in range(n_users):
                model.recommend(u, None, N=N, filter_already_liked_items=False, items=lists[u])
        return run

    n_loop = min(a.loop_users, a.users)
    for M, N in CASES:
        lists = rng.integers(0, ITEMS, size=(a.users, M), dtype=np.int32)
        case(f"{a.users} users, M {M}, N {N}", a.users, M, N, lambda: model.rank_items(users, None, lists, N=N), n_loop,
             loop_of(n_loop, lists, N))
        del lists
    one = rng.integers(0, ITEMS, size=500, dtype=np.int32)
    case("1 user, M 500, N 500", 1, 500, 500, lambda: model.rank_items(0, None, one, N=500), 1, loop_of(1, [one], 500))
    print("\n".join(lines), flush=True)
    with open(os.path.join(a.out, "rank_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
