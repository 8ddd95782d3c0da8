"""PureSVD's kernels and fit on the device (csrc/svd.hip, implicit_amd/svd.py).

    python profiles/svd_bench.py [--out DIR] [--factors 64,128,256] [--reps N] [--cpu-factors 64,128,256] [--limit SECONDS]

On the configs[2]-shaped synthetic matrix (synthetic.named("lastfm360k")) it prints one JSON line per factor count, with the
sketch width l = factors + 10 the model uses, and writes them to DIR/svd_bench.json:
  - spmm alone in both orientations (A Omega -> users x l; A^T Q -> items x l): HIP-event time of its scopes, best and median of
    --reps calls after one untimed call, and the achieved bytes/s over nnz (4 l + 8) + rows 4 l -- every gathered row of the
    dense operand, the row's (column, value) pairs, the output -- beside the micro-architecture guide's 5.5 - 5.8 TB/s for whole
    random rows of 1 - 2 KB gathered by one wave per destination (a reference point, not a pass mark);
  - multiply_small alone (users x l times l x l) as time and TFLOP/s over 2 rows l^2, and the gramian alone (users x l);
  - the driver alone on resident CSR handles, and the whole PureSVD.fit (host transpose and CSR uploads included), on the host
    clock around the synchronous calls.
Afterwards, outside every timed device region, scipy.sparse.linalg.svds of the same matrix on 16 CPU threads for
--cpu-factors, one JSON line each.  One process; SIGALRM ends it after --limit seconds; the first failure ends it."""
import argparse
import json
import os
import signal
import statistics
import sys
import time
import warnings

os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")  # the CPU comparison runs on the 16 CPUs a command may use
os.environ.setdefault("OMP_NUM_THREADS", "16")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GUIDE_GATHER_TBS = (5.5, 5.8)
PEAK_TF = 157.3
OVERSAMPLE, POWER_ITERATIONS = 10, 2
SPMM_SCOPES = ("spmm_long_rows", "spmm_wave_rows", "spmm_group_rows", "zero_rows")
GRAM_SCOPES = ("gramian_partial", "gramian_reduce")


def timed(gpu, scopes, reps, call):
    """(best event ms, median event ms, best wall ms) of `call` over `reps` runs after one untimed run."""
    call()
    gpu.Profiler.enable(True)
    events, walls = [], []
    for _ in range(reps):
        gpu.Profiler.reset()
        t0 = time.perf_counter()
        call()
        walls.append((time.perf_counter() - t0) * 1e3)
        events.append(sum(gpu.Profiler.get(s)[0] for s in scopes))
    gpu.Profiler.enable(False)
    return min(events), statistics.median(events), min(walls)


def spmm_bytes(nnz, rows, width):
    return nnz * (4 * width + 8) + rows * 4 * width


def run(factor_list, reps, out_dir):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("svd_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.svd import PureSVD
    from implicit_amd.synthetic import named, synthetic_csr
    from implicit_amd.utils import transpose_csr

    PureSVD(factors=8, oversample=4).fit(synthetic_csr(300, 64, 3000, seed=1), show_progress=False)  # loads the kernels
    X = named("lastfm360k")
    users, items = X.shape
    Xt = transpose_csr(X)
    A, At = gpu.CSRMatrix(X), gpu.CSRMatrix(Xt)
    solver = gpu.LeastSquaresSolver()
    results = []
    for factors in factor_list:
        width = factors + OVERSAMPLE
        omega = gpu.RandomState(7).randn(items, width)
        Q, Q2, Z = gpu.Matrix.zeros(users, width), gpu.Matrix.zeros(users, width), gpu.Matrix.zeros(items, width)
        W = gpu.Matrix((np.random.default_rng(1).standard_normal((width, width)) / np.sqrt(width)).astype(np.float32))
        G = gpu.Matrix.zeros(width, width)
        fwd = timed(gpu, SPMM_SCOPES, reps, lambda: gpu.spmm(A, omega, out=Q))
        bwd = timed(gpu, SPMM_SCOPES, reps, lambda: gpu.spmm(At, Q, out=Z))
        mul = timed(gpu, ("multiply_small",), reps, lambda: gpu.multiply_small(Q, W, out=Q2))
        gram = timed(gpu, GRAM_SCOPES, reps, lambda: solver.calculate_yty(Q, G, 0.0))
        del Q, Q2, Z, W, G, omega
        driver, fit = [], []
        for _ in range(max(2, reps // 2)):
            t0 = time.perf_counter()
            gpu.randomized_svd(A, At, factors, oversample=OVERSAMPLE, power_iterations=POWER_ITERATIONS, random_state=3)
            driver.append(time.perf_counter() - t0)
        for _ in range(2):
            model = PureSVD(factors=factors, oversample=OVERSAMPLE, power_iterations=POWER_ITERATIONS, random_state=3)
            t0 = time.perf_counter()
            model.fit(X, show_progress=False)
            fit.append(time.perf_counter() - t0)
        fb, bb = spmm_bytes(X.nnz, users, width), spmm_bytes(X.nnz, items, width)
        r = {"shape": "lastfm360k", "users": int(users), "items": int(items), "nnz": int(X.nnz), "factors": factors, "sketch": width,
             "reps": reps,
             "spmm_user_items_ms": round(fwd[0], 3), "spmm_user_items_median_ms": round(fwd[1], 3),
             "spmm_user_items_wall_ms": round(fwd[2], 3), "spmm_user_items_tb_per_s": round(fb / (fwd[0] * 1e-3) / 1e12, 3),
             "spmm_item_users_ms": round(bwd[0], 3), "spmm_item_users_median_ms": round(bwd[1], 3),
             "spmm_item_users_wall_ms": round(bwd[2], 3), "spmm_item_users_tb_per_s": round(bb / (bwd[0] * 1e-3) / 1e12, 3),
             "guide_gather_tb_per_s": list(GUIDE_GATHER_TBS),
             "multiply_small_ms": round(mul[0], 3), "multiply_small_median_ms": round(mul[1], 3),
             "multiply_small_tflops": round(2.0 * users * width * width / (mul[0] * 1e-3) / 1e12, 2),
             "multiply_small_frac_of_fp32_matrix_peak": round(2.0 * users * width * width / (mul[0] * 1e-3) / 1e12 / PEAK_TF, 4),
             "gramian_ms": round(gram[0], 3), "gramian_median_ms": round(gram[1], 3),
             "driver_s": round(min(driver), 4), "driver_all_s": [round(x, 4) for x in driver],
             "fit_s": round(min(fit), 4), "fit_all_s": [round(x, 4) for x in fit],
             "singular_values_head": [round(float(x), 4) for x in model.singular_values[:4]]}
        results.append(r)
        print(json.dumps(r), flush=True)
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "svd_bench.json"), "w") as f:
            json.dump(results, f, indent=1)
        del model
    return X, results


def cpu_baseline(X, cpu_factors, results, out_dir):
    from scipy.sparse.linalg import svds

    for factors in cpu_factors:
        t0 = time.perf_counter()
        s = svds(X, k=factors, return_singular_vectors=True)[1]
        r = {"shape": "lastfm360k", "factors": factors, "cpu_scipy_svds_s": round(time.perf_counter() - t0, 3),
             "cpu_threads": int(os.environ["OPENBLAS_NUM_THREADS"]),
             "cpu_singular_values_head": [round(float(x), 4) for x in np.sort(s)[::-1][:4]]}
        results.append(r)
        print(json.dumps(r), flush=True)
        with open(os.path.join(out_dir, "svd_bench.json"), "w") as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "svd_bench"))
    ap.add_argument("--factors", default="64,128,256")
    ap.add_argument("--cpu-factors", default="64,128,256", help="factor counts of the scipy svds baseline ('' for none)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=1100, help="seconds after which the process ends itself")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"svd_bench: time limit of {a.limit} s reached"))
    signal.alarm(a.limit)
    X, results = run([int(x) for x in a.factors.split(",") if x], a.reps, a.out)
    cpu_baseline(X, [int(x) for x in a.cpu_factors.split(",") if x], results, a.out)


if __name__ == "__main__":
    main()
