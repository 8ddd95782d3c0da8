"""EASE fit and recommend on the device (csrc/ease.hip, csrc/spd_inverse.hip).

    python profiles/ease_bench.py [--out DIR] [--only ml100k,mid8192,ml20m] [--reps N]

For the synthetic ml100k and ml20m shapes and a middle shape of 8 192 items it prints one JSON line per shape and writes them
to DIR/ease_bench.json:
  - the HIP-event times of the three fit stages (scopes ease_gram, spd_inverse, ease_weights), best of --reps runs, and the
    split of the inverse into its phases (the nested scopes spd_inverse_factor, spd_inverse_tri, spd_inverse_wtw);
  - the inverse's rate n^3 / t against the 157.3 TF fp32 matrix peak;
  - recommend at batch 1000, N = 10: users/s on the host clock around the call, and the gather rate 4 items nnz(batch) / t of
    the scoring kernel (scope ease_score) against 8 TB/s.
At the 8 192-item shape only it also times LAPACK's spotrf + spotri (scipy) on the same Gram matrix on 16 CPU threads: the fit
is not done unless the device inverse is the faster one.  One untimed fit of a 64-item matrix loads the kernels first."""
import argparse
import json
import os
import sys
import time
import warnings

os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")  # the CPU comparison runs on the 16 CPUs a command may use

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_TF, PEAK_TBS = 157.3, 8.0
SHAPES = ("ml100k", "mid8192", "ml20m")
BATCH, TOPN, REG = 1000, 10, 500.0


def matrix(name):
    from implicit_amd.synthetic import named, synthetic_csr

    return synthetic_csr(60_000, 8192, 4_000_000) if name == "mid8192" else named(name)


PHASES = ("spd_inverse_factor", "spd_inverse_tri", "spd_inverse_wtw")


def stages(gpu, iu, ui):
    """One fit, stage by stage; returns the weights and the milliseconds of every scope (nested scopes need a name filter)."""
    gpu.Profiler.reset()
    gpu.Profiler.enable(True, only="ease_")
    G = gpu.ease_gram(iu, ui, REG)
    gpu.Profiler.enable(True, only="spd_inverse")
    gpu.spd_inverse(G)
    gpu.Profiler.enable(True, only="ease_")
    gpu.ease_weights(G)
    gpu.Profiler.enable(False)
    return G, {s: gpu.Profiler.get(s)[0] for s in ("ease_gram", "spd_inverse", "ease_weights") + PHASES}


def run(names, reps):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("ease_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.ease import EASE
    from implicit_amd.synthetic import synthetic_csr
    from implicit_amd.utils import transpose_csr

    EASE(regularization=10.0).fit(synthetic_csr(300, 64, 3000, seed=1), show_progress=False)  # loads the kernels
    results = []
    for name in names:
        X = matrix(name)
        items = X.shape[1]
        iu, ui = gpu.CSRMatrix(transpose_csr(X)), gpu.CSRMatrix(X)
        best = None
        for _ in range(reps):
            B, ms = stages(gpu, iu, ui)
            if best is None or ms["spd_inverse"] < best["spd_inverse"]:
                best = ms
        model = EASE(regularization=REG)
        model.item_weights = B
        batch = X[:BATCH]
        users = np.arange(batch.shape[0])
        model.recommend(users, batch, N=TOPN)  # untimed: allocations, kernel load
        gpu.Profiler.enable(True, only="ease_")
        walls, score_ms = [], []
        for _ in range(max(reps, 3)):
            gpu.Profiler.reset()
            t0 = time.perf_counter()
            model.recommend(users, batch, N=TOPN)
            walls.append(time.perf_counter() - t0)
            score_ms.append(gpu.Profiler.get("ease_score")[0])
        gpu.Profiler.enable(False)
        inv_s = best["spd_inverse"] * 1e-3
        gather_bytes = 4.0 * items * batch.nnz
        r = {"shape": name, "users": int(X.shape[0]), "items": int(items), "nnz": int(X.nnz),
             "gram_ms": round(best["ease_gram"], 3), "inverse_ms": round(best["spd_inverse"], 3),
             "weights_ms": round(best["ease_weights"], 3),
             "inverse_phases_ms": {k: round(best[k], 3) for k in PHASES},
             "inverse_tflops": round(items**3 / inv_s / 1e12, 2), "inverse_frac_of_peak": round(items**3 / inv_s / 1e12 / PEAK_TF, 4),
             "recommend_users_per_s": round(len(users) / min(walls)), "recommend_batch_nnz": int(batch.nnz),
             "score_kernel_ms": round(min(score_ms), 3),
             "gather_tb_per_s": round(gather_bytes / (min(score_ms) * 1e-3) / 1e12, 3),
             "gather_frac_of_8tbs": round(gather_bytes / (min(score_ms) * 1e-3) / 1e12 / PEAK_TBS, 4)}
        if name == "mid8192":
            from scipy.linalg import lapack

            G = gpu.ease_gram(iu, ui, REG).to_numpy()
            t0 = time.perf_counter()
            c, info = lapack.spotrf(G, lower=1)
            p, info2 = lapack.spotri(c, lower=1)
            r["cpu_lapack_spotrf_spotri_s"] = round(time.perf_counter() - t0, 3)
            r["cpu_threads"] = int(os.environ["OPENBLAS_NUM_THREADS"])
            assert info == 0 and info2 == 0
            r["gpu_faster_than_cpu_lapack"] = bool(inv_s < r["cpu_lapack_spotrf_spotri_s"])
            # agreement of the two inverses (lower triangles), as a sanity check of what was timed
            Pg = gpu.spd_inverse(gpu.Matrix(G)).to_numpy()
            r["gpu_vs_lapack_rel_diff"] = float(np.linalg.norm(np.tril(Pg) - np.tril(p)) / np.linalg.norm(np.tril(p)))
        results.append(r)
        print(json.dumps(r), flush=True)
        del B, model, iu, ui
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "ease_bench"))
    ap.add_argument("--only", default=None, help="comma-separated subset of " + ",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    names = a.only.split(",") if a.only else list(SHAPES)
    results = run(names, a.reps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ease_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
