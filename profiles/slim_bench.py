"""SLIM fit on the device (csrc/slim.hip).

    python profiles/slim_bench.py [--out DIR] [--only ml100k,mid8192,ml20m] [--reps N] [--lib PATH] [--no-cpu | --cpu-only]

For the synthetic ml100k and ml20m shapes and a middle shape of 8 192 items, with the model's defaults (l1 = 1, l2 = 10) and one
sparser setting (l1 = 10, l2 = 10), it prints one JSON line per run and writes them to DIR/slim_bench.json:
  - the HIP-event times of the Gram matrix (scope ease_gram), the coordinate descent (slim_cd) and the transpose
    (slim_transpose), best of --reps runs by the descent's time;
  - total sweeps, applied updates (imp_slim_stats), density of W;
  - the traffic estimate 4 items updates / t of the descent against 8 TB/s: every applied update reads one row of A;
  - the longest time one column held its workgroup as a share of the descent.
--lib PATH loads a build variant of the library; the one without the descending-diagonal column order is made by

    python -m implicit_amd._build --variant slim_noorder --sources slim.hip IMP_SLIM_NO_ORDER

CPU side (skipped with a note where scikit-learn is absent, or with --no-cpu): scikit-learn's ElasticNet on a seeded sample of
64 columns with 16 processes (one column each at a time), scaled to `items` columns -- an extrapolation, labelled as one."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_TBS = 8.0
SHAPES = ("ml100k", "mid8192", "ml20m")
SETTINGS = (("defaults", 1.0, 10.0), ("sparser", 10.0, 10.0))  # (label, l1, l2)
CPU_COLUMNS, CPU_PROCESSES = 64, 16


def matrix(name):
    from implicit_amd.synthetic import named, synthetic_csr

    return synthetic_csr(60_000, 8192, 4_000_000) if name == "mid8192" else named(name)


_cpu_X = None  # the CSC matrix of the CPU side, inherited by the forked workers


def cpu_column(args):
    j, l1, l2 = args
    from sklearn.linear_model import ElasticNet

    users = _cpu_X.shape[0]
    lo, hi = _cpu_X.indptr[j], _cpu_X.indptr[j + 1]
    y = np.zeros(users)
    y[_cpu_X.indices[lo:hi]] = _cpu_X.data[lo:hi]
    Z = _cpu_X.copy()
    Z.data[lo:hi] = 0.0
    model = ElasticNet(alpha=(l1 + l2) / users, l1_ratio=l1 / (l1 + l2), positive=True, fit_intercept=False, tol=1e-4, max_iter=100)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit(Z, y)
    return int(np.count_nonzero(model.coef_))


def cpu_extrapolation(X, l1, l2):
    """Runs before the device is opened: the workers are forked."""
    global _cpu_X
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return {"cpu_note": "scikit-learn is not installed: no CPU figure"}
    import multiprocessing

    _cpu_X = X.tocsc().astype(np.float64)
    cols = np.random.default_rng(64).choice(X.shape[1], size=min(CPU_COLUMNS, X.shape[1]), replace=False)
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(CPU_PROCESSES) as pool:
        pool.map(cpu_column, [(int(j), l1, l2) for j in cols], chunksize=1)
    wall = time.perf_counter() - t0  # the copy of the design per column included: what a per-item loop over scikit-learn pays
    _cpu_X = None
    return {"cpu_sklearn_sample_columns": len(cols), "cpu_processes": CPU_PROCESSES, "cpu_sample_wall_s": round(wall, 3),
            "cpu_extrapolated_fit_s": round(wall * X.shape[1] / len(cols), 1),
            "cpu_note": "extrapolated from the sample to all columns, not measured"}


def one_fit(gpu, iu, ui, l1, l2):
    gpu.Profiler.reset()
    gpu.Profiler.enable(True)
    A = gpu.ease_gram(iu, ui, l2)
    W, sweeps = gpu.slim_solve(A, l1)
    gpu.Profiler.enable(False)
    ms = {s: gpu.Profiler.get(s)[0] for s in ("ease_gram", "slim_diag", "slim_cd", "slim_transpose")}
    updates, longest = gpu.slim_stats()
    return W, sweeps, ms, updates, longest


def run(names, reps, cpu):
    cpu_side = {name: cpu_extrapolation(matrix(name), SETTINGS[0][1], SETTINGS[0][2]) for name in names} if cpu else {}
    if cpu == "only":
        for name in names:
            print(json.dumps({"shape": name, "setting": SETTINGS[0][0], **cpu_side[name]}), flush=True)
        return [{"shape": name, **cpu_side[name]} for name in names]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("slim_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.slim import SLIM
    from implicit_amd.synthetic import synthetic_csr
    from implicit_amd.utils import transpose_csr

    SLIM().fit(synthetic_csr(300, 64, 3000, seed=1), show_progress=False)  # loads the kernels
    results = []
    for name in names:
        X = matrix(name)
        items = X.shape[1]
        iu, ui = gpu.CSRMatrix(transpose_csr(X)), gpu.CSRMatrix(X)
        for label, l1, l2 in SETTINGS:
            best = None
            for _ in range(reps):
                W, sweeps, ms, updates, longest = one_fit(gpu, iu, ui, l1, l2)
                if best is None or ms["slim_cd"] < best[0]["slim_cd"]:
                    best = (ms, longest)
                nonzero = int(np.count_nonzero(W.to_numpy())) if best[0] is ms else nonzero
                del W
            ms, longest = best
            cd_s = ms["slim_cd"] * 1e-3
            r = {"shape": name, "setting": label, "l1": l1, "l2": l2, "users": int(X.shape[0]), "items": int(items), "nnz": int(X.nnz),
                 "gram_ms": round(ms["ease_gram"], 3), "diag_ms": round(ms["slim_diag"], 3), "solve_ms": round(ms["slim_cd"], 3),
                 "transpose_ms": round(ms["slim_transpose"], 3), "total_sweeps": int(sweeps.sum()), "max_sweeps_of_a_column": int(sweeps.max()),
                 "applied_updates": int(updates), "density": nonzero / max(1, items * (items - 1)),
                 "row_traffic_tb_per_s": round(4.0 * items * updates / cd_s / 1e12, 3),
                 "row_traffic_frac_of_8tbs": round(4.0 * items * updates / cd_s / 1e12 / PEAK_TBS, 4),
                 "longest_column_ms": round(longest * 1e3, 3), "longest_column_share_of_solve": round(longest / cd_s, 4)}
            if cpu and label == SETTINGS[0][0]:
                r.update(cpu_side[name])
            results.append(r)
            print(json.dumps(r), flush=True)
        del iu, ui
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "slim_bench"))
    ap.add_argument("--only", default=None, help="comma-separated subset of " + ",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--lib", default=None, help="a build variant of libimplicit_hip.so to load instead of the in-tree one")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="the scikit-learn side alone: needs no device")
    a = ap.parse_args()
    if a.lib:
        from implicit_amd import _libpath

        _libpath.OVERRIDE = os.path.abspath(a.lib)
    names = a.only.split(",") if a.only else list(SHAPES)
    results = run(names, a.reps, "only" if a.cpu_only else not a.no_cpu)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "slim_bench_cpu.json" if a.cpu_only else "slim_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
