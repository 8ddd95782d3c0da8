"""WARP epoch throughput on the device (imp_warp_update, csrc/warp.hip).

    python profiles/warp_bench.py [--out DIR] [--only shape:factors,...] [--bpr]

Trains six epochs per configuration from BPR's initial factors (learning rate 0.02, regularization 0.01, max_sampled 10)
and prints, for the FIRST epoch (small factors, short trial chains) and for the SIXTH (long chains): ms per epoch (host
clock around the synchronous call), samples/s, trials/s, mean trials per sample, and the HIP-event times of the id
pre-pass (warp_check_ids) and of the update kernel (warp_update).  Every epoch is timed on its own: the state of the
factors is what decides an epoch's cost, so no epoch is a warm-up of another; one untimed single-sample call per
configuration loads the kernel.  Configurations: the lastfm360k and ml20m synthetic shapes at factors 64 / 100 / 128.
--bpr adds BPR's verified epoch from the same initial factors (the first epoch's natural comparison: the same three rows
written, one row dot fewer)."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = [(shape, factors) for shape in ("lastfm360k", "ml20m") for factors in (64, 100, 128)]
LR, REG, MAX_SAMPLED, EPOCHS = 0.02, 0.01, 10, 6


def _init(m, factors, seed=7):
    rs = np.random.default_rng(seed)
    Y = (rs.random((m.shape[1], factors + 1), "float32") - 0.5) / factors
    X = (rs.random((m.shape[0], factors + 1), "float32") - 0.5) / factors
    X[:, factors] = 1.0
    return X, Y


def _timed(gpu, scopes, call):
    gpu.Profiler.reset()
    t0 = time.perf_counter()
    out = call()
    wall = time.perf_counter() - t0
    return out, wall, [gpu.Profiler.get(s)[0] for s in scopes]


def run(configs, bpr):
    if os.environ.get("IMP_LIB_PATH"):  # A/B of a compile-time variant (python -m implicit_amd._build --variant ...), as bench.py
        import implicit_amd._libpath as _libpath

        _libpath.OVERRIDE = os.environ["IMP_LIB_PATH"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("warp_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.synthetic import named

    results, data = [], {}
    for name, factors in configs:
        if name not in data:
            m = named(name)
            userids = np.repeat(np.arange(m.shape[0], dtype=np.int32), np.diff(m.indptr))
            data[name] = (m, gpu.IntVector(userids), gpu.IntVector(m.indices), gpu.IntVector(m.indptr.astype(np.int32)))
        m, uid, iid, ptr = data[name]
        X0, Y0 = _init(m, factors)
        X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
        gpu.warp_epoch(uid, iid, ptr, X, Y, 0.0, 0.0, 0, MAX_SAMPLED, samples=1)  # loads the kernel; a zero step
        gpu.Profiler.enable(True, only="warp")
        for e in range(EPOCHS):
            (_, trials), wall, (check_ms, update_ms) = _timed(
                gpu, ("warp_check_ids", "warp_update"),
                lambda: gpu.warp_epoch(uid, iid, ptr, X, Y, LR, REG, 1000 + e, MAX_SAMPLED))
            if e in (0, EPOCHS - 1):
                r = {"model": "warp", "shape": name, "factors": factors, "epoch": e + 1, "nnz": int(m.nnz),
                     "ms_per_epoch": round(wall * 1e3, 3), "samples_per_s": round(m.nnz / wall), "trials_per_s": round(trials / wall),
                     "trials_per_sample": round(trials / m.nnz, 3), "prepass_ms": round(check_ms, 4),
                     "update_kernel_ms": round(update_ms, 3)}
                results.append(r)
                print(json.dumps(r), flush=True)
        gpu.Profiler.enable(False)
        if bpr:
            X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
            gpu.bpr_epoch(uid, iid, ptr, X, Y, 0.0, 0.0, 0, True, samples=1)
            gpu.Profiler.enable(True, only="bpr")
            (_, skipped), wall, (update_ms,) = _timed(gpu, ("bpr_update",),
                                                      lambda: gpu.bpr_epoch(uid, iid, ptr, X, Y, LR, REG, 1000, True))
            gpu.Profiler.enable(False)
            r = {"model": "bpr", "shape": name, "factors": factors, "epoch": 1, "nnz": int(m.nnz), "ms_per_epoch": round(wall * 1e3, 3),
                 "samples_per_s": round(m.nnz / wall), "skipped_frac": round(skipped / m.nnz, 4), "update_kernel_ms": round(update_ms, 3)}
            results.append(r)
            print(json.dumps(r), flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "warp_bench"))
    ap.add_argument("--only", default=None, help="shape:factors[,shape:factors...]")
    ap.add_argument("--bpr", action="store_true", help="also time BPR's verified first epoch from the same factors")
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [(s.split(":")[0], int(s.split(":")[1])) for s in a.only.split(",")]
    results = run(configs, a.bpr)
    if not a.only:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "warp_bench.json"), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
