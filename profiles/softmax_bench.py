"""Sampled-softmax epoch throughput on the device (imp_softmax_update, csrc/softmax_mf.hip), beside the WARP epoch.

    python profiles/softmax_bench.py [--out DIR] [--only shape:factors,...]

Trains three epochs per configuration from BPR's initial factors (learning rate 0.02, regularization 0.01) and prints, for
the FIRST and the THIRD epoch: ms per epoch (host clock around the synchronous call), samples/s, negative logits/s (samples
x N), the correct and masked shares, and the HIP-event times of the id pre-pass (softmax_check_ids) and of the update kernel
(softmax_update).  Every epoch is timed on its own; one untimed single-sample call per configuration loads the kernel.
Configurations: the lastfm360k and ml20m synthetic shapes at factors 64 / 128 and N = 32 / 128, and per (shape, factors) the
WARP epoch (max_sampled 10) from the same initial factors, timed the same way."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = [(shape, factors) for shape in ("lastfm360k", "ml20m") for factors in (64, 128)]
NEGATIVES = (32, 128)
LR, REG, MAX_SAMPLED, EPOCHS = 0.02, 0.01, 10, 3


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


def run(configs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("softmax_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.synthetic import named

    results, data = [], {}

    def report(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    for name, factors in configs:
        if name not in data:
            m = named(name)
            userids = np.repeat(np.arange(m.shape[0], dtype=np.int32), np.diff(m.indptr))
            data[name] = (m, gpu.IntVector(userids), gpu.IntVector(m.indices), gpu.IntVector(m.indptr.astype(np.int32)))
        m, uid, iid, ptr = data[name]
        X0, Y0 = _init(m, factors)
        base = {"shape": name, "factors": factors, "nnz": int(m.nnz)}
        for N in NEGATIVES:
            X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
            gpu.softmax_epoch(uid, iid, ptr, X, Y, 0.0, 0.0, 0, N, samples=1)  # loads the kernel; a zero step
            gpu.Profiler.enable(True, only="softmax")
            for e in range(EPOCHS):
                (correct, masked), wall, (check_ms, update_ms) = _timed(
                    gpu, ("softmax_check_ids", "softmax_update"),
                    lambda: gpu.softmax_epoch(uid, iid, ptr, X, Y, LR, REG, 1000 + e, N))
                if e in (0, EPOCHS - 1):
                    report({"model": "softmax", **base, "negatives": N, "epoch": e + 1, "ms_per_epoch": round(wall * 1e3, 3),
                            "samples_per_s": round(m.nnz / wall), "negative_logits_per_s": round(m.nnz * N / wall),
                            "correct_share": round(correct / m.nnz, 4), "masked_share": round(masked / (m.nnz * N), 5),
                            "prepass_ms": round(check_ms, 4), "update_kernel_ms": round(update_ms, 3)})
            gpu.Profiler.enable(False)
        X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
        gpu.warp_epoch(uid, iid, ptr, X, Y, 0.0, 0.0, 0, MAX_SAMPLED, samples=1)
        gpu.Profiler.enable(True, only="warp")
        for e in range(EPOCHS):
            (_, trials), wall, (update_ms,) = _timed(gpu, ("warp_update",),
                                                     lambda: gpu.warp_epoch(uid, iid, ptr, X, Y, LR, REG, 1000 + e, MAX_SAMPLED))
            if e in (0, EPOCHS - 1):
                report({"model": "warp", **base, "epoch": e + 1, "ms_per_epoch": round(wall * 1e3, 3), "samples_per_s": round(m.nnz / wall),
                        "trials_per_sample": round(trials / m.nnz, 3), "update_kernel_ms": round(update_ms, 3)})
        gpu.Profiler.enable(False)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "softmax_bench"))
    ap.add_argument("--only", default=None, help="shape:factors[,shape:factors...]")
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [(s.split(":")[0], int(s.split(":")[1])) for s in a.only.split(",")]
    results = run(configs)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "softmax_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
