"""BPR epoch throughput on the device (imp_bpr_update, csrc/bpr.hip).

    python profiles/bpr_bench.py [--epochs 5] [--out DIR] [--rocprof]

Prints, per configuration, ms per epoch (host clock around the synchronous call), samples/s, the skipped fraction, the
HIP-event times of the id pre-pass (bpr_check_ids) and the update kernel (bpr_update), and the update kernel's achieved
row traffic against the model (24 C bytes per non-skipped sample: three rows read and written).  Configurations: the
lastfm360k synthetic shape at factors 64 / 100 / 128 with verification on and off, and ml20m at factors 100.
--rocprof reruns the lastfm360k factors-100 configurations in a child process under `rocprofv3 --kernel-trace --stats`
and prints the per-kernel summary (files under DIR/bpr_rocprof)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = [("lastfm360k", 64), ("lastfm360k", 100), ("lastfm360k", 128), ("ml20m", 100)]


def _init(m, factors, seed=7):
    rs = np.random.default_rng(seed)
    Y = (rs.random((m.shape[1], factors + 1), "float32") - 0.5) / factors
    X = (rs.random((m.shape[0], factors + 1), "float32") - 0.5) / factors
    X[:, factors] = 1.0
    return X, Y


def run(configs, epochs, warmup):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("bpr_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.synthetic import named

    results, data = [], {}
    for name, factors in configs:
        if name not in data:
            m = named(name)
            userids = np.repeat(np.arange(m.shape[0], dtype=np.int32), np.diff(m.indptr))
            data[name] = (m, gpu.IntVector(userids), gpu.IntVector(m.indices), gpu.IntVector(m.indptr.astype(np.int32)))
        m, uid, iid, ptr = data[name]
        X0, Y0 = _init(m, factors)
        for verify in (True, False):
            X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
            for e in range(warmup):
                gpu.bpr_epoch(uid, iid, ptr, X, Y, 0.01, 0.01, 1000 + e, verify)
            gpu.Profiler.reset()
            gpu.Profiler.enable(True, only="bpr")
            skipped_total, t0 = 0, time.perf_counter()
            for e in range(epochs):
                _, skipped = gpu.bpr_epoch(uid, iid, ptr, X, Y, 0.01, 0.01, e, verify)
                skipped_total += skipped
            wall = (time.perf_counter() - t0) / epochs
            gpu.Profiler.enable(False)
            check_ms = gpu.Profiler.get("bpr_check_ids")[0] / epochs
            update_ms = gpu.Profiler.get("bpr_update")[0] / epochs
            C = factors + 1
            done = m.nnz - skipped_total / epochs
            r = {"shape": name, "factors": factors, "verify": verify, "nnz": int(m.nnz), "ms_per_epoch": round(wall * 1e3, 3),
                 "samples_per_s": round(m.nnz / wall), "skipped_frac": round(skipped_total / epochs / m.nnz, 4),
                 "prepass_ms": round(check_ms, 4), "update_kernel_ms": round(update_ms, 3),
                 "row_bytes_model_GB": round(24 * C * done / 1e9, 3),
                 "row_GB_per_s": round(24 * C * done / (update_ms * 1e-3) / 1e9, 1) if update_ms else None,
                 "prepass_GB_per_s": round((2 * m.nnz + m.shape[0] + 1) * 4 / (check_ms * 1e-3) / 1e9, 1) if check_ms else None}
            results.append(r)
            print(json.dumps(r), flush=True)
    return results


def rocprof(out_dir, epochs):
    """The lastfm360k factors-100 configurations under rocprofv3 (a child process; its program goes after --)."""
    d = os.path.join(out_dir, "bpr_rocprof")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "bpr", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--epochs", str(epochs), "--only", "lastfm360k:100"]
    rc = subprocess.run(cmd, timeout=900).returncode
    if rc != 0:
        raise SystemExit(f"bpr_bench: rocprofv3 child exited with {rc}")
    stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    for path in stats:
        print(f"rocprofv3 --kernel-trace --stats summary ({os.path.relpath(path, out_dir)}):")
        with open(path) as f:
            for row in csv.DictReader(f):
                if "bpr" in row.get("Name", ""):
                    print(f"  {row['Name'][:60]:60s} calls {row.get('Calls')}  total {float(row.get('TotalDurationNs', 0)) / 1e6:.3f} ms"
                          f"  avg {float(row.get('AverageNs', 0)) / 1e6:.4f} ms  min {float(row.get('MinNs', 0)) / 1e6:.4f} ms"
                          f"  max {float(row.get('MaxNs', 0)) / 1e6:.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "bpr_bench"))
    ap.add_argument("--only", default=None, help="shape:factors[,shape:factors...]")
    ap.add_argument("--rocprof", action="store_true")
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [(s.split(":")[0], int(s.split(":")[1])) for s in a.only.split(",")]
    results = run(configs, a.epochs, a.warmup)
    if not a.only:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bpr_bench.json"), "w") as f:
            json.dump(results, f, indent=1)
    if a.rocprof:
        rocprof(a.out, a.epochs)


if __name__ == "__main__":
    main()
