"""LMF epoch throughput on the device (imp_lmf_update, csrc/lmf.hip).

    python profiles/lmf_bench.py [--epochs 5] [--out DIR] [--rocprof] [--no-cpu]

Prints, per configuration, ms per epoch (host clock around the two synchronous half-sweeps), the HIP-event time of each
half-sweep's kernels (lmf_rows: rows of <= 512 nonzeros; lmf_segments: the long rows' segment partials; lmf_finish: the
long rows' negatives, partial sums and Adagrad), and the achieved gathered-row bandwidth against the traffic model: a
half-sweep gathers one Y row per nonzero and one per negative, sum_r min(C, n_r neg_prop), each C x 4 bytes (the positive
rows of a long row are gathered once, by its segments).  Configurations: the lastfm360k synthetic shape at factors 30 / 64
/ 126 and ml20m at factors 30, all at neg_prop 30.  Where build/refsuite exists, the reference CPU LMF epoch at 16
threads is timed as the baseline (--no-cpu skips it).  --rocprof reruns lastfm360k / 30 in a child process under
`rocprofv3 --kernel-trace --stats` and prints the per-kernel summary (files under DIR/lmf_rocprof)."""
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
SUITE = os.path.join(ROOT, "build", "refsuite")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = [("lastfm360k", 30), ("lastfm360k", 64), ("lastfm360k", 126), ("ml20m", 30)]
NEG_PROP = 30
KERNELS = ("lmf_rows", "lmf_segments", "lmf_finish")


def gathered_rows(m, C, neg_prop=NEG_PROP):
    n = np.diff(m.indptr).astype(np.int64)
    return int(m.nnz + np.minimum(C, n * neg_prop).sum())


def _init(m, factors, seed=7):
    rs = np.random.default_rng(seed)
    Y = rs.standard_normal((m.shape[1], factors + 2), dtype=np.float32)
    Y[:, -1] = 1.0
    X = rs.standard_normal((m.shape[0], factors + 2), dtype=np.float32)
    X[:, -2] = 1.0
    return X, Y


_CPU_SCRIPT = r"""
import sys, time, warnings
import numpy as np
from scipy.sparse import load_npz
warnings.simplefilter("ignore")
from implicit.cpu.lmf import LogisticMatrixFactorization
m = load_npz(sys.argv[1])
model = LogisticMatrixFactorization(factors=int(sys.argv[2]), iterations=1, neg_prop=30, num_threads=16, random_state=1)
times = []
model.fit(m, show_progress=False, callback=lambda e, t: times.append(t))
print(times[0] * 1e3)
"""


def cpu_epoch_ms(m, factors, out_dir):
    """The reference's CPU LMF (build/refsuite), 16 threads: one epoch (the callback's elapsed)."""
    from scipy.sparse import save_npz

    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "lmf_bench_matrix.npz")
    save_npz(path, m)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([SUITE, ROOT]), OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="16")
    out = subprocess.run([sys.executable, "-c", _CPU_SCRIPT, path, str(factors)], env=env, capture_output=True, text=True,
                         timeout=1800)
    os.remove(path)
    if out.returncode != 0:
        print(out.stderr[-2000:], file=sys.stderr)
        return None
    return float(out.stdout.strip().splitlines()[-1])


def run(configs, epochs, warmup, cpu, out_dir):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("lmf_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.synthetic import named

    results, data = [], {}
    for name, factors in configs:
        if name not in data:
            m = named(name)
            mt = m.T.tocsr()
            mt.sort_indices()
            data[name] = (m, mt, gpu.CSRMatrix(m), gpu.CSRMatrix(mt))
        m, mt, cui, ciu = data[name]
        C = factors + 2
        X0, Y0 = _init(m, factors)
        X, Y = gpu.Matrix(X0), gpu.Matrix(Y0)
        GX, GY = gpu.Matrix.zeros(*X0.shape), gpu.Matrix.zeros(*Y0.shape)

        def half(csr, A, B, GA, one_col, seed, timed):
            if timed:
                gpu.Profiler.reset()
                gpu.Profiler.enable(True, only="lmf")
            gpu.lmf_update(csr, A, B, GA, 1.0, 0.6, NEG_PROP, seed, one_col)
            if timed:
                gpu.Profiler.enable(False)
                return {k: gpu.Profiler.get(k)[0] for k in KERNELS}
            return None

        for e in range(warmup):
            half(cui, X, Y, GX, C - 2, 2 * e, False)
            half(ciu, Y, X, GY, C - 1, 2 * e + 1, False)
        wall = 0.0
        kt = {s: dict.fromkeys(KERNELS, 0.0) for s in ("user", "item")}
        for e in range(epochs):
            t0 = time.perf_counter()
            gpu.lmf_update(cui, X, Y, GX, 1.0, 0.6, NEG_PROP, 100 + 2 * e, C - 2)
            gpu.lmf_update(ciu, Y, X, GY, 1.0, 0.6, NEG_PROP, 101 + 2 * e, C - 1)
            wall += time.perf_counter() - t0
        for e in range(epochs):  # kernel times in a separate pass: the event pairs cost stream time
            for side, (csr, A, B, GA, oc) in (("user", (cui, X, Y, GX, C - 2)), ("item", (ciu, Y, X, GY, C - 1))):
                for k, v in half(csr, A, B, GA, oc, 1000 + e, True).items():
                    kt[side][k] += v / epochs
        rows_u, rows_i = gathered_rows(m, C), gathered_rows(mt, C)
        ms_u, ms_i = sum(kt["user"].values()), sum(kt["item"].values())
        gb = (rows_u + rows_i) * C * 4 / 1e9
        r = {"shape": name, "factors": factors, "C": C, "neg_prop": NEG_PROP, "nnz": int(m.nnz),
             "ms_per_epoch": round(wall / epochs * 1e3, 3),
             "user_half_ms": {k: round(v, 4) for k, v in kt["user"].items()},
             "item_half_ms": {k: round(v, 4) for k, v in kt["item"].items()},
             "gathered_rows_M": round((rows_u + rows_i) / 1e6, 2), "traffic_model_GB": round(gb, 3),
             "kernel_ms": round(ms_u + ms_i, 3),
             "gathered_TB_per_s": round(gb / ((ms_u + ms_i) * 1e-3) / 1e3, 2) if ms_u + ms_i else None,
             "user_half_TB_per_s": round(rows_u * C * 4 / (ms_u * 1e-3) / 1e12, 2) if ms_u else None,
             "item_half_TB_per_s": round(rows_i * C * 4 / (ms_i * 1e-3) / 1e12, 2) if ms_i else None}
        if cpu and os.path.isdir(SUITE):
            cms = cpu_epoch_ms(m, factors, out_dir)
            r["reference_cpu16_ms_per_epoch"] = None if cms is None else round(cms, 1)
        results.append(r)
        print(json.dumps(r), flush=True)
    return results


def rocprof(out_dir, epochs):
    """lastfm360k / 30 under rocprofv3 (a child process; its program goes after --)."""
    d = os.path.join(out_dir, "lmf_rocprof")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "lmf", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--epochs", str(epochs), "--only", "lastfm360k:30", "--no-cpu"]
    rc = subprocess.run(cmd, timeout=900).returncode
    if rc != 0:
        raise SystemExit(f"lmf_bench: rocprofv3 child exited with {rc}")
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        print(f"rocprofv3 --kernel-trace --stats summary ({os.path.relpath(path, out_dir)}):")
        with open(path) as f:
            for row in csv.DictReader(f):
                if "lmf" in row.get("Name", ""):
                    print(f"  {row['Name'][:60]:60s} calls {row.get('Calls')}  total {float(row.get('TotalDurationNs', 0)) / 1e6:.3f} ms"
                          f"  avg {float(row.get('AverageNs', 0)) / 1e6:.4f} ms  min {float(row.get('MinNs', 0)) / 1e6:.4f} ms"
                          f"  max {float(row.get('MaxNs', 0)) / 1e6:.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "lmf_bench"))
    ap.add_argument("--only", default=None, help="shape:factors[,shape:factors...]")
    ap.add_argument("--no-cpu", action="store_true", help="skip the reference CPU baseline")
    ap.add_argument("--rocprof", action="store_true")
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [(s.split(":")[0], int(s.split(":")[1])) for s in a.only.split(",")]
    results = run(configs, a.epochs, a.warmup, not a.no_cpu, a.out)
    if not a.only:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "lmf_bench.json"), "w") as f:
            json.dump(results, f, indent=1)
    if a.rocprof:
        rocprof(a.out, a.epochs)


if __name__ == "__main__":
    main()
