"""The block-subspace solver (block_size=, csrc/als_subspace.hip) against the CG-3 half sweep, same process, same device.

    python profiles/subspace_bench.py [--factors 128,256,512,1024] [--blocks 8,16,32] [--iterations 10] [--reps 3] [--out DIR]

Matrix: the BASELINE configs[2]-shaped synthetic matrix (358 868 users x 292 385 items, 17.5 M nonzeros).  For every factor count
both solvers start from the same initial factors (rng.random * 0.01, as fit() draws them) and run through the model's own
_half_sweep, queued in deferred mode and waited for once per iteration as fit() does:

  * `--iterations` iterations, each under a host clock (profiler off), calculate_loss after each one (not timed): the loss
    curve of each solver, so that time-to-loss can be read off;
  * `--reps` more iterations with the library's HIP-event scopes on (imp_prof: an event pair around every kernel scope on the
    library stream): the sum of all scopes of an iteration is the device time of that iteration without the gaps between
    launches; the best of the reps is reported beside the best host-clock iteration.

One process on the device; the core clock behind a step (imp_debug_core_clock) is noted per configuration.  One JSON line per
configuration, a table at the end."""
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
REG = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", default="128,256,512,1024")
    ap.add_argument("--blocks", default="8,16,32")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the matrix (debug only; flagged in the output)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
        from implicit_amd.gpu.als import AlternatingLeastSquares
        from implicit_amd.synthetic import synthetic_csr
        from implicit_amd.utils import random_factors, transpose_csr
    if not gpu.HAS_CUDA:
        raise SystemExit("subspace_bench: no usable device (there is nothing to measure without one)")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    users, items, nnz, gamma = SHAPE
    if a.scale != 1.0:
        users, items, nnz = int(users * a.scale), int(items * a.scale), int(nnz * a.scale)
    t0 = time.perf_counter()
    C = synthetic_csr(users, items, nnz, gamma=gamma, seed=42)
    Cui, Ciu = gpu.CSRMatrix(C), gpu.CSRMatrix(transpose_csr(C))
    print(f"# matrix {C.shape}, nnz {C.nnz}, scale {a.scale}, set up in {time.perf_counter() - t0:.1f} s", flush=True)
    results, lines = [], []
    lines.append(f"{'f':>5} {'solver':>8} {'ms/iter (HIP events)':>21} {'ms/iter (host clock)':>21} {'clock MHz':>10}  loss after iterations 1 .. {a.iterations}")
    for f in (int(x) for x in a.factors.split(",")):
        rng = np.random.default_rng(1)
        X0, Y0 = random_factors(rng, users, f), random_factors(rng, items, f)
        for block in [None] + [int(b) for b in a.blocks.split(",")]:
            model = AlternatingLeastSquares(factors=f, regularization=REG, block_size=block)
            X, Y, gram = gpu.Matrix(X0), gpu.Matrix(Y0), gpu.Matrix.zeros(f, f)

            def iteration():
                t = time.perf_counter()
                gpu.set_deferred_sync(True)
                try:
                    model._half_sweep(Cui, X, Y, gram)
                    model._half_sweep(Ciu, Y, X, gram)
                    gpu.synchronize()
                finally:
                    gpu.set_deferred_sync(False)
                return (time.perf_counter() - t) * 1e3

            host_ms, losses = [], []
            for _ in range(a.iterations):
                host_ms.append(iteration())
                losses.append(float(model.solver.calculate_loss(Cui, X, Y, REG)))
            clock = round(gpu.core_clock_mhz(50), 1)
            event_ms = []
            for _ in range(a.reps):
                gpu.Profiler.reset()
                gpu.Profiler.enable(True)
                iteration()
                gpu.Profiler.enable(False)
                scopes = {name: round(gpu.Profiler.get(name)[0], 3) for name in gpu.Profiler.names()}
                event_ms.append(sum(scopes.values()))
            name = "cg3" if block is None else f"k={block}"
            r = {"factors": f, "solver": name, "scale": a.scale, "ms_per_iteration_hip_events_best": min(event_ms),
                 "ms_per_iteration_hip_events": event_ms, "ms_per_iteration_host_clock_best": min(host_ms[1:] or host_ms),
                 "ms_per_iteration_host_clock": host_ms, "loss": losses, "core_clock_mhz_behind_a_step": clock,
                 "scopes_ms_last_rep": scopes}
            print(json.dumps(r), flush=True)
            results.append(r)
            lines.append(f"{f:>5} {name:>8} {min(event_ms):>21.2f} {min(host_ms[1:] or host_ms):>21.2f} {clock:>10}  "
                         + " ".join(f"{v:.5f}" for v in losses))
            if a.out:  # kept after every configuration: a later one may be cut short
                with open(os.path.join(a.out, "subspace_bench.json"), "w") as fh:
                    json.dump(results, fh, indent=1)
                with open(os.path.join(a.out, "subspace_bench_table.txt"), "w") as fh:
                    fh.write("\n".join(lines) + "\n")
            del model, X, Y, gram
            gpu.release_workspaces()
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
