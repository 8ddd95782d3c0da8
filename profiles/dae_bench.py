"""Mult-DAE training step on the device (imp_dae_step, csrc/mult_dae.hip).

    python profiles/dae_bench.py [--out DIR] [--only shape:hidden,...] [--steps N]

Per configuration (the lastfm360k and ml20m synthetic shapes, hidden 128 / 512, batch_size 512, dropout 0.5): two untimed
steps load the kernels and size the workspace, then N steps over consecutive batches of a seeded permutation are timed one
by one with the host clock around the synchronous call (median and range printed; ms per epoch is the median times the
steps of an epoch -- extrapolated, not run).  A SEPARATE pass of N steps with the library's HIP-event profiler gives the time
of the encoder, of pass 1 (with the merge of the row statistics), of pass 2, of the rest of the gradients (fold, bias, loss,
scatter) and of Adam.  The dense passes' share of the 157.3 TFLOP/s fp32 matrix peak counts 2 B H items flop for pass 1 and
three times that for pass 2 (tiles padded to 64 items are not counted)."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = [(shape, hidden) for shape in ("lastfm360k", "ml20m") for hidden in (128, 512)]
BATCH, DROPOUT, LR, PEAK_TF = 512, 0.5, 1e-3, 157.3
SCOPES = ("dae_encode", "dae_pass1", "dae_pass2", "dae_rest", "dae_adam")


def run(configs, steps):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("dae_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.synthetic import named

    results, data = [], {}
    for name, H in configs:
        if name not in data:
            m = named(name)
            data = {name: (m, gpu.CSRMatrix(m))}  # one matrix resident at a time
        m, csr = data[name]
        users, items = m.shape
        rs = np.random.default_rng(7)
        std = np.sqrt(2.0 / (items + H))
        params = [gpu.Matrix((rs.standard_normal((items, H)) * std).astype(np.float32)), gpu.Matrix(np.zeros((1, H), np.float32)),
                  gpu.Matrix((rs.standard_normal((items, H + 1)) * std).astype(np.float32))]
        moments = [gpu.Matrix.zeros(*p.shape) for p in params for _ in range(2)]
        order = rs.permutation(users).astype(np.int32)
        batches = [order[b:b + BATCH] for b in range(0, users - BATCH + 1, BATCH)]
        step = 0

        def one():
            nonlocal step
            step += 1
            t0 = time.perf_counter()
            loss = gpu.dae_step(csr, batches[step % len(batches)], params, moments, DROPOUT, step, LR, step)
            return (time.perf_counter() - t0) * 1e3, loss

        for _ in range(2):
            one()
        wall = sorted(one()[0] for _ in range(steps))
        gpu.Profiler.enable(True, only="dae_")
        gpu.Profiler.reset()
        loss = [one()[1] for _ in range(steps)][-1]
        ms = {s: gpu.Profiler.get(s)[0] / steps for s in SCOPES}
        gpu.Profiler.enable(False)
        flop1 = 2.0 * BATCH * H * items
        per_epoch = -(-users // BATCH)
        r = {"shape": name, "users": users, "items": items, "nnz": int(m.nnz), "hidden": H, "batch_size": BATCH, "steps_timed": steps,
             "ms_per_step_median": round(wall[len(wall) // 2], 3), "ms_per_step_min": round(wall[0], 3),
             "ms_per_step_max": round(wall[-1], 3), "steps_per_epoch": per_epoch,
             "ms_per_epoch_extrapolated": round(wall[len(wall) // 2] * per_epoch, 1),
             **{f"{s}_ms": round(v, 3) for s, v in ms.items()},
             "pass1_share_of_peak": round(flop1 / (ms["dae_pass1"] * 1e-3) / (PEAK_TF * 1e12), 4),
             "pass2_share_of_peak": round(3 * flop1 / (ms["dae_pass2"] * 1e-3) / (PEAK_TF * 1e12), 4), "last_loss": round(loss, 4)}
        results.append(r)
        print(json.dumps(r), flush=True)
        del params, moments
        gpu.release_workspaces()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "dae_bench"))
    ap.add_argument("--only", default=None, help="shape:hidden[,shape:hidden...]")
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [(s.split(":")[0], int(s.split(":")[1])) for s in a.only.split(",")]
    results = run(configs, a.steps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "dae_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
