"""Mult-VAE training step on the device (imp_vae_step, csrc/mult_vae.hip), in the manner of dae_bench.py.

    python profiles/vae_bench.py [--out DIR] [--only shape:hidden:latent,...] [--steps N]

Per configuration (the lastfm360k and ml20m synthetic shapes, hidden / latent 128 / 64 and 512 / 256, batch_size 512, dropout
0.5, beta 0.2): two untimed steps load the kernels and size the workspace, then N steps over consecutive batches of a seeded
permutation are timed one by one with the host clock around the synchronous call (median and range printed).  A SEPARATE pass
of N steps with the library's HIP-event profiler gives the time of: zeroing dW_in and the encoder; the two bottleneck forward
kernels; pass 1 with the merge; pass 2 with the fold; the two bottleneck backward kernels; bias / loss and the scatter; Adam.
The cost of the bottleneck is this step against dae_bench.py's at the same shape and hidden width, run in the same session."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = [(shape, hidden, latent) for shape in ("lastfm360k", "ml20m") for hidden, latent in ((128, 64), (512, 256))]
BATCH, DROPOUT, BETA, LR = 512, 0.5, 0.2, 1e-3
SCOPES = ("vae_encode", "vae_forward", "vae_pass1", "vae_pass2", "vae_backward", "vae_rest", "vae_adam")


def run(configs, steps):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("vae_bench: no HIP device (there is no CPU path to measure)")
    from implicit_amd.synthetic import named

    results, data = [], {}
    for name, H, L in configs:
        if name not in data:
            m = named(name)
            data = {name: (m, gpu.CSRMatrix(m))}  # one matrix resident at a time
        m, csr = data[name]
        users, items = m.shape
        rs = np.random.default_rng(7)
        shapes = [(items, H), (1, H), (H, 2 * L), (1, 2 * L), (L, H), (1, H), (items, H + 1)]
        params = [gpu.Matrix(np.zeros(s, np.float32) if s[0] == 1 else (rs.standard_normal(s) * np.sqrt(2.0 / sum(s))).astype(np.float32))
                  for s in shapes]
        moments = [gpu.Matrix.zeros(*p.shape) for p in params for _ in range(2)]
        order = rs.permutation(users).astype(np.int32)
        batches = [order[b:b + BATCH] for b in range(0, users - BATCH + 1, BATCH)]
        step = 0

        def one():
            nonlocal step
            step += 1
            t0 = time.perf_counter()
            nll, kl = gpu.vae_step(csr, batches[step % len(batches)], params, moments, DROPOUT, step, BETA, LR, step)
            return (time.perf_counter() - t0) * 1e3, nll + BETA * kl

        for _ in range(2):
            one()
        wall = sorted(one()[0] for _ in range(steps))
        gpu.Profiler.enable(True, only="vae_")
        gpu.Profiler.reset()
        loss = [one()[1] for _ in range(steps)][-1]
        ms = {s: gpu.Profiler.get(s)[0] / steps for s in SCOPES}
        gpu.Profiler.enable(False)
        r = {"shape": name, "users": users, "items": items, "nnz": int(m.nnz), "hidden": H, "latent": L, "batch_size": BATCH,
             "steps_timed": steps, "ms_per_step_median": round(wall[len(wall) // 2], 3), "ms_per_step_min": round(wall[0], 3),
             "ms_per_step_max": round(wall[-1], 3), **{f"{s}_ms": round(v, 3) for s, v in ms.items()}, "last_loss": round(loss, 4)}
        results.append(r)
        print(json.dumps(r), flush=True)
        del params, moments
        gpu.release_workspaces()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "vae_bench"))
    ap.add_argument("--only", default=None, help="shape:hidden:latent[,shape:hidden:latent...]")
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [(s.split(":")[0], int(s.split(":")[1]), int(s.split(":")[2])) for s in a.only.split(",")]
    results = run(configs, a.steps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "vae_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
