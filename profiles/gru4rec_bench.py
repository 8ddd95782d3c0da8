"""GRU4Rec training step on the device (imp_gru_steps, csrc/gru4rec.hip).

    python profiles/gru4rec_bench.py [--out DIR] [--only shape:hidden:loss,...] [--steps N]

Per configuration (the item counts of the lastfm360k and ml20m synthetic shapes, hidden 128 / 512, both losses, 512 slots, 2048
extra negatives; inputs, targets and negatives uniform over the items, a tenth of the slots reset each step): one untimed call
of N steps loads the kernels and sizes the workspace, then calls of ONE step each are timed with the host clock around the
synchronous call (median and range printed) and one call of N steps gives the time per step when the steps are queued without
a host wait.  A SEPARATE pass of N one-step calls with the library's HIP-event profiler gives the time of the gates, of the
three score launches, of the three backward launches and of the update; what the queued step takes beyond their sum is the
gaps between its 9 launches.  No speed-up is claimed: there is no earlier path."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ITEMS = {"lastfm360k": 292_385, "ml20m": 26_744}
CONFIGS = [(shape, hidden, loss) for shape in ITEMS for hidden in (128, 512) for loss in ("cross-entropy", "bpr-max")]
BATCH, NEGATIVES, LAUNCHES = 512, 2048, 9
SCOPES = ("gru_gates", "gru_scores", "gru_backward", "gru_update")


def run(configs, steps):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
    if not gpu.HAS_CUDA:
        raise SystemExit("gru4rec_bench: no HIP device (there is no CPU path to measure)")
    results = []
    for name, H, loss in configs:
        items, rs = ITEMS[name], np.random.default_rng(7)

        def uniform(rows, cols):
            bound = np.sqrt(6.0 / (rows + cols))
            return gpu.Matrix(rs.uniform(-bound, bound, size=(rows, cols)).astype(np.float32))

        params = [uniform(items, 3 * H), uniform(H, 3 * H), gpu.Matrix(np.zeros((1, 3 * H), np.float32)), uniform(items, H + 1)]
        accs, h = [gpu.Matrix.zeros(*p.shape) for p in params], gpu.Matrix.zeros(BATCH, H)

        def call(n):
            ids = [rs.integers(0, items, (n, BATCH)).astype(np.int32) for _ in range(2)]
            ids += [(rs.random((n, BATCH)) < 0.1).astype(np.int32), rs.integers(0, items, (n, NEGATIVES)).astype(np.int32)]
            t0 = time.perf_counter()
            losses = gpu.gru_steps(params, accs, h, *ids, loss, 1.0, 0.05)
            return (time.perf_counter() - t0) * 1e3, float(losses[-1])

        call(steps)
        wall = sorted(call(1)[0] for _ in range(steps))
        queued = call(steps)[0] / steps
        gpu.Profiler.enable(True, only="gru_")
        gpu.Profiler.reset()
        last = [call(1)[1] for _ in range(steps)][-1]
        ms = {s: gpu.Profiler.get(s)[0] / steps for s in SCOPES}
        gpu.Profiler.enable(False)
        kernels = sum(ms.values())
        r = {"items": name, "n_items": items, "hidden": H, "loss": loss, "batch_size": BATCH, "negatives": NEGATIVES, "steps_timed": steps,
             "ms_per_call_of_one_step_median": round(wall[len(wall) // 2], 3), "ms_per_call_of_one_step_min": round(wall[0], 3),
             "ms_per_call_of_one_step_max": round(wall[-1], 3), "ms_per_queued_step": round(queued, 3),
             **{f"{s}_ms": round(v, 3) for s, v in ms.items()}, "kernels_ms": round(kernels, 3), "launches_per_step": LAUNCHES,
             "gap_share_of_queued_step": round(max(0.0, 1.0 - kernels / queued), 3), "last_loss": round(last, 4)}
        results.append(r)
        print(json.dumps(r), flush=True)
        del params, accs, h
        gpu.release_workspaces()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "gru4rec_bench"))
    ap.add_argument("--only", default=None, help="shape:hidden:loss[,...]")
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [(s.split(":")[0], int(s.split(":")[1]), s.split(":")[2]) for s in a.only.split(",")]
    results = run(configs, a.steps)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "gru4rec_bench.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
