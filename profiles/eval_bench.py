"""Ranking metrics over a fitted model: implicit_amd.evaluation.ranking_metrics_at_k (ids stay on the device,
csrc/evaluation.hip) against the reference's compiled ranking_metrics_at_k driving the same model's recommend().

    python profiles/eval_bench.py [--config lastfm360k] [--scale 1.0] [--K 10] [--reps 2] [--batch-sizes 1000,8192,...] [--out FILE]

The synthetic matrix of the named shape is split 80 / 20 (train_test_split, seed 7), ALS (f = 64) runs a few iterations on
the train part, then both evaluations are timed in this one process with the host clock (each returns only after its
results are on the host).  The new path is timed per batch size; the reference's loop (batches of 1000 users, one
model.recommend, one download and a host hash-set walk each: evaluation.pyx:423-466) is timed where build/refsuite holds
its compiled module -- the only way to get that number for a model of this package.  The two dictionaries must agree to
1e-9 relative (two summation orders over n users differ by at most 2 n 2^-53).  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = os.path.join(ROOT, "build", "refsuite")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="lastfm360k")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch-sizes", default="1000,4096,16384,32768,65536,131072,400000")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import implicit_amd.gpu as gpu
        from implicit_amd import evaluation, synthetic
        from implicit_amd.gpu.als import AlternatingLeastSquares
    lines = []

    def emit(r):
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    C = synthetic.named(a.config, scale=a.scale)
    train, test = evaluation.train_test_split(C, 0.8, random_state=7)
    train, test = train.astype(np.float32), test.astype(np.float32)
    model = AlternatingLeastSquares(factors=64, iterations=a.iterations, random_state=11)
    model.fit(train, show_progress=False)
    users = int((np.diff(test.indptr) > 0).sum())
    emit({"config": a.config, "users": C.shape[0], "items": C.shape[1], "train_nnz": int(train.nnz), "test_nnz": int(test.nnz),
          "evaluated_users": users, "K": a.K, "factors": 64, "default_batch_size": evaluation.DEFAULT_BATCH_SIZE})

    def timed(fn):
        best, res = None, None
        for _ in range(a.reps):
            gpu.synchronize()
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, res

    evaluation.ranking_metrics_at_k(model, train, test, K=a.K, show_progress=False)  # warm-up: code objects, workspaces
    ours = None
    for bs in (int(b) for b in a.batch_sizes.split(",")):
        dt, res = timed(lambda: evaluation.ranking_metrics_at_k(model, train, test, K=a.K, show_progress=False, batch_size=bs))
        emit({"path": "implicit_amd.evaluation", "batch_size": bs, "seconds": dt, "users_per_s": users / dt, **res})
        if bs == evaluation.DEFAULT_BATCH_SIZE or ours is None:
            ours, ours_s = res, dt
    # where the time of the default configuration goes: the host side of a batch (scipy row slice of the train matrix)
    batch = np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)
    t0 = time.perf_counter()
    for s in range(0, len(batch), evaluation.DEFAULT_BATCH_SIZE):
        train[batch[s:s + evaluation.DEFAULT_BATCH_SIZE]]
    emit({"part": "train_user_items[batch] for every batch (host, scipy)", "seconds": time.perf_counter() - t0})
    t0 = time.perf_counter()
    evaluation._canonical_pattern(test)
    emit({"part": "canonical copy of the test pattern (host, scipy)", "seconds": time.perf_counter() - t0})

    if not a.no_reference and os.path.isdir(SUITE):
        sys.path.insert(0, SUITE)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            from implicit import evaluation as ref_evaluation
        ref_evaluation.ranking_metrics_at_k(model, train[:2000], test[:2000], K=a.K, show_progress=False)  # warm-up
        dt, ref = timed(lambda: ref_evaluation.ranking_metrics_at_k(model, train, test, K=a.K, show_progress=False))
        emit({"path": "reference evaluation.pyx over model.recommend", "batch_size": 1000, "seconds": dt, "users_per_s": users / dt,
              **ref})
        worst = max(abs(ours[k] - ref[k]) / abs(ref[k]) for k in ref)
        emit({"agreement": "max relative difference of the four metrics", "value": worst, "speedup": dt / ours_s})
        assert worst <= 1e-9, (ours, ref)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
