"""Host-side checks of GRU4Rec that need no device: the float64 restatement's analytic gradients against central differences
of its own loss, the session-parallel schedule, the fold plan, and the planted problem the GPU learning test relies on."""
import warnings

import numpy as np
import pytest

import gru4rec_reference as ref

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    from implicit_amd.gpu.gru4rec import as_sessions, session_parallel_schedule


@pytest.mark.parametrize("loss", ["cross-entropy", "bpr-max"])
def test_analytic_gradients_against_central_differences(loss):
    """8 slots, slot 7 idle, slots 1 and 2 share a target (a masked column each), a negative equal to slot 0's target."""
    rng = np.random.default_rng(3)
    items, H, B = 9, 4, 8
    params = [rng.standard_normal(s) * 0.5 for s in ((items, 3 * H), (H, 3 * H), (1, 3 * H), (items, H + 1))]
    h = rng.standard_normal((B, H)) * 0.5
    inputs, targets = np.array([0, 1, 2, 2, 3, 4, 5, -1]), np.array([1, 6, 6, 3, 4, 5, 0, -1])
    reset, negatives = np.array([1, 0, 0, 1, 0, 0, 0, 0]), np.array([1, 7, 8, 8])
    out = ref.gradients(params, h, inputs, targets, reset, negatives, loss, 0.7)
    dense = [np.zeros(p.shape) for p in params]
    np.add.at(dense[0], inputs[:7], out["da"][:7])
    dense[1], dense[2] = out["dW_h"], out["db"]
    np.add.at(dense[3], out["cols"][out["cols"] >= 0], out["dcol"][out["cols"] >= 0])
    assert (out["g"] == 0).sum() > B + len(negatives) and (out["da"][7] == 0).all()
    for p, analytic in zip(params, dense):
        for at in [tuple(rng.integers(0, n) for n in p.shape) for _ in range(12)]:
            keep, eps = p[at], 1e-6
            p[at] = keep + eps
            up = ref.gradients(params, h, inputs, targets, reset, negatives, loss, 0.7)["loss"]
            p[at] = keep - eps
            down = ref.gradients(params, h, inputs, targets, reset, negatives, loss, 0.7)["loss"]
            p[at] = keep
            assert abs((up - down) / (2 * eps) - analytic[at]) <= 1e-7 + 1e-6 * abs(analytic[at])


@pytest.mark.parametrize("lengths, B", [([5, 1, 2, 9, 3, 2, 0, 4, 7, 2], 4), ([3, 2], 4), ([2] * 9, 4)])
def test_session_parallel_schedule(lengths, B):
    rng = np.random.default_rng(0)
    sessions = [np.arange(n) + 100 * s for s, n in enumerate(lengths)]  # item 100 s + t: session s, position t
    indptr, items = as_sessions(sessions)
    order = rng.permutation([s for s, n in enumerate(lengths) if n >= 2])
    inputs, targets, reset = session_parallel_schedule(indptr, items, order, B)
    live = inputs >= 0
    assert (targets[live] == inputs[live] + 1).all() and (targets[~live] == -1).all() and (reset[~live] == 0).all()
    pairs = sorted(inputs[live])
    assert pairs == sorted(100 * s + t for s, n in enumerate(lengths) for t in range(n - 1))  # each pair once
    assert np.array_equal(reset[live] == 1, inputs[live] % 100 == 0)  # exactly at a session's first pair
    for r in range(B):
        column = inputs[:, r]
        assert (np.diff(live[:, r].astype(int)) <= 0).all()  # idle only at the tail
        inside = column[live[:, r]]
        assert all(b == a + 1 or b % 100 == 0 for a, b in zip(inside, inside[1:]))  # in order within the slot


def test_fold_plan():
    import implicit_amd.gpu as gpu

    ids = np.array([5, 2, -1, 5, 9, 2, 5, -1, 0], dtype=np.int32)
    unique, start, occ = gpu.gru_fold_plan(ids)
    assert unique.tolist() == [0, 2, 5, 9] and start.tolist() == [0, 1, 3, 6, 7]
    assert occ.tolist() == [8, 1, 5, 0, 3, 6, 4]
    unique, start, occ = gpu.gru_fold_plan(np.full(3, -1, dtype=np.int32))
    assert len(unique) == 0 and start.tolist() == [0] and len(occ) == 0


HYPER = dict(hidden=32, loss="bpr-max", n_sample=64, sample_alpha=0.75, bpreg=1.0, learning_rate=0.1, batch_size=64, iterations=6)
MARGIN = 0.05  # test_gpu_gru4rec.test_learning_against_float64


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_problem_is_learnable_and_float32_is_enough(seed):
    train, held = ref.planted(seed)
    rate64 = ref.hit_rate(held, *ref.fit(train, 40, seed, **HYPER)[0])
    rate32 = ref.hit_rate(held, *ref.fit(train, 40, seed, dtype=np.float32, **HYPER)[0], dtype=np.float32)
    popular = np.bincount(np.concatenate(train), minlength=40).argmax()
    assert rate64 >= 0.9 and np.mean([s[-1] == popular for s in held]) <= 0.1
    assert abs(rate32 - rate64) < MARGIN / 2
