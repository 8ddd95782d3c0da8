"""GRU4Rec on the device (gru_gradients / gru_steps / gru_encode, csrc/gru4rec.hip) and its model, against the float64
restatement gru4rec_reference.py.  The tolerance of a compared array is 4 x the relative Frobenius distance between the float64
and the float32 run of the restatement on the case's own input (DESIGN.md 4.22's rule); for a single number it is never below
the spacing of float32 at that value."""
import io
import pickle

import numpy as np
import pytest

import gru4rec_reference as ref
from test_gru4rec_host import HYPER, MARGIN

pytestmark = pytest.mark.gpu

LOSSES = ("cross-entropy", "bpr-max")
NAMES = ("h1", "da", "dcol", "dh1", "dW_h", "db")


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def _within(name, got, low, want):
    """The rule, for one array or number; prints the two distances."""
    dist, tol = _rel(got, want), 4 * _rel(low, want)
    if np.ndim(want) == 0:
        tol = max(tol, float(np.spacing(np.float32(abs(want)))) / max(abs(float(want)), 1e-300))
    print(f"{name}: fp32 restatement from float64 {_rel(low, want):.3g}, device {dist:.3g}")
    assert np.isfinite(got).all() and dist <= tol, name


def _case(items, H, B, N, seed, steps=1, scale=0.4):
    """Per step: slots B - 2 and B - 1 idle, slots 0 .. 2 share input item 3, slots 4 and 5 share a target, reset mixed;
    negatives[0] is slot 7's target and negatives[1] = negatives[2]."""
    rng = np.random.default_rng(seed)
    params = [(rng.standard_normal(s) * scale).astype(np.float32) for s in ((items, 3 * H), (H, 3 * H), (1, 3 * H), (items, H + 1))]
    h = (rng.standard_normal((B, H)) * 0.5).astype(np.float32)
    inputs, targets = rng.integers(0, items, (steps, B)), rng.integers(0, items, (steps, B))
    reset, negatives = rng.integers(0, 2, (steps, B)), rng.integers(0, items, (steps, N))
    inputs[:, :3], targets[:, 5], reset[:, 0], reset[:, 1] = 3, targets[:, 4], 1, 0
    inputs[:, B - 2:], targets[:, B - 2:] = -1, -1
    if N:
        negatives[:, 0], negatives[:, 1] = targets[:, 7], negatives[:, 2]
    return params, h, [a.astype(np.int32) for a in (inputs, targets, reset, negatives)]


def _check_gradients(gpu, params, h, ids, loss):
    want = ref.gradients(params, h, *ids, loss, 0.8)
    low = ref.gradients(params, h, *ids, loss, 0.8, dtype=np.float32)
    got = gpu.gru_gradients([gpu.Matrix(p) for p in params], gpu.Matrix(h), *ids, loss, 0.8)
    for name in ("loss",) + NAMES:
        _within(name, got[name] if name == "loss" else got[name].to_numpy(), low[name], want[name])
    idle = ids[0] < 0
    assert (got["da"].to_numpy()[idle] == 0).all() and np.array_equal(got["h1"].to_numpy()[idle], h[idle])
    return want


# the cuts of the 32-column and 64-slot blocks and of the column tiles; the last case has fewer items than slots
GRADIENT_CASES = [(65, 32, 64, 0), (65, 96, 64, 64), (130, 512, 64, 64), (130, 32, 128, 192), (40, 96, 128, 64)]


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("items, H, B, N", GRADIENT_CASES)
def test_gradients_against_float64(gpu, items, H, B, N, loss):
    params, h, ids = _case(items, H, B, N, seed=items + H + B)
    _check_gradients(gpu, params, h, [a[0] for a in ids], loss)


@pytest.mark.parametrize("loss", LOSSES)
def test_extreme_scores(gpu, loss):
    """W_out scaled until the float64 scores of row 0 pass +80 and -80."""
    params, h, ids = _case(130, 32, 64, 64, seed=5)
    ids = [a[0] for a in ids]
    first = ref.gradients(params, h, *ids, loss)["scores"][0]
    params[3] = (params[3] * (81.0 / min(first.max(), -first.min()))).astype(np.float32)
    want = _check_gradients(gpu, params, h, ids, loss)
    assert want["scores"][0].max() >= 80 and want["scores"][0].min() <= -80


def _run_steps(gpu, params, h, ids, loss, calls):
    dev = [gpu.Matrix(p) for p in params]
    accs, hd = [gpu.Matrix.zeros(*p.shape) for p in params], gpu.Matrix(h)
    losses = [gpu.gru_steps(dev, accs, hd, *[a[cut] for a in ids], loss, 0.8, 0.05) for cut in calls]
    return [m.to_numpy() for m in dev + accs + [hd]], np.concatenate(losses)


@pytest.mark.parametrize("loss", LOSSES)
def test_chained_steps_against_float64(gpu, loss):
    params, h, ids = _case(40, 32, 64, 64, seed=9, steps=3)
    names = "W_x W_h b W_out acc_W_x acc_W_h acc_b acc_W_out h".split()
    for steps in (1, 3):
        state64, state32 = (params, [np.zeros(p.shape) for p in params], h), (params, [np.zeros(p.shape) for p in params], h)
        want_loss = []
        for t in range(steps):
            value, *state64 = ref.adagrad_step(*state64, *[a[t] for a in ids], loss, 0.8, 0.05)
            _, *state32 = ref.adagrad_step(*state32, *[a[t] for a in ids], loss, 0.8, 0.05, dtype=np.float32)
            want_loss.append(value)
        got, losses = _run_steps(gpu, params, h, ids, loss, [slice(0, steps)])
        for name, g, low, want in zip(names, got, state32[0] + state32[1] + [state32[2]], state64[0] + state64[1] + [state64[2]]):
            _within(f"T={steps} {name}", g, low, want)
        np.testing.assert_allclose(losses, want_loss, rtol=1e-5)
    again, losses_again = _run_steps(gpu, params, h, ids, loss, [slice(0, 3)])
    one_by_one, losses_single = _run_steps(gpu, params, h, ids, loss, [slice(t, t + 1) for t in range(3)])
    for name, a, b, c in zip(names, got, again, one_by_one):
        assert np.array_equal(a, b) and np.array_equal(a, c), name
    assert np.array_equal(losses, losses_again) and np.array_equal(losses, losses_single)


def _sessions(items, seed, n=130):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, items, (0, 1, 2, 70)[s % 4]).astype(np.int32) for s in range(n)]


def test_encode(gpu):
    params, _, _ = _case(65, 96, 64, 0, seed=2, scale=0.1)  # small weights: a contracting recurrence over 70 steps
    sessions = _sessions(65, 4)
    indptr = np.concatenate([[0], np.cumsum([len(s) for s in sessions])])
    got = gpu.gru_encode(indptr, np.concatenate(sessions), *[gpu.Matrix(p) for p in params[:3]]).to_numpy()
    _within("encode", got, ref.encode(sessions, *params[:3], dtype=np.float32), ref.encode(sessions, *params[:3]))
    assert (got[::4, :96] == 0).all() and (got[:, 96] == 1).all()  # the empty sessions: exactly [0 | 1]
    assert gpu.gru_encode(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), *[gpu.Matrix(p) for p in params[:3]]).shape == (0, 97)


def _model(gpu, params, **kwargs):
    import implicit_amd.gru4rec

    model = implicit_amd.gru4rec.GRU4Rec(hidden=params[1].shape[0], **kwargs)
    model.W_x, model.W_h, model.b, model.item_factors = (gpu.Matrix(p) for p in params)
    return model


@pytest.mark.parametrize("filter_seen", [False, True])
def test_serving(gpu, filter_seen):
    params, _, _ = _case(300, 32, 64, 0, seed=11)
    sessions = [s for s in _sessions(300, 6, 256) if len(s)][:64]
    model = _model(gpu, params)
    scores = ref.encode(sessions, *params[:3]) @ params[3].astype(np.float64).T
    if filter_seen:
        for r, s in enumerate(sessions):
            scores[r, s] = -np.inf
    ranked = np.sort(scores, axis=1)[:, ::-1]
    assert (ranked[:, 9] - ranked[:, 10]).min() >= 1e-4  # the gap at the cut, well above float32 error
    ids, _ = model.recommend_sessions(sessions, N=10, filter_seen=filter_seen)
    assert np.array_equal(np.sort(ids, axis=1), np.sort(np.argsort(-scores, axis=1)[:, :10], axis=1))
    assert _rel(model.encode_sessions(sessions).to_numpy(), ref.encode(sessions, *params[:3])) < 1e-5


def test_persistence_and_recalculate(gpu):
    params, _, _ = _case(65, 32, 64, 0, seed=12)
    model = _model(gpu, params, loss="cross-entropy", random_state=3)
    model.user_factors = model.encode_sessions(_sessions(65, 1, 8))
    buffer = io.BytesIO()
    model.save(buffer)
    buffer.seek(0)
    for copy in (type(model).load(buffer), pickle.loads(pickle.dumps(model))):
        assert copy.loss == "cross-entropy" and copy.hidden == 32
        for name, p in zip(("W_x", "W_h", "b", "item_factors"), params):
            assert np.array_equal(getattr(copy, name).to_numpy(), p), name
        assert np.array_equal(copy.user_factors.to_numpy(), model.user_factors.to_numpy())
    from scipy.sparse import csr_matrix

    with pytest.raises(ValueError, match="recommend_sessions"):
        model.recommend(0, csr_matrix((1, 65), dtype=np.float32), recalculate_user=True)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_learning_against_float64(gpu, seed):
    """The model's fit against the float64 restatement trained on the same schedule and negatives: hit rate@1 of 200 held-out
    sessions within 0.05 (ten flipped near-ties), where test_gru4rec_host shows the restatement reaches 0.9 and float32 stays
    within half the margin.  Measured on the MI355X, seeds 0 / 1 / 2: DESIGN.md 4.27."""
    import implicit_amd.gru4rec

    train, held = ref.planted(seed)
    losses = []
    model = implicit_amd.gru4rec.GRU4Rec(random_state=seed, steps_per_call=16, **HYPER)
    model.fit(train, n_items=40, show_progress=False, callback=lambda epoch, elapsed, loss: losses.append(loss))
    ids, _ = model.recommend_sessions([s[:-1] for s in held], N=1)
    rate_gpu = float((ids[:, 0] == np.array([s[-1] for s in held])).mean())
    params, loss64 = ref.fit(train, 40, seed, **HYPER)
    rate_ref = ref.hit_rate(held, *params)
    print(f"seed {seed}: hit rate@1 gpu {rate_gpu:.4f} float64 {rate_ref:.4f}; last epoch's loss gpu {losses[-1]:.6f} float64 {loss64:.6f}")
    assert model.user_factors.shape == (len(train), 33)
    assert abs(rate_gpu - rate_ref) <= MARGIN


def test_errors_leave_the_parameters_alone(gpu):
    params, h, ids = _case(65, 32, 64, 64, seed=13)
    dev, hd = [gpu.Matrix(p) for p in params], gpu.Matrix(h)
    accs = [gpu.Matrix.zeros(*p.shape) for p in params]

    def steps(inputs=ids[0], targets=ids[1], reset=ids[2], negatives=ids[3], loss="bpr-max", p=dev, a=accs, state=hd):
        return gpu.gru_steps(p, a, state, inputs, targets, reset, negatives, loss, 1.0, 0.1)

    def edited(a, at, value):
        a = a.copy()
        a[0, at] = value
        return a

    bad_shape = [gpu.Matrix.zeros(65, 3 * 48), gpu.Matrix.zeros(48, 3 * 48), gpu.Matrix.zeros(1, 3 * 48), gpu.Matrix.zeros(65, 49)]
    invalid = [dict(loss="top1"), dict(negatives=ids[3][:, :32]), dict(inputs=ids[0][:, :32], targets=ids[1][:, :32], reset=ids[2][:, :32]),
               dict(p=bad_shape, a=bad_shape), dict(a=dev), dict(state=gpu.Matrix.zeros(64, 64)), dict(targets=edited(ids[1], 0, -1)),
               dict(a=[gpu.Matrix.zeros(2, 2)] + accs[1:]), dict(a=[m.astype("float16") for m in accs])]
    outside = [dict(inputs=edited(ids[0], 1, 65)), dict(inputs=edited(ids[0], 1, -2)), dict(targets=edited(ids[1], 1, 65)),
               dict(negatives=edited(ids[3], 3, -1)), dict(negatives=edited(ids[3], 3, 65))]
    for error, cases in ((ValueError, invalid), (IndexError, outside)):
        for kwargs in cases:
            with pytest.raises(error):
                steps(**kwargs)
    with pytest.raises(ValueError):
        gpu.gru_gradients(dev, hd, ids[0][0], edited(ids[1], 0, -1)[0], ids[2][0], ids[3][0], "bpr-max")
    with pytest.raises(IndexError):
        gpu.gru_encode(np.array([0, 2]), np.array([1, 65], dtype=np.int32), *dev[:3])
    with pytest.raises(ValueError):
        gpu.gru_encode(np.array([0, 2]), np.array([1, 2], dtype=np.int32), dev[0], dev[1], dev[3])
    for m, before in zip(dev + accs + [hd], params + [np.zeros_like(p) for p in params] + [h]):
        assert np.array_equal(m.to_numpy(), before)
