"""Mult-VAE on the device (vae_gradients / vae_step / vae_encode, csrc/mult_vae.hip) and its model, against the float64
restatement vae_reference.py fed the device's own draws.  The tolerance of an exactness case is 4 x the relative Frobenius
distance between the float64 and the float32 run of the restatement on the case's own input (DESIGN.md 4.22's rule), per array."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import vae_reference as ref

pytestmark = pytest.mark.gpu

STAGES = ("mu_lv", "dh2") + ref.NAMES + ("nll", "kl")
PARAM_NAMES = "W_in b_in W_lat b_lat W_dec b_dec W_out".split()


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def _case(items, H, L, B, seed):
    """B + 2 users: row 1 holds every item, every other non-empty row up to 12 items and item 0; the batch is rows 0 .. B - 5,
    then two stored rows without an entry and two ids of -1.  Some log-variances reach about +-8 (random_params)."""
    rng = np.random.default_rng(seed)
    dense = np.zeros((B + 2, items), dtype=np.float32)
    for u in range(B - 4):
        dense[u, rng.choice(items, size=min(items, int(rng.integers(1, 13))), replace=False)] = 1.0
    dense[:B - 4, 0] = 1.0
    dense[1] = 1.0
    rows = np.concatenate([np.arange(B - 4), [B, B + 1, -1, -1]]).astype(np.int32)
    return csr_matrix(dense), rows, ref.random_params(rng, items, H, L)


def _host(out):
    return {k: v if isinstance(v, float) else v.to_numpy() for k, v in out.items()}


def _assert_close(got, want, low, names, what=""):
    for name in names:
        print(f"{what}{name}: fp32 restatement from float64 {_rel(low[name], want[name]):.3g}, device {_rel(got[name], want[name]):.3g}")
    for name in names:
        assert np.isfinite(got[name]).all(), name
        assert _rel(got[name], want[name]) <= 4 * _rel(low[name], want[name]), name


# one tile in every dimension; three tiles, two row blocks, 2L no power of two; L > H, largest L; largest H, beta 0; both maxima.
# The last entry seeds the input: the first seed at which the float32 restatement's nll and kl are each 2^-24 or more (relative)
# from float64 -- below that, 4 x their distance asks for less than the one rounding of a float32 result.
GRADIENT_CASES = [(65, 32, 32, 64, 0.5, 0.2, 1), (129, 96, 96, 128, 0.5, 1.0, 0), (65, 32, 256, 64, 0.0, 0.2, 1),
                  (129, 512, 32, 64, 0.5, 0.0, 1), (130, 512, 256, 128, 0.0, 0.2, 0)]


@pytest.mark.parametrize("items, H, L, B, dropout, beta, case_seed", GRADIENT_CASES)
def test_gradients_and_draws(gpu, items, H, L, B, dropout, beta, case_seed):
    m, rows, params = _case(items, H, L, B, case_seed)
    seed = 1000 + items
    dev = gpu.CSRMatrix(m), rows, [gpu.Matrix(p) for p in params], dropout, seed, beta
    got, again = _host(gpu.vae_gradients(*dev)), _host(gpu.vae_gradients(*dev))
    draw = np.abs(got["eps"] - ref.draws(B, L, seed)).max()
    print(f"draw: largest |eps - float64 rule| {draw:.3g}; lv in {got['mu_lv'][:, L:].min():.2f} .. {got['mu_lv'][:, L:].max():.2f}")
    assert draw <= 1e-5
    want = ref.gradients(m, rows, params, dropout, seed, beta, got["eps"])
    low = ref.gradients(m, rows, params, dropout, seed, beta, got["eps"], dtype=np.float32)
    assert want["mu_lv"][:, L:].max() > 7 and want["mu_lv"][:, L:].min() < -7 and m[1].nnz == items
    _assert_close(got, want, low, STAGES)
    for name in ("eps", "mu_lv", "dW_lat", "dW_dec", "dh2"):
        assert np.array_equal(got[name], again[name]), name


def test_sampling_off_and_empty_slots(gpu):
    m, rows, params = _case(65, 32, 32, 64, seed=0)  # chosen as GRADIENT_CASES' seeds are
    dev = [gpu.Matrix(p) for p in params]
    got = _host(gpu.vae_gradients(gpu.CSRMatrix(m), rows, dev, 0.5, 7, 0.2, sample=False))
    assert not got["eps"].any()
    want = ref.gradients(m, rows, params, 0.5, 7, 0.2, None)  # z is mu itself
    _assert_close(got, want, ref.gradients(m, rows, params, 0.5, 7, 0.2, None, dtype=np.float32), STAGES, "sample 0 ")
    empty = np.where(np.arange(64) % 2, -1, 64).astype(np.int32)  # ids of -1 and a stored row without an entry
    got = _host(gpu.vae_gradients(gpu.CSRMatrix(m), empty, dev, 0.5, 7, 0.2))
    assert got["kl"] == 0 and got["nll"] == 0 and not got["dW_lat"].any() and not got["db_lat"].any()


@pytest.mark.parametrize("steps", [1, 3])
def test_chained_steps_against_float64(gpu, steps):
    m, rows, params = _case(130, 32, 32, 64, seed=9)
    hyper = dict(lr=0.01, reg=0.01)
    csr, dev = gpu.CSRMatrix(m), [gpu.Matrix(p) for p in params]
    dev_moments = [gpu.Matrix.zeros(*p.shape) for p in params for _ in range(2)]
    p64, m64 = params, [np.zeros(p.shape) for p in params for _ in range(2)]
    p32, m32 = params, [np.zeros(p.shape, dtype=np.float32) for p in params for _ in range(2)]
    for t in range(1, steps + 1):
        beta = 0.1 * t
        eps = gpu.vae_gradients(csr, rows, dev, 0.5, 40 + t, beta)["eps"].to_numpy()
        _, _, p64, m64 = ref.adam_step(m, rows, p64, m64, 0.5, 40 + t, beta, eps, step=t, **hyper)
        _, _, p32, m32 = ref.adam_step(m, rows, p32, m32, 0.5, 40 + t, beta, eps, step=t, dtype=np.float32, **hyper)
        gpu.vae_step(csr, rows, dev, dev_moments, 0.5, 40 + t, beta, hyper["lr"], t, hyper["reg"])
    names = PARAM_NAMES + [f"{k}_{n}" for n in PARAM_NAMES for k in "mv"]
    got, want, low = (dict(zip(names, x)) for x in ([a.to_numpy() for a in dev + dev_moments], p64 + m64, p32 + m32))
    _assert_close(got, want, low, names)


ERRORS = dict(beta=(ValueError, dict(beta=-0.5)), dropout=(ValueError, dict(dropout=1.0)), step=(ValueError, dict(step=0)),
              row=(IndexError, dict(bad_row=66)), W_lat=(ValueError, dict(W_lat_cols=96)), b_dec=(ValueError, dict(b_dec_cols=64)),
              overlap=(ValueError, dict(alias=True)))


@pytest.mark.parametrize("what", sorted(ERRORS))
def test_argument_errors_write_nothing(gpu, what):
    error, kw = ERRORS[what]
    m, rows, params = _case(65, 32, 32, 64, seed=2)
    if "bad_row" in kw:
        rows[3] = kw["bad_row"]
    if "W_lat_cols" in kw:
        params[2] = np.ones((32, kw["W_lat_cols"]), dtype=np.float32)
    if "b_dec_cols" in kw:
        params[5] = np.ones((1, kw["b_dec_cols"]), dtype=np.float32)
    dev = [gpu.Matrix(p) for p in params]
    moments = [gpu.Matrix(np.full(p.shape, 0.25, dtype=np.float32)) for p in params for _ in range(2)]
    if kw.get("alias"):
        moments[1] = moments[0]
    with pytest.raises(error):
        gpu.vae_step(gpu.CSRMatrix(m), rows, dev, moments, kw.get("dropout", 0.5), 1, kw.get("beta", 0.2), 0.01, kw.get("step", 1))
    assert all(np.array_equal(d.to_numpy(), p) for d, p in zip(dev, params)) and all((a.to_numpy() == 0.25).all() for a in moments)
    if "beta" in kw:
        with pytest.raises(error):
            gpu.vae_gradients(gpu.CSRMatrix(m), rows, dev, 0.5, 1, kw["beta"])


# ---- the model --------------------------------------------------------------------------------------------------------------
def test_serving(gpu):
    import implicit_amd.vae

    params, sets = ref.serving_case()
    model = implicit_amd.vae.MultVAE(hidden=32, latent=32)
    for name, p in zip(PARAM_NAMES[:6] + ["item_factors"], params):
        setattr(model, name, gpu.Matrix(p))
    known = sets[0][0]
    model.user_factors = gpu.vae_encode(gpu.CSRMatrix(known), np.arange(64, dtype=np.int32), model._encoder())
    for ids_of, (rows, want, gap, _), recalc in ((np.arange(64), sets[0], False), (5000 + np.arange(20), sets[1], True)):
        assert gap >= 1e-4
        ids, _ = model.recommend(ids_of, rows, N=10, recalculate_user=recalc)
        assert np.array_equal(np.sort(ids, axis=1), np.sort(want, axis=1))
    assert _rel(model.user_factors.to_numpy(), ref.encode(known, np.arange(64), params)) < 1e-6
    candidates = np.arange(7, 500, 11)
    ids, got = model.rank_items(np.arange(64), None, candidates)
    np.testing.assert_allclose(got, np.take_along_axis(sets[0][3], ids.astype(np.int64), axis=1), rtol=1e-5, atol=1e-5)
    assert (np.diff(got, axis=1) <= 0).all() and (np.sort(ids, axis=1) == candidates).all()


HYPER = dict(hidden=32, latent=32, dropout=0.0, anneal_cap=0.2, learning_rate=0.01, regularization=0.0, batch_size=256, iterations=6)
LOSS_GAP, RECALL_GAP = 1e-3 + 1.3e-7, 0.005 + 0.0  # stated margin + worst gap measured in two runs


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_learning_against_float64(gpu, seed):
    """The model's fit on Mult-DAE's planted rank-8 problem against the float64 restatement stepped over the same batches from
    the same weights with the device's draws: the last epoch's mean NLL + beta KL and the held-out recall@20.  The asserted
    gaps are the margins stated for what another order of dW_in's atomic adds can move (1e-3 relative loss, 0.005 recall) plus
    the worst gaps measured in two runs.  Measured on the MI355X, seeds 0 / 1 / 2, both runs alike: float64 loss
    138.304 / 131.034 / 139.415, device - float64 relative +1.3e-7 / -6e-8 / +2e-9; recall@20 0.3423 / 0.4541 / 0.3257 on both sides,
    popularity 0.110 / 0.095 / 0.098."""
    import implicit_amd.vae
    from test_gpu_dae import _planted, _recall20

    train, held = _planted(seed)
    losses = []
    model = implicit_amd.vae.MultVAE(random_state=seed, **HYPER)
    model.fit(train, show_progress=False, callback=lambda epoch, elapsed, loss: losses.append(loss))
    ids, _ = model.recommend(np.arange(2048), train, N=20)
    recall_gpu = float((ids == held[:, None]).any(axis=1).mean())

    rs, H, L, B = np.random.default_rng(seed), HYPER["hidden"], HYPER["latent"], HYPER["batch_size"]  # fit's draws, in fit's order
    shapes = [(1024, H), (1, H), (H, 2 * L), (1, 2 * L), (L, H), (1, H)]
    params = [np.zeros(s) if s[0] == 1 else (rs.standard_normal(s) * np.sqrt(2.0 / sum(s))).astype(np.float32) for s in shapes]
    params.append((rs.standard_normal((1024, H + 1)) * np.sqrt(2.0 / (1024 + H))).astype(np.float32))
    params[6][:, H] = 0.0
    moments, step = [np.zeros(p.shape) for p in params for _ in range(2)], 0
    nothing = gpu.CSRMatrix(csr_matrix(np.ones((1, 1), dtype=np.float32))), np.full(B, -1, dtype=np.int32)  # eps depends on (seed, slot, l) only
    tiny = [gpu.Matrix(np.zeros(s, dtype=np.float32)) for s in [(1, H)] + shapes[1:] + [(1, H + 1)]]
    for _ in range(HYPER["iterations"]):
        order, epoch = rs.permutation(2048), []
        for b in range(0, 2048, B):
            step += 1
            draw, beta = rs.integers(2**31), HYPER["anneal_cap"] * min(1.0, step / 9)  # the ramp: a fifth of 48 steps
            eps = gpu.vae_gradients(*nothing, tiny, 0.0, draw)["eps"].to_numpy()
            nll, kl, params, moments = ref.adam_step(train, order[b:b + B], params, moments, 0.0, draw, beta, eps, HYPER["learning_rate"], step)
            epoch.append(nll + beta * kl)
    recall_ref = _recall20(ref.encode(train, np.arange(2048), params) @ params[6].T, train, held)
    popularity = _recall20(np.tile(np.asarray(train.sum(axis=0)), (2048, 1)), train, held)
    print(f"seed {seed}: loss gpu {losses[-1]:.6f} float64 {np.mean(epoch):.6f} relative {losses[-1] / np.mean(epoch) - 1:.2g}; "
          f"recall@20 gpu {recall_gpu:.4f} float64 {recall_ref:.4f} popularity {popularity:.4f}")
    assert recall_gpu > popularity and recall_ref > popularity
    assert abs(losses[-1] - np.mean(epoch)) <= LOSS_GAP * np.mean(epoch)
    assert abs(recall_gpu - recall_ref) <= RECALL_GAP
