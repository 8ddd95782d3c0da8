"""Hybrid WARP training on the device (imp_hybrid_warp_update / hybrid_warp_epoch, csrc/hybrid_warp.hip) and the model built on
it (implicit_amd.gpu.hybrid), judged against the float64 restatement of the contract in hybrid_warp_reference.py.  The
matrices, the planted problem and the margin filter are those of the BPR and WARP tests."""
import io
import pickle

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal
from scipy.sparse import csr_matrix, identity

import bpr_reference as bref
import hybrid_warp_reference as ref
import sgd_cases as sc
import warp_reference as wref
from test_gpu_bpr import _device_ids, _factors, _knn_ids, _planted, _rel, _small_matrix

pytestmark = pytest.mark.gpu

LR, REG = 0.05, 0.01
MARGIN = 1e-4  # test_gpu_warp.MARGIN
LONG = 70  # a feature row longer than the widest lane group (64): the walk's outer loop runs twice at every G


def _bound(F):
    """2e-6 is the project's bound for the WARP step; a representation adds an nf-term fp32 chain in front of it."""
    return 2e-6 * max(1.0, np.diff(F.indptr).max() / 4)


def _mixed_features(rows, rng):
    """rows x (rows + 90): row r is empty (r % 5 == 0), its own feature alone (1), or its own, a tag all these rows share and
    LONG - 2 more tags (2) or one of three (3, 4).  Weights in [0.5, 1.5)."""
    dense = np.zeros((rows, rows + 90), dtype=np.float32)
    for r in range(rows):
        cols = [] if r % 5 == 0 else [r] if r % 5 == 1 else [r, rows]
        if r % 5 == 2:
            cols += (rows + 4 + rng.choice(86, LONG - 2, replace=False)).tolist()
        if r % 5 > 2:
            cols += [rows + 1 + int(rng.integers(3))]
        dense[r, cols] = rng.uniform(0.5, 1.5, len(cols))
    return csr_matrix(dense)


def _check(Eg, E64, E0, touched, bound, what):
    for r in touched:
        assert _rel(Eg[r], E64[r]) < bound, (what, r, _rel(Eg[r], E64[r]))
    rest = np.array(sorted(set(range(E0.shape[0])) - set(touched)), dtype=np.int64)
    assert_array_equal(Eg[rest].view(np.uint32), E0[rest].view(np.uint32))


# ---- 1. single samples are exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sc.DISPATCH_C)  # both ends of every (lanes, columns per lane) instantiation
def test_single_steps_exact(gpu, C):
    """20 chained single-sample calls, max_sampled 6, seeds picked on the host for a closest margin >= 1e-4.  Among the feature
    rows of the updating samples: an empty row, a one-feature row, a row longer than a lane group holds, and a positive and
    negative that share a feature."""
    m = _small_matrix()
    rows, items, max_sampled = wref.liked_sets(m), m.shape[1], 6
    rng = np.random.default_rng(C)
    UF, IF = _mixed_features(m.shape[0], rng), _mixed_features(items, rng)
    EUc, EIc = _factors(UF.shape[1], C, rng, bias=1.0), _factors(IF.shape[1], C, rng)
    EUc[:, :-1] *= 0.2
    EIc *= 0.2
    bias = EUc[:, -1].copy()
    uid, iid, ptr = _device_ids(gpu, m)
    dUF, dIF, EU, EI = gpu.CSRMatrix(UF), gpu.CSRMatrix(IF), gpu.Matrix(EUc), gpu.Matrix(EIc)
    done, seen, worst = 0, set(), 0.0
    for s in (int(v) for v in rng.integers(0, 2**62, 2000)):
        if done == 20:
            break
        (u,), (i,) = (v.tolist() for v in ref.positives(m, s, 1))
        cand = ref.candidates(s, 0, items, max_sampled)
        EU64, EI64 = EUc.astype(np.float64), EIc.astype(np.float64)
        t, trials, closest = ref.step64(EU64, EI64, UF, IF, rows[u], u, i, cand, LR, REG)
        if closest < MARGIN:
            continue
        got = gpu.hybrid_warp_epoch(uid, iid, ptr, dUF, dIF, EU, EI, LR, REG, s, max_sampled, samples=1)
        assert got == (int(t is None), trials), (s, got, t, trials)
        tu, ti = set(), set()
        if t is not None:
            j = int(cand[t - 1])
            fu, fi, fj = (set(ref.feature_row(F, r)[0].tolist()) for F, r in ((UF, u), (IF, i), (IF, j)))
            tu, ti = fu, fi | fj
            seen |= {len(f) if len(f) < 2 else "long" for f in (fu, fi, fj) if len(f) < 2 or len(f) == LONG}
            seen |= {"shared"} if fi & fj else set()
        EUg, EIg = EU.to_numpy(), EI.to_numpy()
        _check(EUg, EU64, EUc, tu, _bound(UF), "user feature")
        _check(EIg, EI64, EIc, ti, _bound(IF), "item feature")
        assert_array_equal(EUg[:, -1].view(np.uint32), bias.view(np.uint32))
        worst = max([worst] + [_rel(EUg[r], EU64[r]) for r in tu] + [_rel(EIg[r], EI64[r]) for r in ti])
        EUc, EIc, done = EUg, EIg, done + 1
    print(f"C={C}: worst relative distance of a touched row {worst:.3g} (bound {_bound(IF):.3g})")
    assert done == 20 and seen == {0, 1, "long", "shared"}, (done, seen)


@pytest.mark.parametrize("C", sc.DISPATCH_C)
def test_satisfied_sample_writes_nothing(gpu, C):
    """test_gpu_warp's construction with the biases set through the feature biases: every item has its own feature, whose
    bias is -4 outside the sampled user's row and 0 inside it, and a tag all items share; |dot| < 1 without the bias."""
    m = _small_matrix()
    users, items = m.shape
    rng = np.random.default_rng(1000 + C)
    IF = csr_matrix(np.hstack([np.eye(items), np.full((items, 1), 0.5)]).astype(np.float32))
    UF = identity(users, dtype=np.float32, format="csr")
    EU0, EI0 = _factors(users, C, rng) * np.float32(0.05), _factors(items + 1, C, rng) * np.float32(0.05)
    seed = 4242 + C
    (u,), _ = (v.tolist() for v in ref.positives(m, seed, 1))
    EI0[:, -1] = -4.0
    EI0[m.indices[m.indptr[u]:m.indptr[u + 1]], -1] = 0.0
    EI0[items, -1] = 0.0
    Y = IF.astype(np.float64) @ EI0.astype(np.float64)
    assert np.abs(EU0[:, :-1].astype(np.float64) @ Y[:, :-1].T).max() < 1.0
    uid, iid, ptr = _device_ids(gpu, m)
    dUF, dIF, EU, EI = gpu.CSRMatrix(UF), gpu.CSRMatrix(IF), gpu.Matrix(EU0), gpu.Matrix(EI0)
    for max_sampled in (1, 4, 5):
        assert gpu.hybrid_warp_epoch(uid, iid, ptr, dUF, dIF, EU, EI, LR, REG, seed, max_sampled, samples=1) == (1, max_sampled)
        assert_array_equal(EU.to_numpy(), EU0)
        assert_array_equal(EI.to_numpy(), EI0)


# ---- 2. a multi-sample call without conflicts is exact; identity features reproduce WARP -------------------------------------
@pytest.fixture(scope="module")
def sparse_matrix():
    from implicit_amd.synthetic import synthetic_csr

    m = synthetic_csr(4000, 20000, 60_000, gamma=1.0, seed=3)
    return m, wref.liked_sets(m)


def _two_features(rows):
    """rows x rows, two features per row from disjoint blocks: r // 2 in the lower half of the columns and a permuted one in the
    upper half, weights 1.0 and 0.5.  Every feature is carried by two rows."""
    half = rows // 2
    cols = np.stack([np.arange(rows) // 2, half + (np.arange(rows) * 7 + 3) % half], axis=1)
    data = np.tile(np.array([1.0, 0.5], dtype=np.float32), rows)
    return csr_matrix((data, cols.ravel(), 2 * np.arange(rows + 1)), shape=(rows, rows))


@pytest.mark.parametrize("C, plain", [(17, True), (257, True), (17, False), (101, False), (1024, False)])
def test_conflict_free_call_exact(gpu, C, plain, sparse_matrix):
    """test_gpu_warp's call: 64 samples, max_sampled 4, the first seed below 5000 whose samples touch no embedding row twice
    and keep every margin >= 1e-4.  plain: identity features, where the restatement must equal warp_reference.step64 on the
    same candidates; otherwise two features per row."""
    m, rows = sparse_matrix
    n, max_sampled, (users, items) = 64, 4, m.shape
    UF, IF = (identity(users, dtype=np.float32, format="csr"), identity(items, dtype=np.float32, format="csr")) if plain else \
        (_two_features(users), _two_features(items))
    rng = np.random.default_rng(C)
    EU0, EI0 = _factors(users, C, rng, bias=1.0), _factors(items, C, rng)
    EU64, EI64 = EU0.astype(np.float64), EI0.astype(np.float64)
    X64, Y64 = EU64.copy(), EI64.copy()  # WARP's own restatement, for the identity case
    for seed in range(1, 5000):
        us, iis = (v.tolist() for v in ref.positives(m, seed, n))
        tu = UF[us].indices.tolist()
        if len(set(tu)) < len(tu) or len(set(IF[iis].indices.tolist())) < IF[iis].nnz:
            continue
        satisfied = trials = 0
        examined, closest = list(iis), np.inf
        for s, (u, i) in enumerate(zip(us, iis)):
            cand = ref.candidates(seed, s, items, max_sampled)
            t, used, margin = ref.step64(EU64, EI64, UF, IF, rows[u], u, i, cand, LR, REG)
            if plain:
                assert wref.step64(X64, Y64, rows[u], u, i, cand, LR, REG)[:2] == (t, used)
            satisfied, trials, closest = satisfied + (t is None), trials + used, min(closest, margin)
            examined += [j for j in cand[:used].tolist() if j not in rows[u]]
        ti = IF[examined].indices.tolist()
        if len(set(ti)) == len(ti) and closest >= MARGIN:
            break
        EU64[tu], EI64[ti], X64[tu], Y64[ti] = EU0[tu], EI0[ti], EU0[tu], EI0[ti]  # as before this seed
    else:
        pytest.fail("no conflict-free seed found")
    assert satisfied < n  # the call does update
    if plain:
        assert_allclose(EU64, X64, rtol=1e-13, atol=0)  # float64 rounding: the two sum in different orders
        assert_allclose(EI64, Y64, rtol=1e-13, atol=0)
    uid, iid, ptr = _device_ids(gpu, m)
    EU, EI = gpu.Matrix(EU0), gpu.Matrix(EI0)
    got = gpu.hybrid_warp_epoch(uid, iid, ptr, gpu.CSRMatrix(UF), gpu.CSRMatrix(IF), EU, EI, LR, REG, seed, max_sampled, samples=n)
    assert got == (satisfied, trials)
    EUg = EU.to_numpy()
    _check(EUg, EU64, EU0, tu, _bound(UF), "user feature")
    _check(EI.to_numpy(), EI64, EI0, ti, _bound(IF), "item feature")
    assert (EUg[:, -1] == 1.0).all()


# ---- 3. learning and cold start -------------------------------------------------------------------------------------------
def _cold_auc(X, Y_cold, liked_cold):
    """Mean over users with both kinds of the share of (liked, not liked) pairs of cold items ranked in that order."""
    s = np.asarray(X, dtype=np.float64) @ np.asarray(Y_cold, dtype=np.float64).T
    aucs = [(s[u][liked_cold[u]][:, None] > s[u][~liked_cold[u]][None, :]).mean() for u in range(len(s))
            if liked_cold[u].any() and not liked_cold[u].all()]
    return float(np.mean(aucs))


def test_learning_and_cold_start(gpu):
    """The planted problem of the BPR tests with item features that carry its structure: the positive and the negative parts
    of the items' planted vectors, 16 features, no feature of an item's own.  Every fifth item is cold: its interactions are
    left out of training and it is ranked from represent_items alone.  Seeds 0 / 1 / 2, factors 8, lr 0.02, reg 0.01,
    max_sampled 10, 6 epochs.  The GPU model's cold-start AUC is held against the serial float64 SGD over the same draws
    and against a feature-free WARPMatrixFactorization, which knows nothing about a cold item.  Calibrated on the MI355X with
    16 samples in flight (hogwild_in_flight over the feature counts): the first measurement gave GPU - serial = -0.0052 /
    +0.0180 / -0.0215 (serial AUC 0.893 / 0.874 / 0.908, feature-free WARP 0.450 / 0.452 / 0.482); the margin, 0.0365, is
    the worst of the three plus 0.015 of slack for the run-to-run variation of Hogwild, as in test_gpu_warp (DESIGN.md
    4.21)."""
    import implicit_amd.gpu.warp as gwarp
    import implicit_amd.hybrid

    worst = 1.0
    for seed in range(3):
        train, held = _planted(seed)
        rng = np.random.default_rng(seed)
        V = (rng.standard_normal((300, 8)), rng.standard_normal((200, 8)))[1]  # _planted's item vectors: its first draws
        full = train.toarray() > 0
        full[np.arange(300), held] = True
        cold = np.arange(200) % 5 == 4
        IF = csr_matrix(np.hstack([np.maximum(V, 0), np.maximum(-V, 0)]).astype(np.float32))
        warm = csr_matrix(np.where(cold[None, :], 0, full).astype(np.float32))
        args = dict(factors=8, learning_rate=0.02, regularization=0.01, iterations=6, max_sampled=10, random_state=seed)
        model = implicit_amd.hybrid.HybridWARP(**args)
        model.fit(warm, item_features=IF, show_progress=False)
        auc_gpu = _cold_auc(model.user_factors.to_numpy(), model.represent_items(IF[cold]).to_numpy(), full[:, cold])
        EU0, EI0, rs = bref.init_factors(csr_matrix(np.ones((300, 16), dtype=np.float32)), 8, seed)
        seeds = [rs.integers(2**31) for _ in range(6)]
        UF = identity(300, dtype=np.float32, format="csr")
        EU, EI, _ = ref.serial_epochs(warm, UF, IF, EU0, EI0, seeds, 0.02, 0.01, 10)
        X = EU.copy()
        X[:, -1] = 1.0
        auc_ser = _cold_auc(X, IF[cold].astype(np.float64) @ EI, full[:, cold])
        plain = gwarp.WARPMatrixFactorization(**args)
        plain.fit(warm, show_progress=False)
        auc_plain = _cold_auc(plain.user_factors.to_numpy(), plain.item_factors.to_numpy()[cold], full[:, cold])
        print(f"seed {seed}: cold-start AUC gpu {auc_gpu:.4f} serial {auc_ser:.4f} (diff {auc_gpu - auc_ser:+.4f}), "
              f"feature-free WARP {auc_plain:.4f}")
        worst = min(worst, auc_gpu - auc_ser)
        assert auc_ser > 0.7 and auc_gpu > auc_plain + 0.1
    assert worst > -0.0365


# ---- 4. the model and the argument errors -----------------------------------------------------------------------------------
def test_model_surface(gpu, tmp_path):
    import implicit_amd.gpu.hybrid as ghybrid
    import implicit_amd.hybrid

    m = _small_matrix()
    rng = np.random.default_rng(5)
    UF, IF = _mixed_features(m.shape[0], rng), _mixed_features(m.shape[1], rng)
    model = implicit_amd.hybrid.HybridWARP(factors=16, learning_rate=0.001, iterations=3, max_sampled=7, random_state=42)  # rows of 70 unnormalised features
    model.fit(m, UF, IF, show_progress=False)
    EU, EI = model.user_embeddings.to_numpy(), model.item_embeddings.to_numpy()
    X, Y = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    want_x = UF.astype(np.float64) @ EU.astype(np.float64)
    want_x[:, -1] = 1.0
    assert np.abs(X - want_x).max() < 1e-5 and np.abs(Y - IF.astype(np.float64) @ EI.astype(np.float64)).max() < 1e-5
    assert_array_equal(model.item_feature_biases, EI[:, -1])
    assert_array_equal(model.user_feature_biases, EU[:, -1])
    assert_array_equal(model.represent_items(IF[5:9]).to_numpy(), Y[5:9])
    assert_array_equal(model.represent_users(UF[5:9]).to_numpy(), X[5:9])
    users = np.arange(m.shape[0])
    ids, _ = model.recommend(users, m, N=10, filter_already_liked_items=False)
    assert (ids == _knn_ids(gpu, Y, X, 10)).mean() > 0.99
    path = str(tmp_path / "hybrid.npz")
    model.save(path)
    buf = io.BytesIO()
    pickle.dump(model, buf)
    for again in (ghybrid.HybridWARP.load(path), pickle.loads(buf.getvalue())):
        assert (again.max_sampled, again.factors) == (7, 16)
        for name in ("user_embeddings", "item_embeddings", "user_factors", "item_factors"):
            assert_array_equal(getattr(again, name).to_numpy(), getattr(model, name).to_numpy())
        assert_array_equal(again.recommend(0, m[0], N=3)[0], model.recommend(0, m[0], N=3)[0])
    without = implicit_amd.hybrid.HybridWARP(factors=16, iterations=1, random_state=1)
    without.fit(m, show_progress=False)  # None: identity features
    assert without.user_embeddings.shape == (m.shape[0], 17) and without.item_embeddings.shape == (m.shape[1], 17)
    with pytest.raises(ValueError):
        model.fit(m, UF[:-1], IF, show_progress=False)
    with pytest.raises(ValueError):
        model.represent_items(IF[:, :-1])


def test_argument_errors(gpu):
    m = _small_matrix()
    users, items = m.shape
    uid, iid, ptr = _device_ids(gpu, m)
    rng = np.random.default_rng(3)
    UF, IF = gpu.CSRMatrix(_mixed_features(users, rng)), gpu.CSRMatrix(_mixed_features(items, rng))
    EU0, EI0 = _factors(users + 90, 17, rng, bias=1.0), _factors(items + 90, 17, rng)
    EU, EI = gpu.Matrix(EU0), gpu.Matrix(EI0)
    short_ids = gpu.IntVector(np.asarray(m.indices[:-1], dtype=np.int32))
    bad_items = np.asarray(m.indices, dtype=np.int32).copy()
    bad_items[len(bad_items) // 2] = items  # one past the last row of item_features
    bad_users = bref.coo_ids(m)[0].copy()
    bad_users[0] = -1
    bad_ptr = np.asarray(m.indptr, dtype=np.int32).copy()
    bad_ptr[5] = m.nnz + 1
    wide = gpu.Matrix(_factors(items + 90, 1025, rng))
    cases = [
        (ValueError, dict(max_sampled=0)), (ValueError, dict(max_sampled=5000)),
        (ValueError, dict(EI=gpu.Matrix(_factors(items + 90, 18, rng)))),  # column counts differ
        (ValueError, dict(EU=gpu.Matrix(_factors(users + 90, 1025, rng)), EI=wide)),  # more than 1024 columns
        (ValueError, dict(EU=EU.astype(np.float16), EI=EI.astype(np.float16))),  # not fp32
        (ValueError, dict(EU=gpu.Matrix(EU0[:-1]))), (ValueError, dict(EI=gpu.Matrix(EI0[:-1]))),  # rows are not UF / IF
        (ValueError, dict(UF=gpu.CSRMatrix(_mixed_features(users - 1, rng)), EU=gpu.Matrix(EU0[:-1]))),  # rows are not users
        (ValueError, dict(ptr=gpu.IntVector(np.asarray(m.indptr[:-1], dtype=np.int32)))), (ValueError, dict(iid=short_ids)),
        (IndexError, dict(iid=gpu.IntVector(bad_items))),  # also what an item_features with too few rows gives
        (IndexError, dict(uid=gpu.IntVector(bad_users))), (IndexError, dict(ptr=gpu.IntVector(bad_ptr))),
    ]
    for error, change in cases:
        a = dict(uid=uid, iid=iid, ptr=ptr, UF=UF, IF=IF, EU=EU, EI=EI, max_sampled=10)
        a.update(change)
        with pytest.raises(error):
            gpu.hybrid_warp_epoch(a["uid"], a["iid"], a["ptr"], a["UF"], a["IF"], a["EU"], a["EI"], LR, REG, 1, a["max_sampled"])
        assert_array_equal(EU.to_numpy().view(np.uint32), EU0.view(np.uint32))
        assert_array_equal(EI.to_numpy().view(np.uint32), EI0.view(np.uint32))
    empty = gpu.IntVector(np.zeros(0, np.int32))
    assert gpu.hybrid_warp_epoch(empty, empty, gpu.IntVector(np.zeros(users + 1, np.int32)), UF, IF, EU, EI, LR, REG, 1) == (0, 0)
