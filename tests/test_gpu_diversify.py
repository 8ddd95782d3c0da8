"""KnnQuery.diversify / diversify_items (csrc/diversify.hip) against tests/diversify_reference.py.  Picks and counts: exactly
the float64 restatement's, on inputs whose every pick is decided by a relative gap >= 1e-4 in that run (asserted; seeds found on
the CPU).  Gains: relative Frobenius distance from float64 within 4 x the float32 restatement's (tests/test_gpu_softmax.py)."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal
from scipy.sparse import csr_matrix

import diversify_reference as ref

pytestmark = pytest.mark.gpu

# (w, fp16, M, n, lists, seed).  Resident lists end at M = 4096 (w <= 8), 1024 (w = 33, 64), 512 (128), 256 (256), the small
# register form at a quarter of that (w <= 32: half); w = 256 with n = 259 keeps the basis in the device scratch.
CASES = [
    (1, False, 1, 1, 8, 0), (1, False, 2, 2, 8, 0), (1, False, 65, 4, 4, 0),
    (8, False, 63, 11, 2, 1), (8, False, 2049, 2, 2, 0), (8, False, 4096, 2, 2, 1),
    (33, True, 64, 36, 2, 1), (33, True, 65, 65, 2, 0), (33, True, 257, 2, 3, 0), (33, True, 1024, 1, 4, 1), (33, True, 1025, 36, 1, 1),
    (64, False, 256, 1, 8, 2), (64, False, 257, 67, 1, 0), (64, False, 1024, 2, 3, 0), (64, False, 1025, 2, 3, 0),
    (64, False, 4096, 2, 2, 0),
    (128, False, 2, 2, 4, 0), (128, False, 63, 131, 1, 0), (128, False, 129, 2, 3, 0), (128, False, 512, 2, 3, 1),
    (128, False, 513, 2, 3, 2),
    (256, False, 64, 64, 1, 0), (256, False, 65, 1, 8, 0), (256, False, 256, 259, 1, 13), (256, False, 257, 259, 1, 0),
]


def inputs(w, half, M, lists, seed):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((M + 9, w)).astype(np.float16 if half else np.float32)
    ids = [rng.permutation(M + 9)[:M].astype(np.int32) for _ in range(lists)]
    quality = [np.exp(rng.uniform(-1, 1, M)).astype(np.float32) for _ in range(lists)]
    return Y, ids, quality


def run(gpu, Y, ids, quality, n, rule, knn=None, **kw):
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in ids])])
    flat = lambda parts, dt: np.concatenate(parts).astype(dt) if len(parts) else np.zeros(0, dt)  # noqa: E731
    Y = Y if isinstance(Y, gpu.Matrix) else gpu.Matrix(Y)
    return (knn or gpu.KnnQuery()).diversify(Y, offsets, flat(ids, np.int32), flat(quality, np.float32), n, rule, **kw)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("rule", ["dpp", "mmr"])
@pytest.mark.parametrize("w, half, M, n, lists, seed", CASES)
def test_against_float64(gpu, w, half, M, n, lists, seed, rule):
    Y, ids, quality = inputs(w, half, M, lists, seed)
    ids64, gains64, counts64, closest = ref.batch(Y, ids, quality, n, rule)
    gains32 = ref.batch(Y, ids, quality, n, rule, dtype=np.float32)[1]
    assert closest >= 1e-4
    got_ids, got_gains, got_counts = run(gpu, Y, ids, quality, n, rule)
    made = ids64 >= 0
    print(f"fp32 restatement from float64: {rel(gains32[made], gains64[made]):.3g}; device: {rel(got_gains[made], gains64[made]):.3g}")
    assert_array_equal(got_counts, counts64)
    assert_array_equal(got_ids, ids64)
    assert (got_gains[~made] == -ref.FLT_MAX).all()
    if rule == "dpp" and n == w + 3:
        assert (counts64 == min(w, M)).all() and (got_ids[:, min(w, M):] == -1).all()
    assert rel(got_gains[made], gains64[made]) <= 4 * rel(gains32[made], gains64[made])


@pytest.mark.parametrize("rule", ["dpp", "mmr"])
@pytest.mark.parametrize("w, half, M", [(128, False, 100), (33, True, 300), (256, False, 256)])
def test_path_independence(gpu, w, half, M, rule):
    rng = np.random.default_rng(w)
    Y = gpu.Matrix(rng.standard_normal((5000, w)).astype(np.float16 if half else np.float32))
    mine, q = rng.permutation(5000)[:M].astype(np.int32), np.exp(rng.uniform(-1, 1, M)).astype(np.float32)
    others = [rng.integers(0, 5000, m).astype(np.int32) for m in (4096, 0, 7, 1500)]
    n = 40
    alone = run(gpu, Y, [mine], [q], n, rule)
    lists = others[:2] + [mine] + others[2:]
    qs = [np.ones(len(l), np.float32) for l in lists[:2]] + [q] + [np.ones(len(l), np.float32) for l in lists[3:]]
    batched = run(gpu, Y, lists, qs, n, rule)  # the 4096 list streams every list of the launch
    chunked = run(gpu, Y, lists, qs, n, rule, knn=gpu.KnnQuery(max_temp_memory=64 << 10))
    # streamed on its own: padding past every register form that can never be picked ahead of a real candidate
    pad = 4096 - M
    padded = run(gpu, Y, [np.concatenate([mine, np.zeros(pad, np.int32)])],
                 [np.concatenate([q, np.full(pad, 0.0 if rule == "dpp" else -ref.FLT_MAX, np.float32)])], n, rule)
    for other, row in ((batched, 2), (chunked, 2), (padded, 0)):
        assert_array_equal(other[0][row], alone[0][0])
        assert_array_equal(other[1][row].view(np.uint32), alone[1][0].view(np.uint32))
    assert_array_equal(batched[1].view(np.uint32), chunked[1].view(np.uint32))


def test_edges(gpu):
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((12, 8)).astype(np.float32)
    Y[3] = 0.0
    Y[7] = Y[6]
    ids = [[], [1, 2, 1, 4], [3, 5, 9], [5, 9, 10], [6, 7, 8]]
    quality = [[], [1.0, 0.5, 1.0, 0.8], [2.0, 1.0, 0.9], [1.0, 0.0, 0.7], [1.0, 1.0, 0.2]]
    got_ids, got_gains, counts = run(gpu, Y, [np.array(l, np.int32) for l in ids], [np.array(l, np.float32) for l in quality], 4, "dpp")
    assert_array_equal(counts, [0, 3, 2, 2, 2])
    assert (got_ids[0] == -1).all() and (got_gains[0] == -ref.FLT_MAX).all()  # the empty list
    assert sorted(got_ids[1][:3]) == [1, 2, 4] and got_ids[1][3] == -1         # the repeated id once
    assert sorted(got_ids[2][:2]) == [5, 9]                                    # never the zero row
    assert sorted(got_ids[3][:2]) == [5, 10]                                   # never the quality 0
    assert_array_equal(got_ids[4], [7, 8, -1, -1])                             # identical rows: the larger id, and only once
    mmr = run(gpu, Y, [np.array([6, 7, 8], np.int32)], [np.array([1.0, 1.0, 0.2], np.float32)], 3, "mmr", param=1.0)
    assert_array_equal(mmr[0][0], [7, 6, 8])


def test_liked_filter_through_the_model(gpu):
    model, liked, lists = _model(gpu)
    users = np.arange(4)
    dpp, _ = model.diversify_items(users, liked, lists, 6, filter_already_liked_items=True)
    mmr, _ = model.diversify_items(users, liked, lists, 30, rule="mmr", filter_already_liked_items=True)
    for u in users:
        mine = liked.indices[liked.indptr[u]:liked.indptr[u + 1]]
        hit = np.isin(lists[u], mine)
        assert hit.any() and not np.isin(dpp[u], mine).any()
        assert sorted(mmr[u][30 - hit.sum():]) == sorted(lists[u][hit])


BAD = {
    "offsets start": dict(offsets=[1, 3]), "offsets decrease": dict(offsets=[0, 3, 2]), "id": dict(cand=[0, 99, 2]),
    "negative id": dict(cand=[0, -1, 2]), "n": dict(n=0), "infinite": dict(quality=[1.0, np.inf, 1.0]),
    "nan": dict(quality=[1.0, np.nan, 1.0], rule=1), "negative": dict(quality=[1.0, -1.0, 1.0]), "long": dict(length=4097),
    "width": dict(width=1025), "rule": dict(rule=2), "lambda": dict(rule=1, param=1.5), "min_gain": dict(min_gain=1.0),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_refusals_write_nothing(gpu, what):
    from implicit_amd.gpu import _hip

    bad = BAD[what]
    length = bad.get("length", 3)
    items = gpu.Matrix(np.ones((20, bad.get("width", 8)), np.float32))
    offsets = np.array(bad.get("offsets", [0, length]), np.int64)
    cand = np.array(bad.get("cand", np.arange(length) % 20), np.int32)
    quality = np.array(bad.get("quality", np.ones(length)), np.float32)
    n = bad.get("n", 2)
    out = np.full((len(offsets) - 1) * max(n, 1), 77, np.int32), np.full((len(offsets) - 1) * max(n, 1), 77, np.float32), \
        np.full(len(offsets) - 1, 77, np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    status = _hip.lib().imp_knn_diversify(gpu.KnnQuery()._h, items._h, len(offsets) - 1, vp(offsets), vp(cand), vp(quality), n,
                                          bad.get("rule", 0), bad.get("param", 0.5), bad.get("min_gain", 1e-6), *map(vp, out))
    assert status == _hip.IMP_INVALID_ARGUMENT
    assert all((o == 77).all() for o in out)


def test_refusals_raise(gpu):
    model, liked, lists = _model(gpu)
    with pytest.raises(ValueError):
        gpu.KnnQuery().diversify(model.item_factors, [0, 3], [0, 999, 2], [1.0, 1.0, 1.0], 2)
    with pytest.raises(IndexError):
        model.diversify_items(0, None, [0, 1, 500], 2)
    with pytest.raises(ValueError):
        model.diversify_items(0, None, lists[0], 2, relevance_weight=1.0)


def _model(gpu):
    from implicit_amd.gpu.als import AlternatingLeastSquares

    rng = np.random.default_rng(9)
    model = AlternatingLeastSquares(factors=32)
    model.user_factors = gpu.Matrix(rng.standard_normal((6, 32)).astype(np.float32))
    model.item_factors = gpu.Matrix(rng.standard_normal((200, 32)).astype(np.float32))
    lists = np.stack([rng.permutation(200)[:30] for _ in range(4)]).astype(np.int32)
    rows = np.repeat(np.arange(4), 3)
    liked = csr_matrix((np.ones(12, np.float32), (rows, lists[:, [0, 7, 29]].reshape(-1))), shape=(4, 200))
    return model, liked, lists


@pytest.mark.parametrize("filtered", [False, True])
def test_model_layer(gpu, filtered):
    model, liked, lists = _model(gpu)
    users = np.arange(4)
    want = model.rank_items(users, liked, lists, N=30, filter_already_liked_items=filtered)
    got = model.diversify_items(users, liked, lists, 30, rule="mmr", relevance_weight=1.0, filter_already_liked_items=filtered)
    assert_array_equal(got[0], want[0])  # no diversity term: the plain order
    top, _ = model.diversify_items(users, liked, lists, 1, filter_already_liked_items=filtered)
    assert_array_equal(top[:, 0], want[0][:, 0])
    one = model.diversify_items(1, liked[1], lists[1], 5, filter_already_liked_items=filtered)
    many = model.diversify_items(users, liked, lists, 5, filter_already_liked_items=filtered)
    assert_array_equal(one[0], many[0][1])  # a scalar user: the row of the batch
    assert_array_equal(one[1].view(np.uint32), many[1][1].view(np.uint32))
