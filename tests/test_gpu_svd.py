"""PureSVD on the device (csrc/svd.hip, implicit_amd.gpu.randomized_svd, implicit_amd/svd.py) on the inputs of
tests/svd_reference.py.

spmm is bitwise defined and checked with zero tolerance against spmm32.  multiply_small is held to its documented bound
(l + 1) 2^-24 sum |y w| against float64, to exactness on integers and to equal bits on repeat.  The driver runs with a supplied
Omega against the float64 restatement with the same Omega; the yardstick of each metric is what the float32 restatement loses
on the same input, and the assertion m(gpu) <= max(2 m(float32), 2^-20): two stable orderings of the same sums differ by an
O(1) factor, and the floor covers a restatement that happens to round luckily."""
import io
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_equal

import serving_reference as serving
import svd_reference as ref
from implicit_amd.synthetic import synthetic_csr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- spmm: one answer ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spmm_inputs():
    """name -> (scipy matrix, its float32 / float64 answers per width, computed once and left unchanged)."""
    A = ref.spmm_case()
    mats = {"rows": A, "transposed": ref.transpose_keeping_entries(A)}
    want = {}
    for name, M in mats.items():
        for l in ref.SPMM_WIDTHS:
            D = ref.dense_case(M.shape[1], l)
            want[name, l] = (D,) + ref.spmm32(M, D)
    return mats, want


@pytest.mark.parametrize("l", ref.SPMM_WIDTHS)
@pytest.mark.parametrize("name", ["rows", "transposed"])
def test_spmm_bitwise(gpu, spmm_inputs, name, l):
    mats, want = spmm_inputs
    D, out32, _ = want[name, l]
    C, Dd = gpu.CSRMatrix(mats[name]), gpu.Matrix(D)
    got = gpu.spmm(C, Dd)
    assert got.shape == out32.shape
    first = got.to_numpy()
    assert_array_equal(bits(first), bits(out32))
    # into a buffer that held something else, empty rows included; equal bits on repeat
    out = gpu.Matrix(np.full(out32.shape, 7.0, dtype=np.float32))
    assert gpu.spmm(C, Dd, out=out) is out
    assert_array_equal(bits(out.to_numpy()), bits(first))
    assert_array_equal(bits(Dd.to_numpy()), bits(D))


def test_spmm_exact_on_integers(gpu):
    A = ref.spmm_case(integer=True)
    for M in (A, ref.transpose_keeping_entries(A)):
        for l in (3, 65):
            D = ref.dense_case(M.shape[1], l, integer=True)
            _, exact = ref.spmm32(M, D)
            got = gpu.spmm(gpu.CSRMatrix(M), gpu.Matrix(D)).to_numpy()
            assert_array_equal(got.astype(np.float64), exact)


def test_spmm_int64_offsets(gpu):
    A = ref.spmm_case()
    A64 = sp.csr_matrix((A.data, A.indices, A.indptr), shape=A.shape)
    A64.indptr = A64.indptr.astype(np.int64)  # the constructor would narrow it again
    assert A64.indptr.dtype == np.int64
    D = ref.dense_case(A.shape[1], 130)
    got = gpu.spmm(gpu.CSRMatrix(A64), gpu.Matrix(D)).to_numpy()
    assert_array_equal(bits(got), bits(ref.spmm32(A, D)[0]))


def test_spmm_no_entries(gpu):
    D = gpu.Matrix(ref.dense_case(9, 5))
    empty = sp.csr_matrix((4, 9), dtype=np.float32)
    assert_array_equal(gpu.spmm(gpu.CSRMatrix(empty), D, out=gpu.Matrix(np.ones((4, 5), dtype=np.float32))).to_numpy(), 0)


# ---- multiply_small -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,m", ref.MULTIPLY_SHAPES)
@pytest.mark.parametrize("rows", ref.MULTIPLY_ROWS)
def test_multiply_small_bound(gpu, rows, l, m):
    Y, W = ref.dense_case(rows, l), ref.dense_case(l, m, seed=6)
    Yd, Wd = gpu.Matrix(Y) if rows else gpu.Matrix.zeros(0, l), gpu.Matrix(W)
    got = gpu.multiply_small(Yd, Wd)
    assert got.shape == (rows, m)
    if rows == 0:
        return
    first = got.to_numpy()
    exact, bound = ref.multiply_bound(Y, W)
    err = np.abs(first.astype(np.float64) - exact)
    print(f"multiply_small {rows} x {l} x {m}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert (err <= bound).all()
    out = gpu.Matrix(np.full((rows, m), 7.0, dtype=np.float32))
    assert gpu.multiply_small(Yd, Wd, out=out) is out
    assert_array_equal(bits(out.to_numpy()), bits(first))


@pytest.mark.parametrize("l,m", ref.MULTIPLY_SHAPES)
def test_multiply_small_exact_on_integers(gpu, l, m):
    Y, W = ref.dense_case(65, l, integer=True), ref.dense_case(l, m, integer=True, seed=6)
    got = gpu.multiply_small(gpu.Matrix(Y), gpu.Matrix(W)).to_numpy()
    assert_array_equal(got.astype(np.float64), Y.astype(np.float64) @ W.astype(np.float64))


# ---- argument errors: ValueError, the output untouched -----------------------------------------------------------------------
def test_spmm_rejects(gpu):
    A = gpu.CSRMatrix(synthetic_csr(30, 20, 100, seed=1))
    f32 = lambda r, c: gpu.Matrix(np.full((r, c), 3.0, dtype=np.float32))  # noqa: E731
    f16 = lambda r, c: gpu.Matrix(np.full((r, c), 3.0, dtype=np.float16))  # noqa: E731
    square = gpu.CSRMatrix(synthetic_csr(20, 20, 100, seed=2))
    shared = f32(40, 4)
    bad = [(A, f16(20, 4), f32(30, 4)),       # D not fp32
           (A, f32(20, 4), f16(30, 4)),       # out not fp32
           (A, f32(19, 4), f32(30, 4)),       # D's rows are not A's columns
           (A, f32(20, 4), f32(29, 4)),       # out's rows are not A's rows
           (A, f32(20, 4), f32(30, 5)),       # out's columns are not D's
           (A, f32(20, 1025), f32(30, 1025)),  # l above 1024
           (A, gpu.Matrix.zeros(20, 0), f32(30, 4)),  # l below 1
           (square, shared[0:20], shared[10:30]),  # out overlaps D
           (square, shared[0:20], shared[0:20])]
    for csr, D, out in bad:
        before = out.to_numpy().copy()
        with pytest.raises(ValueError):
            gpu.spmm(csr, D, out=out)
        assert_array_equal(out.to_numpy(), before)
    # disjoint views of one allocation are fine
    got = gpu.spmm(square, shared[0:20], out=shared[20:40]).to_numpy()
    assert_array_equal(got, ref.spmm32(synthetic_csr(20, 20, 100, seed=2), np.full((20, 4), 3.0, dtype=np.float32))[0])


def test_spmm_rejects_row_blocks(gpu, monkeypatch):
    """More than 2^31 - 1 nonzeros arrive as row blocks (imp_csr_create64); IMP_CSR_PART_NNZ makes a small matrix take that
    form."""
    X = synthetic_csr(30, 20, 100, seed=1)
    X64 = X.copy()
    X64.indptr = X64.indptr.astype(np.int64)
    monkeypatch.setenv("IMP_CSR_PART_NNZ", "40")
    blocks = gpu.CSRMatrix(X64)
    monkeypatch.delenv("IMP_CSR_PART_NNZ")
    out = gpu.Matrix(np.full((30, 4), 3.0, dtype=np.float32))
    with pytest.raises(ValueError, match="2\\^31"):
        gpu.spmm(blocks, gpu.Matrix(np.ones((20, 4), dtype=np.float32)), out=out)
    assert_array_equal(out.to_numpy(), 3.0)


def test_multiply_small_rejects(gpu):
    f32 = lambda r, c: gpu.Matrix(np.full((r, c), 3.0, dtype=np.float32))  # noqa: E731
    f16 = lambda r, c: gpu.Matrix(np.full((r, c), 3.0, dtype=np.float16))  # noqa: E731
    shared = f32(40, 8)
    bad = [(f16(10, 8), f32(8, 4), f32(10, 4)),
           (f32(10, 8), f16(8, 4), f32(10, 4)),
           (f32(10, 8), f32(8, 4), f16(10, 4)),
           (f32(10, 8), f32(7, 4), f32(10, 4)),
           (f32(10, 8), f32(8, 4), f32(9, 4)),
           (f32(10, 8), f32(8, 4), f32(10, 5)),
           (f32(10, 1025), f32(1025, 4), f32(10, 4)),
           (f32(10, 8), f32(8, 1025), f32(10, 1025)),
           (gpu.Matrix.zeros(10, 0), gpu.Matrix.zeros(0, 4), f32(10, 4)),
           (shared[0:20], f32(8, 8), shared[10:30]),  # out overlaps Y
           (f32(10, 8), shared[0:8], shared[0:10])]   # out overlaps W
    for Y, W, out in bad:
        before = out.to_numpy().copy()
        with pytest.raises(ValueError):
            gpu.multiply_small(Y, W, out=out)
        assert_array_equal(out.to_numpy(), before)
    with pytest.raises(TypeError):
        gpu.multiply_small(np.ones((2, 2), dtype=np.float32), f32(2, 2))
    with pytest.raises(TypeError):
        gpu.spmm(synthetic_csr(30, 20, 100, seed=1), f32(20, 2))


# ---- the driver, against the float64 restatement with the same Omega ---------------------------------------------------------
@pytest.fixture(scope="module")
def driver_cases():
    """name -> (A, k, p, q, omega, float64 triplets, metrics of the float32 restatement)."""
    out = {}
    for name, (A, k, p, q) in ref.driver_cases().items():
        omega = ref.omega_for(A, k, p)
        t64 = ref.rsvd(A, k, p, q, omega, np.float64)
        out[name] = (A, k, p, q, omega, t64, ref.metrics(*ref.rsvd(A, k, p, q, omega, np.float32), *t64))
    return out


def device_svd(gpu, A, k, p, q, omega):
    At = ref.transpose_keeping_entries(A)
    U, sigma, V = gpu.randomized_svd(gpu.CSRMatrix(A), gpu.CSRMatrix(At), k, oversample=p, power_iterations=q, omega=gpu.Matrix(omega))
    assert U.shape == (A.shape[0], k) and V.shape == (A.shape[1], k)
    assert sigma.dtype == np.float64 and sigma.shape == (k,)
    return U.to_numpy(), sigma, V.to_numpy()


@pytest.mark.parametrize("name", ["rank12", "generic300", "generic500", "longrow"])
def test_driver_against_float64(gpu, driver_cases, name):
    A, k, p, q, omega, t64, m32 = driver_cases[name]
    U, sigma, V = device_svd(gpu, A, k, p, q, omega)
    assert (np.diff(sigma) <= 0).all()
    m = ref.metrics(U, sigma, V, *t64)
    limits = [max(2 * x, ref.FLOOR) for x in m32]
    print(f"{name}: m1..m4 gpu {m}\n  float32 restatement {m32}\n  gpu / limit {[a / b for a, b in zip(m, limits)]}")
    for got, limit in zip(m, limits):
        assert got <= limit


def test_driver_rank_deficient(gpu, driver_cases):
    A, k, p, q, omega, _, _ = driver_cases["rank12"]
    U, sigma, V = device_svd(gpu, A, k, p, q, omega)
    exact = np.linalg.svd(np.asarray(A.copy().todense(), dtype=np.float64), compute_uv=False)
    assert int((sigma > 0).sum()) == 12 and (sigma[:12] > 0).all()
    err = np.abs(sigma[:12] - exact[:12]).max() / exact[0]
    print(f"rank12: |sigma - exact| / sigma_1 = {err:.3g}")
    assert err <= 2e-6
    assert_array_equal(sigma[12:], 0)
    assert_array_equal(U[:, 12:], 0)
    assert_array_equal(V[:, 12:], 0)


def test_driver_rejects(gpu):
    X = synthetic_csr(30, 20, 100, seed=1)
    A, At = gpu.CSRMatrix(X), gpu.CSRMatrix(ref.transpose_keeping_entries(X))
    with pytest.raises(ValueError):
        gpu.randomized_svd(A, At, 1020, oversample=5)
    with pytest.raises(ValueError):
        gpu.randomized_svd(A, A, 4)
    with pytest.raises(ValueError):
        gpu.randomized_svd(A, At, 4, oversample=2, omega=gpu.Matrix.zeros(20, 5))


# ---- the model ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(gpu):
    from implicit_amd.svd import PureSVD

    X = synthetic_csr(300, 200, 3000, seed=7)
    model = PureSVD(factors=16, oversample=8, power_iterations=2, random_state=3)
    model.fit(X, show_progress=False)
    return model, X


def test_fit_is_deterministic_and_an_svd(gpu, fitted):
    from implicit_amd.svd import PureSVD

    model, X = fitted
    again = PureSVD(factors=16, oversample=8, power_iterations=2, random_state=3)
    again.fit(X, show_progress=False)
    assert_array_equal(bits(again.item_factors.to_numpy()), bits(model.item_factors.to_numpy()))
    assert_array_equal(bits(again.user_factors.to_numpy()), bits(model.user_factors.to_numpy()))
    assert_array_equal(again.singular_values, model.singular_values)
    assert model.item_factors.shape == (200, 16) and model.user_factors.shape == (300, 16)
    exact = np.linalg.svd(np.asarray(X.todense(), dtype=np.float64), compute_uv=False)[:16]
    # a randomized method never overestimates; with an oversample of 8 and two power iterations the float64 restatement reads
    # 0.948 .. 0.960 of the exact 16th value on this matrix over six Gaussian test matrices
    assert (model.singular_values <= exact * (1 + 1e-5)).all() and (model.singular_values >= 0.9 * exact).all()
    # user_factors = A V exactly as spmm defines it
    V = model.item_factors.to_numpy()
    assert_array_equal(bits(model.user_factors.to_numpy()), bits(ref.spmm32(X, V)[0]))


def test_recalculate_user_returns_the_stored_rows(gpu, fitted):
    model, X = fitted
    users = np.array([0, 7, 150, 299])
    stored = model.user_factors.to_numpy()[users]
    assert_array_equal(bits(model.recalculate_user(users, X[users]).to_numpy()), bits(stored))
    assert_array_equal(bits(model.recalculate_user(7, X[7]).to_numpy()), bits(stored[1:2]))
    items = model.recalculate_item(np.array([3, 4]), X.T.tocsr()[[3, 4]])
    assert items.shape == (2, 16)


def test_recommend_matches_float64_ranking(gpu, fitted):
    model, X = fitted
    Xf, Yf = model.user_factors.to_numpy(), model.item_factors.to_numpy()
    users = np.arange(40)
    for kw in (dict(N=10), dict(N=7, filter_already_liked_items=False)):
        got = model.recommend(users, X[users], **kw)
        want = serving.recommend(Xf, Yf, users, X[users], **kw)
        assert got[0].shape == want[0].shape
        np.testing.assert_allclose(got[1], want[1], rtol=1e-4, atol=1e-7)
        Q, Y = Xf[users].astype(np.float64), Yf.astype(np.float64)
        exceptions = serving.audit(got[0], want[0], want[1], lambda r, i: Q[r] @ Y[i], 16)
        assert exceptions <= 0.01 * got[0].size
    one = model.recommend(5, X[5], N=10)
    assert_array_equal(one[0], model.recommend(np.array([5]), X[5], N=10)[0][0])


def test_recommend_for_an_unseen_user(gpu, fitted):
    model, X = fitted
    row = sp.csr_matrix((np.array([1.0, 2.0, 1.0], dtype=np.float32), np.array([1, 5, 40], dtype=np.int32),
                         np.array([0, 3], dtype=np.int32)), shape=(1, 200))
    ids, scores = model.recommend(0, row, N=10, recalculate_user=True)
    Y = model.item_factors.to_numpy()
    q = ref.spmm32(row, Y)[0]
    want = serving.recommend(q, Y, 0, row, N=10)
    np.testing.assert_allclose(scores, want[1], rtol=1e-4, atol=1e-7)
    serving.audit(ids[None], want[0][None], want[1][None], lambda r, i: q[0].astype(np.float64) @ Y[i].astype(np.float64), 16)
    assert not set(ids.tolist()) & {1, 5, 40}


def test_save_load_and_pickle_round_trips(gpu, fitted, tmp_path):
    from implicit_amd.svd import PureSVD

    model, X = fitted
    want = model.recommend(np.arange(10), X[:10], N=5)
    path = str(tmp_path / "svd_model.npz")
    model.save(path)
    buf = io.BytesIO()
    model.save(buf)
    buf.seek(0)
    for other in (PureSVD.load(path), PureSVD.load(buf), pickle.loads(pickle.dumps(model))):
        assert (other.factors, other.oversample, other.power_iterations) == (16, 8, 2)
        assert_array_equal(other.singular_values, model.singular_values)
        assert_array_equal(bits(other.item_factors.to_numpy()), bits(model.item_factors.to_numpy()))
        assert_array_equal(bits(other.user_factors.to_numpy()), bits(model.user_factors.to_numpy()))
        got = other.recommend(np.arange(10), X[:10], N=5)
        assert_array_equal(got[0], want[0])
        assert_array_equal(bits(got[1]), bits(want[1]))


def test_refit_serves_the_new_model(gpu):
    """fit -> recommend -> fit on another matrix -> recommend: the second model's ids (the writers drop the top-k plane cache)."""
    from implicit_amd.svd import PureSVD

    X1, X2 = synthetic_csr(300, 200, 3000, seed=7), synthetic_csr(300, 200, 3000, seed=8)
    users = np.arange(20)
    model = PureSVD(factors=16, oversample=8, random_state=3)
    model.fit(X1, show_progress=False)
    first = model.recommend(users, X1[users], N=10)
    model.similar_items(3, N=5)
    model.fit(X2, show_progress=False)
    second = model.recommend(users, X2[users], N=10)
    fresh = PureSVD(factors=16, oversample=8, random_state=3)
    fresh.fit(X2, show_progress=False)
    want = fresh.recommend(users, X2[users], N=10)
    assert_array_equal(second[0], want[0])
    assert_array_equal(bits(second[1]), bits(want[1]))
    assert (first[0] != second[0]).any()
    a, b = model.similar_items(3, N=5), fresh.similar_items(3, N=5)
    assert_array_equal(a[0], b[0])


def test_writing_into_served_factors_drops_the_cache(gpu):
    """Both products write another model's factors over the matrices a model has just served from, in place."""
    from implicit_amd.svd import PureSVD

    X1, X2 = synthetic_csr(300, 200, 3000, seed=7), synthetic_csr(300, 200, 3000, seed=8)
    users = np.arange(20)
    model, other = PureSVD(factors=16, oversample=8, random_state=3), PureSVD(factors=16, oversample=8, random_state=3)
    model.fit(X1, show_progress=False)
    other.fit(X2, show_progress=False)
    first = model.recommend(users, X2[users], N=10)
    gpu.multiply_small(other.item_factors, gpu.Matrix(np.eye(16, dtype=np.float32)), out=model.item_factors)
    gpu.spmm(gpu.CSRMatrix(X2), other.item_factors, out=model.user_factors)
    assert_array_equal(model.item_factors.to_numpy(), other.item_factors.to_numpy())
    assert_array_equal(bits(model.user_factors.to_numpy()), bits(other.user_factors.to_numpy()))
    got, want = model.recommend(users, X2[users], N=10), other.recommend(users, X2[users], N=10)
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])
    assert (first[0] != got[0]).any()


def test_constructor_and_fit_errors(gpu):
    from implicit_amd.svd import PureSVD

    with pytest.raises(ValueError):
        PureSVD(factors=1020, oversample=10)
    with pytest.raises(NotImplementedError):
        PureSVD(factors=4).fit(synthetic_csr(30, 20, 100, seed=1), callback=lambda *a: None)
    assert not hasattr(PureSVD, "to_cpu")
