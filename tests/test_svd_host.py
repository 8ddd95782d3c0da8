"""The yardsticks of tests/test_gpu_svd.py hold on their own (no device): the float32 restatement of the randomized SVD finds
the rank of a rank-deficient matrix and sits within a few ulps of sigma_1 of the float64 one, and spmm32 / multiply_bound
say what they claim.  Figures read on a CPU when the tests were written are quoted next to each bound."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import svd_reference as ref


@pytest.fixture(scope="module")
def cases():
    return ref.driver_cases()


def test_rank12_float32_restatement_finds_the_rank(cases):
    A, k, p, q = cases["rank12"]
    U, sigma, V = ref.rsvd(A, k, p, q, ref.omega_for(A, k, p), np.float32)
    exact = np.linalg.svd(np.asarray(A.copy().todense(), dtype=np.float64), compute_uv=False)
    assert (exact[:12] > 1e-3 * exact[0]).all() and (exact[12:] < 1e-10 * exact[0]).all()  # the case has rank 12
    assert int((sigma > 0).sum()) == 12 and (sigma[:12] > 0).all()
    assert_array_equal(U[:, 12:], 0)
    assert_array_equal(V[:, 12:], 0)
    err = np.abs(sigma[:12] - exact[:12]).max() / exact[0]
    vdef = np.abs(V[:, :12].T.astype(np.float64) @ V[:, :12] - np.eye(12)).max()
    udef = np.abs(U[:, :12].T.astype(np.float64) @ U[:, :12] - np.eye(12)).max()
    print(f"rank12 float32: sigma err / sigma_1 {err:.3g} (probe 2.2e-7), defects V {vdef:.3g} (5e-7) U {udef:.3g} (1.1e-6)")
    assert err <= 2e-6
    assert vdef <= 1e-5 and udef <= 1e-5


def test_rank12_float64_restatement_is_exact(cases):
    A, k, p, q = cases["rank12"]
    _, sigma, _ = ref.rsvd(A, k, p, q, ref.omega_for(A, k, p), np.float64)
    exact = np.linalg.svd(np.asarray(A.copy().todense(), dtype=np.float64), compute_uv=False)
    assert int((sigma > 0).sum()) == 12
    assert np.abs(sigma[:12] - exact[:12]).max() <= 1e-12 * exact[0]


@pytest.mark.parametrize("name", ["generic300", "generic500", "longrow"])
def test_float32_restatement_tracks_float64(cases, name):
    A, k, p, q = cases[name]
    omega = ref.omega_for(A, k, p)
    U64, s64, V64 = ref.rsvd(A, k, p, q, omega, np.float64)
    U32, s32, V32 = ref.rsvd(A, k, p, q, omega, np.float32)
    m = ref.metrics(U32, s32, V32, U64, s64, V64)
    print(f"{name}: float32 against float64 restatement m1..m4 = {m} (probes of m1: 2.5e-7, 8e-8)")
    assert (s64 > 0).all() and (s32 > 0).all()
    assert m[0] <= 1e-5
    # the float64 restatement itself is orthonormal to rounding
    assert np.abs(V64.T @ V64 - np.eye(k)).max() <= 1e-12 and np.abs(U64.T @ U64 - np.eye(k)).max() <= 1e-12


def test_long_row_case_has_a_long_row(cases):
    A = cases["longrow"][0]
    assert A.shape == (301, 200) and np.diff(A.indptr).max() == 1500 > ref.SEGMENT


def test_spmm32_is_the_product():
    A = ref.spmm_case()
    lengths = np.diff(A.indptr)
    assert A.shape == (ref.SPMM_ROWS, ref.SPMM_COLS) and set(ref.SPMM_LENGTHS) <= set(lengths.tolist())
    long_rows = np.flatnonzero(lengths > ref.SEGMENT)
    assert any(lengths[r] == 0 for r in range(long_rows.min(), long_rows.max()))  # an empty row between long ones
    D = ref.dense_case(ref.SPMM_COLS, 5)
    out, exact = ref.spmm32(A, D)
    assert out.dtype == np.float32
    assert_array_equal(out[lengths == 0], 0)
    # scipy's operators may sum the duplicates of their operand in place: they only ever see copies
    dense_abs, dense = np.zeros(A.shape), np.zeros(A.shape)
    rows = np.repeat(np.arange(A.shape[0]), lengths)
    np.add.at(dense_abs, (rows, A.indices), np.abs(A.data).astype(np.float64))
    np.add.at(dense, (rows, A.indices), A.data.astype(np.float64))
    bound = (lengths[:, None] + 1) * 2.0**-24 * (dense_abs @ np.abs(D).astype(np.float64))
    assert (np.abs(out - exact) <= bound).all()
    np.testing.assert_allclose(exact, dense @ D.astype(np.float64), rtol=1e-12, atol=1e-12)
    # a row of at most one segment is the plain chain
    r = int(np.flatnonzero(lengths == 65)[0])
    s = np.zeros(5, dtype=np.float32)
    for e in range(A.indptr[r], A.indptr[r + 1]):
        s = s + A.data[e] * D[A.indices[e]]
    assert_array_equal(out[r], s)


def test_spmm32_exact_on_integers():
    A = ref.spmm_case(integer=True)
    D = ref.dense_case(ref.SPMM_COLS, 7, integer=True)
    out, exact = ref.spmm32(A, D)
    assert_array_equal(out.astype(np.float64), exact)
    At = ref.transpose_keeping_entries(A)
    assert At.nnz == A.nnz and np.diff(At.indptr).max() <= ref.SEGMENT
    np.testing.assert_array_equal(np.asarray(At.copy().todense()), np.asarray(A.copy().todense()).T)


def test_multiply_bound_covers_float32_blas():
    Y, W = ref.dense_case(65, 264), ref.dense_case(264, 256)
    exact, bound = ref.multiply_bound(Y, W)
    assert (np.abs((Y @ W).astype(np.float64) - exact) <= bound).all()
