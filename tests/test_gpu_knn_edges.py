"""imp_sparse_topk_product (csrc/knn.hip) at its cuts, bit for bit: every case of tests/knn_cases.py against the float64
restatement knn_reference.product_topk, which tests/test_knn_cases_host.py proves bitwise equal to a literal triple loop on the
same cases.  The contract is bitwise (summation in A[r]'s stored order, every operation rounded separately, the total order
(score, column) descending), so every comparison is exact: counts, ids at every position, score bits at every position, the
(-1, -inf) padding included.  There is no tolerance, no tie tolerance and no budget of exceptions.

Not reached: the multi-chunk loop of imp_sparse_topk_product (r0 += chunk) starts only above about 1 GiB of output."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import knn_cases as kc
import knn_reference as kr

pytestmark = pytest.mark.gpu

_WANT = {}


def want(name):
    """The restatement's result of a case, computed once and shared."""
    if name not in _WANT:
        c = kc.get(name)
        _WANT[name] = kr.product_topk(c.A, c.B, c.k, c.zero_own)
    return _WANT[name]


def assert_bitwise(got, ref, what):
    gi, gs, gc = got
    wi, ws, wc = ref
    assert gi.dtype == np.int32 and gs.dtype == np.float64 and gc.dtype == np.int32 and gi.shape == wi.shape == gs.shape
    np.testing.assert_array_equal(gc, wc, err_msg=f"{what}: counts")
    np.testing.assert_array_equal(gi, wi, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(gs.view(np.int64), ws.view(np.int64), err_msg=f"{what}: score bits")


def run(gpu, c, B=None):
    return gpu.sparse_topk_product(gpu.SpMat(c.A), B if B is not None else gpu.SpMat(c.B), c.k, c.zero_own)


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_equals_the_restatement_bitwise(gpu, name):
    c = kc.get(name)
    B = gpu.SpMat(c.B)
    got = run(gpu, c, B)
    assert_bitwise(got, want(name), name)
    assert_bitwise(run(gpu, c, B), got, name + " run twice")
    if c.family not in kc.CUT_FAMILIES:
        return
    # every row alone in a one-row A: neither its company nor the dense worker that took it may show
    for r in range(c.A.shape[0]):
        alone = gpu.sparse_topk_product(gpu.SpMat(kc.one_row(c.A, r)), B, c.k, c.zero_own)
        assert_bitwise(alone, tuple(x[r:r + 1] for x in got), f"{name} row {r} alone")


def _num_cus():
    """multiProcessorCount of the current device, asked of the HIP runtime the library has loaded into this process."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    dev, cus = ctypes.c_int(-1), ctypes.c_int(0)
    multiprocessor_count = 63  # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert hip.hipGetDevice(ctypes.byref(dev)) == 0
    assert hip.hipDeviceGetAttribute(ctypes.byref(cus), multiprocessor_count, dev) == 0
    return cus.value


def test_dense_workers_are_reused(gpu):
    c = kc.get("dense_reuse_k20")
    cus = _num_cus()
    assert 32 <= cus <= 1024  # a compute-unit count, not another attribute
    workers = kc.dense_workers(cus, c.B.shape[1])
    assert c.A.shape[0] > 2 * workers  # every worker takes a third row after its second


def test_accumulator_state_across_calls(gpu):
    """The dense accumulators live in the context: kept at C = 4096 by the per-row reset alone when only B changes, allocated
    and filled anew for a larger C, filled anew for a smaller C that the allocation would hold, and again for the first."""
    results = []
    for name in kc.STATE_SEQUENCE:
        got = run(gpu, kc.get(name))
        assert_bitwise(got, want(name), f"state sequence, {name}")
        results.append(got)
    assert_bitwise(results[-1], results[0], "state sequence, last against first")


def _create(gpu, rows, cols, indptr, indices, data):
    from implicit_amd.gpu import _hip

    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int32), np.asarray(data, np.float64)
    h = ctypes.c_void_p()
    st = _hip.lib().imp_spmat_create(rows, cols, len(data), indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, ctypes.byref(h))
    assert st != 0 and not h.value
    _hip.check(st)


def test_failure_paths_leave_the_device_usable(gpu):
    from implicit_amd.gpu import _hip

    cut = kc.get("table_cut_k100")

    def still_exact(after):
        assert_bitwise(run(gpu, cut), want(cut.name), f"{cut.name} after {after}")

    # B with a column repeated within a row: refused, nothing written
    rep = kc.csr_from_rows([([1, 2, 1], [1.0, 2.0, 3.0]), ([0], [1.0]), ([], [])], 3)
    A = gpu.SpMat(sp.csr_matrix(np.eye(3)))
    B = gpu.SpMat(rep)
    with pytest.raises(ValueError, match="repeats a column"):
        gpu.sparse_topk_product(A, B, 2)
    ids, scores, counts = np.full((3, 2), 7, np.int32), np.full((3, 2), 7.0), np.full(3, 7, np.int32)
    st = _hip.lib().imp_sparse_topk_product(A._h, B._h, 2, 0, ids.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    assert st == _hip.IMP_INVALID_ARGUMENT
    assert np.all(ids == 7) and np.all(scores == 7.0) and np.all(counts == 7)
    still_exact("a refused B")
    # the same matrix is a valid left operand: A may repeat columns
    ok = gpu.sparse_topk_product(B, gpu.SpMat(sp.csr_matrix(np.eye(3))), 2)
    assert_bitwise(ok, kr.product_topk(rep, sp.csr_matrix(np.eye(3)), 2), "A with repeated columns")
    # malformed offsets; every array is as long as the offsets claim at most, so the check reads nothing beyond them
    for what, indptr in (("indptr[0] != 0", [1, 2, 3]), ("a decreasing indptr", [0, 2, 1, 3]), ("indptr[rows] != nnz", [0, 1, 2]),
                         ("an offset beyond nnz", [0, 5, 3, 3])):
        with pytest.raises(ValueError, match="indptr"):
            _create(gpu, len(indptr) - 1, 4, indptr, [0, 1, 2], [1.0, 2.0, 3.0])
        still_exact(what)
