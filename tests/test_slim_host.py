"""The host side of SLIM (tests/slim_reference.py): the kernel's chunked loop is the sequential rule bit for bit, the float32
rule sits where it was measured against scikit-learn's optimum, and the float64 rule pins the parameter mapping."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import slim_reference as ref
from ease_reference import gram64


LONG_SIGNED = (100, 1e-4)


def host_columns(n, positive, setting):
    """The columns of the shared cases (every one for n <= 65, 16 above), with ONE reduction, for the run time of the
    pure-Python model alone: at n = 1023, 1024 and 1025 the signed (100, 1e-4) run -- a dense support re-evaluated after each
    of its ~900 applied coordinates per sweep, seconds per column and chunk width -- checks 4 of the 16 columns: 0, 1, n - 1 and
    the one with the largest diagonal.  Every other (size, sign, setting, width) of the list runs in full."""
    A, empty, twins = ref.case(n)
    cols = ref.columns(n, A, empty, twins)
    if n >= ref.CHUNK - 1 and not positive and setting == LONG_SIGNED:
        cols = cols[:4]
    return cols


@pytest.mark.parametrize("chunk", [1, 64, 1024])
@pytest.mark.parametrize("setting", ref.SETTINGS, ids=lambda s: f"sweeps{s[0]}-tol{s[1]:g}")
@pytest.mark.parametrize("positive", [True, False], ids=["positive", "signed"])
@pytest.mark.parametrize("n", ref.SIZES)
def test_the_chunked_loop_is_the_sequential_rule(n, positive, setting, chunk):
    """63 / 64 / 65 and 1023 / 1024 / 1025 put the end of the matrix before, on and after the end of a chunk of 64 and of 1024."""
    max_sweeps, tol = setting
    A, empty, _ = ref.case(n)
    for j in host_columns(n, positive, setting):
        w, sweeps = ref.expected(n, j, ref.L1, positive, max_sweeps, tol)
        wc, sc = ref.chunked32(A, j, ref.L1, positive, max_sweeps, tol, chunk)
        assert sc == sweeps, (j, sc, sweeps)
        assert_array_equal(ref.bits(wc), ref.bits(w), err_msg=f"column {j}")
        assert w[j] == 0 and not np.signbit(w[j])
        if positive:
            assert np.all(w >= 0)
        if empty is not None:
            assert w[empty] == 0  # nobody has it: it explains nothing
            if j == empty:
                assert not w.any() and sweeps == 1


@pytest.mark.parametrize("setting", [0, 1])
@pytest.mark.parametrize("positive", [True, False])
def test_solve32_against_the_golden(setting, positive):
    g = ref.golden()
    l1, l2 = float(g["l1"][setting]), float(g["l2"][setting])
    A = gram64(g["X"], l2).astype(np.float32)
    W = np.stack([ref.solve32(A, j, l1, positive, ref.GOLDEN_MAX_SWEEPS, ref.GOLDEN_TOL)[0] for j in range(A.shape[0])], axis=1)
    distance, support = ref.column_distance(W, g["W"][setting, int(positive)])
    print(f"solve32 against scikit-learn, l1={l1} l2={l2} positive={positive}: distance {distance:.6e}, support difference {support}")
    assert distance <= 2 * ref.GOLDEN_DISTANCE[(setting, positive)]
    assert support == 0


@pytest.mark.parametrize("setting", [0, 1])
@pytest.mark.parametrize("positive", [True, False])
def test_solve64_pins_the_parameter_mapping(setting, positive):
    g = ref.golden()
    l1, l2 = float(g["l1"][setting]), float(g["l2"][setting])
    A = gram64(g["X"], l2)
    W = np.stack([ref.solve64(A, j, l1, positive, 100000, 1e-13)[0] for j in range(A.shape[0])], axis=1)
    distance, support = ref.column_distance(W, g["W"][setting, int(positive)])
    print(f"solve64 against scikit-learn: distance {distance:.3e}")
    assert distance <= 1e-9 and support == 0


def test_the_golden_input_has_its_planted_columns():
    X = ref.golden()["X"]
    assert X.shape == (60, 40) and np.all(X == np.rint(X))
    assert not X[1].any() and not X[:, 38].any() and np.array_equal(X[:, 4], X[:, 5]) and X[:, 4].any()
