"""CPU proof that the restatements and problems of tests/subspace_cases.py are what the GPU tests (tests/test_gpu_subspace.py)
take them for: sweep_f64 is the contract (it is the exact solve at k >= f and a descent method below), sweep_f32 is a float32
run of the same steps whose sums really are left to right and whose distance from sweep_f64 is the non-zero yardstick, and the
problems are positive definite exactly where they claim to be."""
import numpy as np
import pytest

import cholesky_cases as cc
import subspace_cases as sc


def test_the_ordered_sum_is_a_left_to_right_loop():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal((3001, 5)) * 10.0 ** rng.integers(-3, 4, size=(3001, 5))).astype(np.float32)
    acc = np.zeros(5, np.float32)
    for row in a:
        acc = acc + row
    assert sc._ordered_sum(a).dtype == np.float32 and sc._ordered_sum(a).tobytes() == acc.tobytes()
    assert sc._ordered_sum(a).tobytes() != a.sum(axis=0, dtype=np.float64).astype(np.float32).tobytes()  # the order shows
    one = np.abs(a[:, :1]) + np.float32(1)  # a single column of positive terms: pairwise summation would be closer to the truth
    acc = np.zeros(1, np.float32)
    for row in one:
        acc = acc + row
    assert sc._ordered_sum(one).tobytes() == acc.tobytes() and sc._ordered_sum(one[:, :, None]).tobytes() == acc.tobytes()
    assert one.sum(axis=0).tobytes() != acc.tobytes()
    u, y = a[:700, :3], a[:700, 1:5]
    gram = np.zeros((3, 4), np.float32)
    for ui, yi in zip(u, y):
        gram = gram + ui[:, None] * yi[None, :]
    assert sc._ordered_gram(u, y, chunk=64).tobytes() == gram.tobytes()


def test_the_batched_newton_step_solves_and_flags():
    rng = np.random.default_rng(1)
    M = rng.standard_normal((4, 6, 6))
    H = M @ M.transpose(0, 2, 1) + 0.1 * np.eye(6)
    H[2, 3, 3] = -1.0
    g = rng.standard_normal((4, 6))
    delta, bad = sc._newton(H, g)
    assert bad.tolist() == [False, False, True, False]
    for i in (0, 1, 3):
        np.testing.assert_allclose(delta[i], -np.linalg.solve(H[i], g[i]), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("f,k", [(8, 8), (20, 32), (32, 32), (64, 64)])
def test_a_sweep_of_one_block_is_the_cholesky_half_sweep(f, k):
    p = sc.routes_problem(f)
    want, failing = cc.solve_f64(p.C, p.Y, p.gram, p.reg)
    assert failing == []
    for X0 in (p.X0, np.zeros_like(p.X0), p.X0[::-1] * 50):
        (got,), bad = sc.sweep_f64(p.C, X0, p.Y, p.gram, p.reg, k)
        assert bad == []
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert sc.distance(got, want) <= 1e-12


@pytest.mark.parametrize("f,k", [(20, 8), (64, 16), (130, 32)])
def test_the_energy_of_every_row_never_increases(f, k):
    p = sc.routes_problem(f)
    xs, bad = sc.sweep_f64(p.C, p.X0, p.Y, p.gram, p.reg, k, sweeps=8)
    assert bad == []
    before = sc.row_energy(p.C, p.X0.astype(np.float64), p.Y, p.gram, p.reg)
    for X in xs:
        after = sc.row_energy(p.C, X, p.Y, p.gram, p.reg)
        for u in after:
            assert after[u] <= before[u] + 1e-12 * max(1.0, abs(before[u])), (u, before[u], after[u])
        before = after
    exact, _ = cc.solve_f64(p.C, p.Y, p.gram, p.reg)
    assert sc.distance(xs[-1], exact) < sc.distance(xs[0], exact)


@pytest.mark.parametrize("f,k", sc.GRID)
def test_the_yardstick_is_not_zero(f, k):
    x64, x32, bad = sc.reference("routes", f, k, max(sc.SWEEPS))
    assert bad == []
    for s in sc.SWEEPS:
        d = sc.distance(x32[s - 1], x64[s - 1])
        print(f"f={f} k={k} sweeps={s}: d_f32 = {d:.3e}")
        assert 1e-8 < d < 1e-5
        assert x32[s - 1].dtype == np.float32
    lens = np.diff(sc.routes_problem(f).C.indptr)
    assert not x64[0][lens == 0].any() and not x32[0][lens == 0].any()  # empty rows


def test_the_routes_problem_is_what_it_says():
    p = sc.routes_problem(32)
    lens = np.diff(p.C.indptr).tolist()
    assert lens == sc.LENGTHS and p.C.shape == (len(sc.LENGTHS), sc.COLS) and p.X0.shape[0] == len(lens) + sc.EXTRA_ROWS
    for n in (sc.WAVE_CUT - 1, sc.WAVE_CUT, sc.WAVE_CUT + 1, 2 * sc.SEGMENT - 1, 2 * sc.SEGMENT, 2 * sc.SEGMENT + 1, 5000, 0):
        assert n in lens
    c = p.C.data
    assert 1.0 <= np.abs(c).min() and np.abs(c).max() <= 40.0
    assert 0.05 < (c < 0).mean() < 0.15 and 10 < (c == 1.0).sum() < 0.05 * len(c)
    assert np.abs(p.Y).max() <= 0.15 and 0 <= p.X0.min() and p.X0.max() < 0.01 and p.reg == 0.01
    for u in range(p.C.shape[0]):
        ids = p.C.indices[p.C.indptr[u]:p.C.indptr[u + 1]]
        assert (np.diff(ids) > 0).all()


@pytest.mark.parametrize("failing", sc.FAILING_SETS)
def test_the_failing_rows_fail_in_their_first_block_and_only_they(failing):
    for f, k in ((64, 16), (20, 8), (32, 32)):
        p = sc.failing_problem(f, tuple(failing))
        assert np.array_equal(p.gram, np.eye(f)) and p.reg == 0.0
        spectra = sc.block_spectra(p.C, p.Y, p.gram, p.reg, k)
        for u, mins in spectra.items():
            if u in failing:
                assert mins[0] < 0 and abs(mins[0] - (1 - 0.75 * 9)) < 1.0, (u, mins)
                assert all(m > 0 for m in mins[1:])
            else:
                assert min(mins) > 0.5, (u, mins)
        _, bad = sc.sweep_f64(p.C, p.X0, p.Y, p.gram, p.reg, k)
        assert bad == sorted(failing)
        _, bad32 = sc.sweep_f32(p.C, p.X0, p.Y, p.gram, p.reg, k)
        assert bad32 == sorted(failing)


@pytest.mark.parametrize("f,k", sc.GRID)
def test_every_block_of_the_routes_problem_is_positive_definite(f, k):
    p = sc.routes_problem(f)
    spectra = sc.block_spectra(p.C, p.Y, p.gram, p.reg, k)
    assert len(spectra) == sum(1 for n in sc.LENGTHS if n)
    assert min(min(m) for m in spectra.values()) > 0
