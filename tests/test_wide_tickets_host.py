"""The ticket bookkeeping of the chained 1024-thread CG launch (csrc/team_tickets.h, WideTickets), checked on the host through
imp_host_wide_tickets: the entry point runs the arithmetic launch_wide_chain keeps per device, so no device is needed.

Class 0 is (256,512], one team of 16 wavefronts -- the workgroup -- per row; class 1 are the short rows, whose ticketed unit is
a group of 16 consecutive schedule rows.  In both a workgroup is the team.  `simulate` plays the draw protocol of the kernel's
loops (team_rows and group_rows, TICKETS) through: the draws it makes must be what the host advances the bases by, or every
later launch's tickets are shifted -- rows solved twice or not at all."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def tickets():
    import os

    from implicit_amd import _build, utils
    from implicit_amd.gpu import _hip

    if not os.path.exists(_hip.LIB_PATH):
        _build.build(verbose=False)
    return utils.wide_tickets


def simulate(counter, base, count, teams, rng):
    """One queue of one launch as the kernel runs it -- `count` units (rows or groups), `teams` workgroups interleaved at
    random: returns the counter after the launch and how often each unit was solved.  Counter arithmetic is modulo 2^32."""
    solved = np.zeros(count, dtype=np.int64)
    if count <= 0:
        return counter, solved
    held = [[g + k * teams for k in range(4)] for g in range(teams)]  # static tickets g, g + N, g + 2 N, g + 3 N
    active = [g for g in range(teams) if held[g][0] < count]
    while active:
        g = active[rng.integers(len(active))]
        t = held[g]
        solved[t[0]] += 1
        if t[3] < count:  # a draw while the newest ticket held is inside the queue
            new = min(((counter - base) & 0xFFFFFFFF) + 4 * teams, count)
            counter = (counter + 1) & 0xFFFFFFFF
        else:
            new = count
        held[g] = [t[1], t[2], t[3], new]
        if held[g][0] >= count:
            active.remove(g)
    return counter, solved


def members(n, q):
    """Members of 0 .. n - 1 congruent to q modulo 8: the units of a queue, or the workgroups that serve it."""
    return len(range(q, n, 8))


def units(rows):
    """Ticketed units per class: rows of (256,512], groups of 16 short rows (the last group may be short)."""
    return [rows[0], -(-rows[1] // 16)]


def launch(tickets, state, counters, rows, workgroups, rng):
    """One launch: bases from the host bookkeeping, every queue of both classes played on the simulated device counters.
    Returns the draws per queue."""
    before = state.copy()
    base, draws = tickets(state, rows, workgroups)
    assert np.array_equal(base, before)
    for c, n in enumerate(units(rows)):
        for q in range(8):
            count, teams = members(n, q), members(workgroups, q)
            if teams == 0:
                assert workgroups < 8 and draws[c][q] == 0  # the launcher never uses such a grid
                continue
            counters[c][q], solved = simulate(int(counters[c][q]), int(base[c][q]), count, teams, rng)
            assert (solved == 1).all(), (c, q, rows, workgroups)
            assert (int(before[c][q]) + int(draws[c][q])) & 0xFFFFFFFF == int(state[c][q]) == counters[c][q]
    return draws


def fresh(start=0):
    return np.full((2, 8), start, np.uint32), [[start] * 8 for _ in range(2)]


def test_random_pairs_across_many_calls(tickets):
    """Random (count, workgroups) pairs on one state, launch after launch."""
    rng = np.random.default_rng(0)
    state, counters = fresh()
    for _ in range(60):
        workgroups = int(rng.integers(8, 65))
        rows = [int(rng.integers(0, 8 * workgroups)), int(rng.integers(0, 16 * 8 * workgroups))]
        launch(tickets, state, counters, rows, workgroups, rng)
    assert state.all()


@pytest.mark.parametrize("workgroups", [8, 24, 256])
def test_small_counts(tickets, workgroups):
    """Fewer units than queues, fewer than workgroups, and just below / at / just above four tickets per workgroup."""
    rng = np.random.default_rng(workgroups)
    state, counters = fresh(7)
    for n in (1, 3, 7, 8, 9, workgroups - 1, workgroups + 1, 3 * workgroups, 4 * workgroups - 1, 4 * workgroups, 4 * workgroups + 1,
              4 * workgroups + 9, 5 * workgroups + 3):
        for last in (1, 15, 16):  # rows in the last group
            launch(tickets, state, counters, [n, 16 * (n - 1) + last], workgroups, rng)


@pytest.mark.parametrize("n", [0, 1, 24, 25, 32, 33, 40, 100])
def test_draws_at_every_cut(tickets, n):
    """64 workgroups = 8 per queue and n units per queue: no draw up to 3 N = 24, one past-the-end draw per workgroup with
    g + 3 N < n up to 4 N = 32, then n - 4 N + N.  The same in both classes: 8 n rows, and 8 n groups of which the last holds 1 row."""
    state, counters = fresh()
    rows = [8 * n, max(16 * 8 * n - 15, 0)]
    draws = launch(tickets, state, counters, rows, 64, np.random.default_rng(n))
    want = 0 if n <= 24 else (n - 24 if n <= 32 else n - 32 + 8)
    assert (draws == want).all()


def test_one_class_alone(tickets):
    rng = np.random.default_rng(2)
    state, counters = fresh(5)
    launch(tickets, state, counters, [0, 0], 16, rng)
    assert (state == 5).all()  # an empty class draws nothing
    draws = launch(tickets, state, counters, [30 * 8, 0], 16, rng)  # 2 workgroups and 30 rows per queue
    assert (draws[0] == 30 - 8 + 2).all() and not draws[1].any()
    draws = launch(tickets, state, counters, [0, 16 * 50 * 8], 16, rng)  # 50 groups per queue
    assert not draws[0].any() and (draws[1] == 50 - 8 + 2).all()
    assert (state == np.array([[5 + 24], [5 + 44]])).all()


def test_32_bit_wrap(tickets):
    rng = np.random.default_rng(1)
    state, counters = fresh(0xFFFFFFF0)
    for _ in range(6):
        launch(tickets, state, counters, [700, 16 * 900 + 1], 16, rng)
    assert (state < 0x10000).all()  # every counter wrapped


def test_arguments_are_checked(tickets):
    state = np.zeros((2, 8), np.uint32)
    for rows, workgroups in (([-1, 0], 8), ([0, 1 << 30], 8), ([1, 1], 0)):
        with pytest.raises(ValueError):
            tickets(state, rows, workgroups)
    assert not state.any()
