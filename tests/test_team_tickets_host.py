"""The ticket bookkeeping of the chained mid-row CG launch (csrc/team_tickets.h), checked on the host through
imp_host_chain_tickets: the entry point runs the arithmetic launch_team_chain keeps per device, so no device is needed.

The device counters are never reset: a launch is told their values at its start (its bases) and the host advances them by
the number of tickets the launch draws.  That number is fixed by the protocol, which `simulate` below plays through with a
model of the kernel's row loop (team_rows, TICKETS): a wrong count would shift every later launch's tickets -- rows solved
twice or not at all."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def tickets():
    import os

    from implicit_amd import _build, utils
    from implicit_amd.gpu import _hip

    if not os.path.exists(_hip.LIB_PATH):
        _build.build(verbose=False)
    return utils.chain_tickets


def simulate(counter, base, count, teams, rng):
    """One class of one launch as the kernel runs it, the teams interleaved at random: returns the counter after the launch
    and how often each row was solved.  All counter arithmetic is modulo 2^32."""
    solved = np.zeros(count, dtype=np.int64)
    if count <= 0:
        return counter, solved  # the kernel skips an empty class
    held = [[g + k * teams for k in range(4)] for g in range(teams)]  # static tickets g, g + N, g + 2 N, g + 3 N
    active = [g for g in range(teams) if held[g][0] < count]
    while active:
        g = active[rng.integers(len(active))]
        t = held[g]
        solved[t[0]] += 1
        if t[3] < count:  # the leader draws while the team's newest ticket is inside the class
            new = min(((counter - base) & 0xFFFFFFFF) + 4 * teams, count)
            counter = (counter + 1) & 0xFFFFFFFF
        else:
            new = count
        held[g] = [t[1], t[2], t[3], new]
        if held[g][0] >= count:
            active.remove(g)
    return counter, solved


TEAMS = (1, 2, 4)  # teams of the three classes in a workgroup of 8 wavefronts


def queue_rows(n, q):
    """Members of 0 .. n - 1 that are congruent to q modulo 8: the rows of a queue, or the workgroups that serve it."""
    return len(range(q, n, 8))


def launch(tickets, state, counters, counts, workgroups, rng):
    """One launch: bases from the host bookkeeping, every queue of the three classes played on the simulated device counters.
    Returns the draws per queue."""
    before = state.copy()
    base, draws = tickets(state, counts, workgroups, TEAMS)
    assert np.array_equal(base, before)
    for c in range(3):
        for q in range(8):
            rows, teams = queue_rows(counts[c], q), queue_rows(workgroups, q) * TEAMS[c]
            counters[c][q], solved = simulate(int(counters[c][q]), int(base[c][q]), rows if teams else 0, max(teams, 1), rng)
            assert teams > 0 or rows == 0 or workgroups < 8  # a queue nobody serves needs a grid of fewer than 8 workgroups
            if teams:
                assert (solved == 1).all(), (c, q, counts[c], workgroups)
            assert (int(before[c][q]) + int(draws[c][q])) & 0xFFFFFFFF == int(state[c][q]) == counters[c][q]
    return draws


def fresh(start=0):
    return np.full((3, 8), start, np.uint32), [[start] * 8 for _ in range(3)]


def test_bases_across_many_calls(tickets):
    rng = np.random.default_rng(0)
    state, counters = fresh()
    for _ in range(40):
        workgroups = 8 * int(rng.integers(1, 5))
        counts = [int(rng.integers(0, 12 * workgroups * TEAMS[c])) for c in range(3)]
        launch(tickets, state, counters, counts, workgroups, rng)
    assert state.all()


@pytest.mark.parametrize("rows", [0, 1, 7, 8, 9, 15, 16, 23, 24, 25, 31, 32, 33, 40, 100])
def test_draws_at_every_cut(tickets, rows):
    """64 workgroups = 8 teams of width 8 per queue: no draw up to 3 N rows per queue, one past-the-end draw per team with
    g + 3 N < rows up to 4 N, then rows - 4 N + N.  The class holds 8 rows per queue row, less 3: queues 5 .. 7 are one short."""
    state, counters = fresh()
    count = max(8 * rows - 3, 0)
    draws = launch(tickets, state, counters, [count, 0, 0], 64, np.random.default_rng(rows))
    want = lambda r: 0 if r <= 24 else (r - 24 if r <= 32 else r - 32 + 8)
    assert draws[0].tolist() == [want(rows)] * 5 + [want(max(rows - 1, 0))] * 3
    assert not draws[1:].any()


def test_uneven_grid(tickets):
    """A grid that is no multiple of 8: queues 0 .. 3 have one workgroup more."""
    rng = np.random.default_rng(3)
    state, counters = fresh()
    for counts in ([500, 900, 2000], [37, 0, 5000], [4, 3, 2]):
        launch(tickets, state, counters, counts, 20, rng)


def test_32_bit_wrap(tickets):
    rng = np.random.default_rng(1)
    state, counters = fresh(0xFFFFFFF0)
    for _ in range(6):
        launch(tickets, state, counters, [700, 1300, 3000], 16, rng)
    assert (state < 0x10000).all()  # every counter wrapped


def test_empty_classes(tickets):
    rng = np.random.default_rng(2)
    state, counters = fresh(5)
    launch(tickets, state, counters, [0, 0, 0], 16, rng)
    assert (state == 5).all()  # an empty class draws nothing
    draws = launch(tickets, state, counters, [30 * 8, 0, 70 * 8], 16, rng)  # 2 / 8 teams per queue, 30 / 70 rows per queue
    assert (draws[0] == 30 - 8 + 2).all() and not draws[1].any() and (draws[2] == 70 - 32 + 8).all()
    draws = launch(tickets, state, counters, [0, 50 * 8, 0], 16, rng)
    assert not draws[0].any() and (draws[1] == 50 - 16 + 4).all() and not draws[2].any()
    assert (state == np.array([[5 + 24], [5 + 38], [5 + 46]])).all()


def test_arguments_are_checked(tickets):
    state = np.zeros((3, 8), np.uint32)
    for counts, workgroups, teams in (([-1, 0, 0], 8, TEAMS), ([0, 1 << 30, 0], 8, TEAMS), ([1, 1, 1], 0, TEAMS), ([1, 1, 1], 8, (1, 0, 4))):
        with pytest.raises(ValueError):
            tickets(state, counts, workgroups, teams)
    assert not state.any()
