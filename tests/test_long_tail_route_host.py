"""Who runs the tail of the long-row path of a CG half sweep (csrc/long_tail_route.h), checked on the host through
imp_host_long_tail_route: the entry point runs the function the class dispatch calls (run_classes_q, csrc/als_cg_q.hip), so no
device is needed.

The tail has two parts: the FINISH of the long rows cut into more than one segment, and the fp32 FIX-UP of the rows a
normal-matrix solve listed.  Restated here from what each part needs:
  * a part that does not exist is run by nobody (no multi-segment row; a fix list of capacity 0 = no normal-matrix launch);
  * a part rides a chained launch only on the chained route and only where that chain has rows of its own -- a chain without
    rows is not launched: the finish rides the chain of (128,256], (64,128], (32,64], the fix-up the chain of (256,512] and the
    short rows, which is the last launch of the half sweep;
  * a stand-alone fix-up is queued behind the last launch that can list a row: behind the team chain where that carries the
    finish items, ahead of the classes otherwise."""
import itertools
import os

import pytest

NO, ALONE, TEAM_CHAIN = 0, 1, 2
NO_FIXUP, AHEAD_OF_CLASSES, BEHIND_TEAM_CHAIN, WIDE_CHAIN = 0, 1, 2, 3


@pytest.fixture(scope="module")
def route():
    from implicit_amd import _build, utils
    from implicit_amd.gpu import _hip

    if not os.path.exists(_hip.LIB_PATH):
        _build.build(verbose=False)
    return utils.long_tail_route


def restated(chain, wide, n_multi, capacity, chained):
    team_launch, wide_launch = chained and any(chain), chained and any(wide)
    finish = NO if n_multi == 0 else (TEAM_CHAIN if team_launch else ALONE)
    if capacity == 0:
        fixup = NO_FIXUP
    elif wide_launch:
        fixup = WIDE_CHAIN
    else:
        fixup = BEHIND_TEAM_CHAIN if finish == TEAM_CHAIN else AHEAD_OF_CLASSES
    return finish, fixup


def test_every_combination_of_zero_and_nonzero_counts(route):
    seen = set()
    for bits in itertools.product([0, 1], repeat=8):
        chain = [7 * bits[0], 300 * bits[1], 1 * bits[2]]
        wide = [5 * bits[3], 40000 * bits[4]]
        capacity = 9 * bits[6]
        n_multi = 4 * bits[5] * bits[6]  # rows of more than one segment are long rows
        chained = bool(bits[7])
        got = route(chain, wide, n_multi, capacity, chained)
        assert got == restated(chain, wide, n_multi, capacity, chained), (chain, wide, n_multi, capacity, chained)
        seen.add(got)
    assert seen == {(NO, NO_FIXUP), (NO, AHEAD_OF_CLASSES), (NO, WIDE_CHAIN), (ALONE, AHEAD_OF_CLASSES), (ALONE, WIDE_CHAIN),
                    (TEAM_CHAIN, BEHIND_TEAM_CHAIN), (TEAM_CHAIN, WIDE_CHAIN)}


def test_the_named_routes(route):
    # the flagship shape: everything present, both parts folded
    assert route([1000, 5000, 20000], [300, 100000], 272, 1500, True) == (TEAM_CHAIN, WIDE_CHAIN)
    # team chain not launched: stand-alone reduce + finish, the fix-up still rides the wide chain
    assert route([0, 0, 0], [300, 100000], 272, 1500, True) == (ALONE, WIDE_CHAIN)
    # wide chain not launched: the stand-alone fix-up follows the team chain
    assert route([0, 0, 1], [0, 0], 272, 1500, True) == (TEAM_CHAIN, BEHIND_TEAM_CHAIN)
    # neither launched, and every non-chained route (f = 64, float16 storage, a per-kernel profiler pass): the old order
    assert route([0, 0, 0], [0, 0], 272, 1500, True) == (ALONE, AHEAD_OF_CLASSES)
    assert route([1000, 5000, 20000], [300, 100000], 272, 1500, False) == (ALONE, AHEAD_OF_CLASSES)
    # whole long rows only: nothing to finish, the list can still fill
    assert route([1000, 5000, 20000], [300, 100000], 0, 1500, True) == (NO, WIDE_CHAIN)
    # no long rows at all
    assert route([1000, 5000, 20000], [300, 100000], 0, 0, True) == (NO, NO_FIXUP)


def test_arguments_are_checked(route):
    for chain, wide, n_multi, capacity in (([-1, 0, 0], [0, 0], 0, 0), ([0, 0, 0], [0, -5], 0, 0), ([0, 0, 0], [0, 0], -1, 0),
                                           ([0, 0, 0], [0, 0], 3, 2), ([0, 0, 0], [0, 0], 0, -1)):
        with pytest.raises(ValueError):
            route(chain, wide, n_multi, capacity, True)
