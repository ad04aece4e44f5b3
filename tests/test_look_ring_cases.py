"""tests/look_ring_cases.py on the CPU: what tests/test_gpu_look_ring.py assumes of its inputs, shown with the oracle alone.

How many track entries a step consumes does not depend on the agent: the event loop of a step ends when the midprice has moved or the
session is over.  So the entries a look-ahead d steps deep needs beyond the real cursor are those the next d REAL steps consume, whatever
the look-ahead's actions (a -1 only makes it fewer).  The oracle reports its cursor in records, and an event holds at least one record:
records consumed bound the entries consumed from above, steps played bound them from below (a completed step consumes at least one).

 * Test 2 (no cell outside the window).  The deepest look-ahead is 64 steps and is always preceded by a refill (64 > LOB_TRACK_REFILL),
   after which the window ends REACH = 252 entries beyond the cursor, or the pre-pass is complete.  A shallower one runs at most 16 steps
   behind a refill.  So it suffices that no 80 consecutive steps consume more than REACH records.
 * Test 5 (the wall within the budget).  Behind the fork the window ends at most REACH entries beyond the branch's cursor and every
   completed step consumes at least one; the books must not run dry first, which holds when the oracle plays 20 + WALL_BUDGET more steps
   with every book live.
 * Test 6 (the day library).  Which day a book plays changes nothing of the argument of test 2: each day of the library, played alone,
   consumes no more than REACH records in 80 consecutive steps; the short day is shorter than the ring altogether.
 * The roll-out into the wall needs a stream whose steps are long; that a plan gets there is asserted by the GPU test itself.  Here only
   the necessary condition: the records of its 64 steps exceed what is left of the first fill.
CPU only."""
import numpy as np
import pytest

from rl_markets_amd import abi
from tests import look_ring_cases as lc
from tests import oracle_lib as ol


def play(p, rec, B, max_steps=None):
    """-> cursors [S + 1][B] (records) and terminal words [S + 1][B] of the episode under the GPU tests' step actions."""
    o = ol.Oracle(p, rec)
    o.reset()
    rng = lc.step_rng(B)
    book = o.recs()["book"]
    cur, term = [book["cursor"].copy()], [book["terminal"].copy()]
    while (term[-1] == 0).any() and (max_steps is None or len(cur) <= max_steps):
        assert len(cur) < 3000
        o.env_step(rng.integers(0, lc.N, size=B).astype(np.int32))
        book = o.recs()["book"]
        cur.append(book["cursor"].copy())
        term.append(book["terminal"].copy())
    o.close()
    return np.array(cur), np.array(term)


@pytest.mark.parametrize("B,depth,trades,normed", lc.CONFIGS)
def test_no_look_ahead_of_test_2_can_leave_the_window(B, depth, trades, normed):
    p = lc.make_params(depth, trades, normed)
    cur, term = play(p, lc.records(p, B), B)
    steps = len(cur) - 1
    assert steps >= 300, steps
    span = lc.LONG[1] + lc.REFILL
    worst = max(int((cur[min(s + span, steps)] - cur[s]).max()) for s in range(steps))
    assert worst <= lc.REACH, "%d records in %d consecutive steps: a look-ahead could reach the window's end" % (worst, span)
    assert {1, 2} <= set(int(x) for x in np.unique(term[-1])), "books that end with the session and books that run dry"
    # ... and the real step itself: no 16 steps consume the ring
    assert max(int((cur[min(s + lc.REFILL, steps)] - cur[s]).max()) for s in range(steps)) <= lc.REACH


def test_the_wall_of_test_5_is_within_the_budget():
    B, depth, trades = 70, 4, 3
    p = lc.make_params(depth, trades)
    cur, term = play(p, lc.records(p, B, mixed=False), B, max_steps=20 + lc.WALL_BUDGET)
    assert len(cur) - 1 >= 20 + lc.WALL_BUDGET and (term[-1] == 0).all(), "every book is live %d steps behind the fork" % lc.WALL_BUDGET
    assert lc.WALL_BUDGET > lc.REACH


def test_the_roll_out_into_the_wall_has_long_steps():
    B, depth, trades = 70, 10, 2
    p = lc.make_params(depth, trades)
    cur, term = play(p, lc.records(p, B, mixed=False, move_div=4), B, max_steps=15 + lc.LONG[1])
    assert len(cur) - 1 == 15 + lc.LONG[1] and (term[-1] == 0).all()
    assert cur[15].max() < lc.REACH, "the 15 real steps stay inside the first fill (the warm-up's entries are part of it)"
    assert ((cur[-1] - cur[0]) > lc.REACH).any(), "a book whose 64 further steps consume more records than the first fill holds"
    assert abi.TRACK_WINDOW_MARGIN == lc.RING - lc.REACH


def test_the_day_library_cannot_leave_the_window():
    depth, trades = 10, 2
    p = lc.make_params(depth, trades)
    span = lc.LONG[1] + lc.REFILL
    lengths = []
    for day in lc.make_days(depth, trades):
        cur, term = play(p, np.ascontiguousarray(day[None]), 1)
        steps = len(cur) - 1
        assert steps > 20 and (term[-1] == 2).all(), steps
        worst = max(int((cur[min(s + span, steps)] - cur[s]).max()) for s in range(steps))
        assert worst <= lc.REACH, "%d records in %d consecutive steps of the day of %d events" % (worst, span, day.shape[0])
        lengths.append(day.shape[0])
    assert min(lengths) < lc.RING < max(lengths), "a day inside the ring beside days that need it"
