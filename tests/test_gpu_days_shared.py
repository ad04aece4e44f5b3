"""One shared weight vector on days of unequal length, against the batched oracle over days (Oracle.set_days, pinned by
tests/test_oracle_days.py): the regime the day library was built for and profiles/days_library.json measures -- a fresh day
per book and episode (src/main.cpp:51-55), recorded days that never have one length, and after the short days are over a long
tail in which a shrinking minority of the books is live.

What only this regime reaches: the shared-theta fast paths (the group-0 memo and hit-list replay of env_step_kernel /
env_step16_kernel, learn_q_pair_kernel / learn_q_lane_kernel, trace_lane_kernel, trace_rest_kernel, apply_kernel) while every
book has its own rec_len[b] (DevState::events_of); the hand-back count, the dense-sum / block-sum switch and the ring refill
(maybe_refill_track / prepass_extend_kernel) while the live count falls and books run dry at different steps of one batch;
finalize_kernel rolling the ending episode back on its days before the day sets swap, where one book's damage would reach
every book through the weights; and the small-batch general kernels (env_kernel, act_kernel, learn_kernel, update_kernel)
on unequal days.  The yardstick is always the oracle, never a second engine."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import days_ref
from tests import oracle_lib as ol
from tests.parity import compare_env, compare_learner_step
from tests.test_gpu_days import make_days
from tests.test_gpu_episode_stats import check_record
from tests.test_gpu_fuzz import random_case
from tests.test_gpu_steady import light_books
from tests.test_gpu_step_log import Expect, assert_log_equals, oracle_books
from tests.test_gpu_training_schedule import (SWITCH, assert_hints_arrived, compare_theta, eps_after, flow_delta, set_epsilon,
                                              td_steps)

pytestmark = pytest.mark.gpu

# The library: 6 days of 6 lengths, the longest three times the shortest and longer than the 256-entry track ring the tests
# set.  A day of n events is ~(n - 45) / 1.8 learner steps: the five short days end after 30-50 steps, the long one after ~140,
# so about two thirds of every episode is a tail in which the sixth of the books that drew the long day is live.  Three
# episodes are ~5.5 M oracle book-steps per algorithm (and as many of the shadow oracle's): the existing schedule test's
# 4 M + 4 M, a little more for the tail.
LENGTHS = [100, 108, 116, 124, 132, 300]
RING = 256


def finish_steps(p, days):
    """Per day, the 0-based learner step at which a book playing it is found over (out of data, or the close): a function of
    the stream alone (a step ends when the mid-price has moved -- Base::performAction, base.cpp:285-305 -- whatever the agent
    does), taken from a one-book oracle."""
    q = copy.copy(p)
    q.memory_size, q.theta_mode = 4099, abi.THETA_PRIVATE
    out = []
    for d in days:
        o = ol.Oracle(q, np.asarray(d)[None])
        o.reset()
        n = 0
        while True:
            o.td_step(1)
            if o.counters()[2] == 0:
                break
            n += 1
            assert n < len(d)
        o.close()
        out.append(n)
    return np.array(out)


def schedule_params(algo):
    p = engine.default_params()
    p.depth, p.max_trades = 10, 2
    p.algo, p.theta_mode, p.memory_size = algo, abi.THETA_SHARED, 20000000
    p.epsilon = eps_after(0)
    return p


def random_draws(p, B, n_days, episodes):
    """RandomSampler's draws 2 .. episodes + 1 of every book (tests/days_ref.py).  The first draw of consecutive seeds is one or
    two neighbouring days for every book (minstd_rand0's first value is 16807 x seed): the tests draw it and replace it before
    the first reset, as tests/test_gpu_days.py does."""
    return np.array([days_ref.book_days(p.seed, b, n_days, episodes + 1) for b in range(B)])[:, 1:]


def run_schedule(algo, B, episodes, every_step, observers=False):
    """The reference's training loop on library days of unequal length -- lob_days_select(RANDOM) + lob_reset, steps until no
    book is live, ClearInventory, HandleTerminal, the next epsilon of test_gpu_training_schedule.py's schedule -- against the
    batched oracle (and a shadow oracle whose weights are nudged by 1e-13 after step 3, for compare_theta's floor)."""
    days = make_days(LENGTHS, depth=10)
    lib = ol.DayLibrary(days)
    n_days = len(days)
    lengths = np.array(LENGTHS)
    assert n_days >= 5 and len(set(LENGTHS)) >= 4 and lengths.max() >= 3 * lengths.min() and lengths.max() > RING
    p = schedule_params(algo)
    fin = finish_steps(p, days)
    draws = random_draws(p, B, n_days, episodes)
    eng = engine.Engine(p, B)
    eng.load_days(days)
    np.testing.assert_array_equal(eng.day_first[:-1], lib.day_first)
    eng.days_select(abi.DAYS_RANDOM, 0, n_days)          # (the correlated first draw, replaced below before any reset)
    orc = ol.Oracle(p, np.stack([days[0]] * B))          # (this buffer is never played: every episode's days come by set_days)
    shadow = ol.Oracle(p, orc.records)
    eps = [eps_after(k) for k in range(3)]
    assert eps[0] > SWITCH > eps[1] > eps[2], eps
    sel = None
    if observers:
        # 64 books, ~11 of each day of the first episode
        sel = np.sort(np.concatenate([np.flatnonzero(draws[:, 0] == d)[:11] for d in range(n_days)])[:64]).astype(np.int32)
        assert len(sel) == 64
        eng.step_log_enable(sel, 512)
    problems = []
    for ep in range(episodes):
        tag = "days, shared theta: algo %d, %d books, episode %d (eps %.4g)" % (algo, B, ep, eps[ep])
        eng.days_select(abi.DAYS_RANDOM, 0, n_days)
        eng.reset()
        d = eng.days()
        np.testing.assert_array_equal(d, draws[:, ep], err_msg=tag + " days drawn")
        assert len(np.unique(d)) == n_days
        assert (lengths[draws[:, ep]] != lengths[draws[:, ep - 1]]).mean() > 0.5 if ep else True
        for o in (orc, shadow):
            o.set_days(*lib.of(d))
            o.reset()
        if observers:
            assert len(np.unique(d[sel])) == n_days, "the logged books are spread over all days"
            ex = Expect(oracle_books(orc, sel))
        # when the books of each day finish, and with that the live count of every step: from the one-book oracles, and held
        # against the batched oracle's own count below
        per_day = np.bincount(d, minlength=n_days)
        T = int(fin.max()) + 1
        live = [int(per_day[fin > s].sum()) for s in range(T)]
        near_an_end = {int(f) + k for f in set(fin) for k in range(-2, 3)}
        flow0, light0 = eng.flow_stats(), light_books(eng)
        compared = 0
        for step in range(T):
            td_steps(eng, orc, shadow)
            if ep == 0 and step == 3:
                th = shadow.theta()
                th[th != 0] *= 1.0 + 1e-13
            n_live, o_live = int(eng.counters()[2]), int(orc.counters()[2])
            assert o_live == live[step], (tag, step, o_live, live[step])
            assert n_live == o_live, (tag, step, n_live, o_live)
            if every_step or step < 4 or step % 8 == 7 or step in near_an_end or step >= T - 10:
                compare_learner_step(eng, orc, "%s step %d of %d (%d live)" % (tag, step, T, n_live), exact=False, rtol=1e-9)
                compared += 1
            if observers:
                ex.after_step(oracle_books(orc, sel))
        assert eng.counters()[2] == 0 and orc.counters()[2] == 0
        # the tail is really run: from the oracle's counts alone
        tail = sum(1 for n in live if 0 < n < B / 4)
        assert 4 * tail >= T, (tag, tail, T)
        books = orc.recs()["book"]
        assert (books["terminal"] == 2).all() and (books["cursor"][lengths[d] == lengths.max()] > RING).all(), \
            tag + ": every day runs out of data, the long day past the ring"
        flow = flow_delta(eng.flow_stats(), flow0)
        served = light_books(eng) - light0
        hs = assert_hints_arrived(eng, tag)
        print("%s: %d steps (%d compared in full), tail %d steps = %.0f%% (live %s), flow %s, hit-list books %d of %d live book-steps, "
              "hints %s" % (tag, T, compared, tail, 100.0 * tail / T, sorted(set(live), reverse=True), flow, served, sum(live), hs))
        # test_training_schedule_on_library_days's rule per algorithm and epsilon, over the tail as well
        if algo == abi.ALGO_SARSA or (algo == abi.ALGO_QLAMBDA and eps[ep] < SWITCH):
            if not (flow["dense_sums"] == T and flow["block_sums"] == T and flow["added_in_place"] == 0):
                problems.append((tag, "dense sums in every step", T, flow))
        else:
            # (the first step of an episode acts without hit lists: act_fast_kernel, not the fused flow)
            if not (flow["added_in_place"] >= T - 1 and flow["dense_sums"] == 0 and flow["block_sums"] == 0):
                problems.append((tag, "added in place in every step", T, flow))
        if flow["every_book"] != 0 or served <= 0:
            problems.append((tag, "every_book / served", flow, served))
        drift = compare_theta(eng, orc, algo, tag, 20000 if B >= 32768 else 5000, shadow)
        print("%s: shadow drift %s" % (tag, drift))
        if observers:
            # lob_episode_stats(by_day) against test_gpu_episode_stats.py's host reduction of the ORACLE's dumps
            st = eng.episode_stats(True)
            ids = int(p.book_id_offset) + np.arange(B, dtype=np.int64)
            assert len(st) == 1 + n_days
            check_record(st[0], books, ids, -1, tag + " stats, whole")
            for day in range(n_days):
                m = d == day
                check_record(st[1 + day], books[m], ids[m], day, "%s stats, day %d" % (tag, day))
            # ... and the step log of the 64 books against the rows the oracle's dumps give
            n_rows = assert_log_equals(eng, sel, ex.rows, tag + " step log")
            assert n_rows.min() > 20 and n_rows.max() > 100, (tag, n_rows.min(), n_rows.max())
        eng.clear_inventory(); orc.clear_inventory(); shadow.clear_inventory()
        compare_learner_step(eng, orc, tag + " after ClearInventory", exact=False, rtol=1e-9)
        eng.handle_terminal(); orc.handle_terminal(); shadow.handle_terminal()
        if ep + 1 < episodes:
            set_epsilon(eng, orc, eps[ep + 1])
            ol.load().oracle_set_epsilon(shadow.h, C.c_double(eps[ep + 1]))
    assert eng.hint_stats()["hint_read"] > 0
    assert not problems, problems
    eng.close()
    orc.close()
    shadow.close()


# ---- a. the training schedule on unequal days, at scale ---------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q, abi.ALGO_SARSA], ids=["qlambda", "double_q", "sarsa"])
def test_training_schedule_on_unequal_days(monkeypatch, algo):
    """32 768 books (the lane-per-book kernels with no switch set), D = 10, two trade slots, M = 20 M, one weight vector, six
    days of 100-300 events in a 256-entry track ring (ring mode for every book; the 300-event day wraps it), three episodes
    across the 0.34 switch.  Every step: the live count.  In full: steps 0-3, every 8th step, every step within +-2 of the
    step at which the books of a day finish, the last 10 steps, after ClearInventory; theta (and theta_b) at the end of
    every episode, to 100 x the shadow oracle's drift."""
    monkeypatch.setenv("LOB_TRACK_RING", str(RING))
    run_schedule(algo, 32768, 3, every_step=False)


# ---- b. the 16-lanes-per-book dispatch, d. the observers on the same run -------------------------------------------------------------

def test_sixteen_lanes_per_book_on_unequal_days_with_observers(monkeypatch):
    """4 096 books, SARSA(lambda): env_step16_kernel with no switch set.  The same loop, two episodes, EVERY step compared,
    the ring held at 256.  At the end of each episode lob_episode_stats(by_day=True) against the host reduction of the oracle's
    book dumps, and the step log of 64 books spread over all days against the rows the oracle's dumps give."""
    monkeypatch.setenv("LOB_TRACK_RING", str(RING))
    run_schedule(abi.ALGO_SARSA, 4096, 2, every_step=True, observers=True)


# ---- c. randomised sweep on small batches ---------------------------------------------------------------------------------------------

N_SEEDS = int(os.environ.get("LOB_FUZZ_SEEDS", "32"))
# The ring of the sweep is refilled every 16 steps, as in the other tests of a 256-entry ring (test_gpu_parity.py,
# test_gpu_replay.py): a refill leaves a book 252 events ahead, and random_case's streams can spend those in fewer than the
# default 64 steps (seed 11: a book at record 253 after 41 steps), which the engine reports as a ring underrun and voids the
# run.  In 16 steps the default seeds' books move 162 records at most.
REFILL = 16
MIXED = {}     # seed -> (B, two books of different day length were live at step 30 of an episode)


def days_case(seed):
    """-> (p, B, days, assignment per episode [2][B], ring or None): test_gpu_fuzz.random_case's parameters and stream statistics
    (seed 9000 + seed), B from {1, 3, 8, 64}, a library of 2-5 days of distinct lengths in 150-600, a random lob_days_set
    assignment per episode that uses both the shortest and the longest day (one book: the shortest, then the longest), and for
    half of the seeds a 256-entry track ring (refilled every REFILL steps)."""
    p, g, _ = random_case(9000 + seed)
    r = np.random.default_rng(19000 + seed)
    B = int(r.choice([1, 3, 8, 64]))
    n_days = int(r.integers(2, 6))
    lengths = [int(n) for n in r.choice(np.arange(150, 601), size=n_days, replace=False)]
    days = []
    for i, n in enumerate(lengths):
        g.n_events = n
        days.append(engine.gen_stream_host(g, p.depth, p.max_trades, p.book_id_offset + 500 + i, 1)[0])
    lo, hi = int(np.argmin(lengths)), int(np.argmax(lengths))
    assign = r.integers(0, n_days, size=(2, B)).astype(np.int32)
    for ep in range(2):
        if B == 1:
            assign[ep, 0] = (lo, hi)[ep]
        else:
            where = r.choice(B, size=2, replace=False)
            assign[ep, where[0]], assign[ep, where[1]] = lo, hi
    return p, B, days, assign, (RING if seed % 2 else None)


def mixed_at_30(recs, day_len_of_book):
    live = recs["book"]["terminal"] == 0
    return len(set(np.asarray(day_len_of_book)[live])) >= 2


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_configuration_on_unequal_days(monkeypatch, seed):
    """Two episodes of 70 steps (or to the end, if that comes sooner), every step compared: exact with private theta or one
    book, rtol 1e-9 otherwise, as test_gpu_fuzz.py::test_random_configuration."""
    p, B, days, assign, ring = days_case(seed)
    if ring:
        monkeypatch.setenv("LOB_TRACK_RING", str(ring))
        monkeypatch.setenv("LOB_TRACK_REFILL", str(REFILL))
    lib = ol.DayLibrary(days)
    eng = engine.Engine(p, B)
    eng.load_days(days)
    orc = ol.Oracle(p, np.stack([days[0]] * B))
    exact = p.theta_mode == abi.THETA_PRIVATE or B == 1
    mixed = False
    for episode in range(2):
        eng.days_set(assign[episode])
        eng.reset()
        np.testing.assert_array_equal(eng.days(), assign[episode])
        orc.set_days(*lib.of(assign[episode]))
        orc.reset()
        tag = "days seed %d (B %d, days of %s events, ring %s) episode %d" % (seed, B, list(lib.day_len), ring, episode)
        compare_learner_step(eng, orc, tag + " reset", exact=exact, rtol=1e-9)
        at_refill = orc.recs()["book"]["cursor"] * 0
        for step in range(70):
            eng.td_step(1)
            orc.td_step(1)
            if ring:
                # (from the oracle alone: the case stays inside what the ring holds between two refills)
                cursor = orc.recs()["book"]["cursor"]
                assert (cursor - at_refill < ring - 8).all(), "%s step %d: a %d-entry ring refilled every %d steps is too small " \
                    "for this stream" % (tag, step, ring, REFILL)
                if step % REFILL == REFILL - 1:
                    at_refill = cursor
            compare_learner_step(eng, orc, "%s step %d" % (tag, step), exact=exact, rtol=1e-9)
            n_live = int(eng.counters()[2])
            assert n_live == int(orc.counters()[2]), (tag, step)
            if step == 30:
                mixed = mixed or mixed_at_30(orc.recs(), lib.day_len[assign[episode]])
            if n_live == 0:
                break
        eng.clear_inventory(); orc.clear_inventory()
        compare_env(eng, orc, tag + " after ClearInventory")      # (the books alone: an episode cut at 70 steps has books that stepped)
        eng.handle_terminal(); orc.handle_terminal()
    for which in range(B if p.theta_mode == abi.THETA_PRIVATE else 1):
        a, b = eng.theta(which), orc.theta(which)
        if exact:
            np.testing.assert_array_equal(a, b)
        else:
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
    MIXED[seed] = (B, mixed)
    eng.close()
    orc.close()


def test_zz_the_sweep_had_books_of_different_day_length_live():
    """Over the sweep above: in at least three quarters of the cases with B >= 3, two books playing days of different length
    were live at step 30 of an episode -- the sweep is about unequal days, not about one survivor."""
    if len(MIXED) < N_SEEDS:
        return      # (only part of the sweep ran in this process)
    big = [m for B, m in MIXED.values() if B >= 3]
    print("unequal-days sweep: %d cases, %d with B >= 3, %d of them with days of different length live at step 30" % (len(MIXED), len(big), sum(big)))
    assert big and 4 * sum(big) >= 3 * len(big), (sum(big), len(big))
