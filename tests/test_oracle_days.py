"""oracle_set_days (oracle/lob_oracle.h): a day per book and episode in the batched oracle -- the yardstick of
tests/test_gpu_days_shared.py -- pinned on the CPU:

  a. a batched oracle over unequal days is B one-book oracles, record for record (private theta);
  b. a one-book oracle driven by set_days is the UNMODIFIED reference loading another day before every episode
     (src/main.cpp:53-55; oracle/ref_harness `episode` mode with a stream per episode), on random configurations;
  c. the positive twin of tests/test_days_abi.py::test_dry_padding_is_not_the_same_day: the day itself, handed over with its
     true length, plays exactly like oracle_create on that day -- out of the very buffer that holds the padding."""
import os
import tempfile

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import oracle_lib as ol
from tests.test_gpu_fuzz import random_case
from tests.test_gpu_step_log import day_into_the_close
from tests.test_oracle_golden import replay_multi
from tests.test_oracle_ref_sweep import ALGOS, REWARD_OF, VAR_OF, check_sparse, f32, sparse

DEPTH, TRADES = 5, 2


def make_days(lengths, first_id=3000, gen=None, depth=DEPTH, trades=TRADES):
    """Synthetic days of the given lengths, each its own generator book id (different content)."""
    out = []
    for i, n in enumerate(lengths):
        g = gen or engine.default_gen_params()
        g.n_events = int(n)
        out.append(engine.gen_stream_host(g, depth, trades, first_id + i, 1)[0])
    return out


def params(algo, first_book=0, theta_mode=abi.THETA_PRIVATE, mem=1 << 16):
    p = engine.default_params()
    p.depth, p.max_trades = DEPTH, TRADES
    p.algo, p.theta_mode, p.memory_size = algo, theta_mode, mem
    p.book_id_offset = first_book
    return p


# ---- a. batched equals single ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", range(6), ids=[a[0] for a in ALGOS])
def test_batched_over_days_equals_one_book_oracles(algo):
    """B = 7 books, private theta, 5 days of 5 lengths, three episodes; every book changes to a day of another length at
    every episode boundary.  The batched oracle gets every episode's days through set_days (its oracle_create buffer is
    never played); each one-book oracle is oracle_create on its first day, then set_days.  Every field of every book's
    oracle_step_rec byte for byte after the reset, every step until no book is live, and after ClearInventory; the weights
    at the end."""
    B, episodes = 7, 3
    lengths = [150, 230, 310, 420, 560]
    days = make_days(lengths)
    lib = ol.DayLibrary(days)
    np.testing.assert_array_equal(lib.day_len, lengths)
    assign = np.array([[(b + 2 * ep) % 5 for ep in range(episodes)] for b in range(B)])
    assert (np.diff(np.array(lengths)[assign], axis=1) != 0).all(), "every book changes length at every boundary"
    batch = ol.Oracle(params(algo), np.stack([days[0]] * B))
    ones = [ol.Oracle(params(algo, first_book=b), days[assign[b, 0]][None]) for b in range(B)]
    for ep in range(episodes):
        batch.set_days(*lib.of(assign[:, ep]))
        if ep:
            for b, o in enumerate(ones):
                o.set_days(*lib.of(assign[b:b + 1, ep]))
        batch.reset()
        for o in ones:
            o.reset()
        steps = 0
        while True:
            got = batch.recs()
            for b, o in enumerate(ones):
                assert got[b].tobytes() == o.rec(0).tobytes(), "algo %d episode %d step %d book %d" % (algo, ep, steps, b)
            live = int(batch.counters()[2])
            assert live == sum(int(o.counters()[2]) for o in ones)
            if steps and live == 0:
                break
            batch.td_step(1)
            for o in ones:
                o.td_step(1)
            steps += 1
            assert steps < 700
        assert steps > 40, steps
        assert (got["book"]["terminal"] == 2).all(), "synthetic days end mid-session: every book runs out of data"
        ticks = got["book"]["total_ticks"]
        assert len(set(ticks[np.array(lengths)[assign[:, ep]] == n].max() for n in set(np.array(lengths)[assign[:, ep]]))) > 1, \
            "days of different length end at different steps"
        batch.clear_inventory(); batch.handle_terminal()
        for o in ones:
            o.clear_inventory(); o.handle_terminal()
        got = batch.recs()
        for b, o in enumerate(ones):
            assert got[b].tobytes() == o.rec(0).tobytes(), "algo %d episode %d after ClearInventory, book %d" % (algo, ep, b)
    double = algo in (abi.ALGO_DOUBLE_Q, abi.ALGO_DOUBLE_R_LEARN)
    for b, o in enumerate(ones):
        assert np.count_nonzero(o.theta(0)) > 100
        np.testing.assert_array_equal(batch.theta(b), o.theta(0), err_msg="theta of book %d" % b)
        if double:
            np.testing.assert_array_equal(batch.theta_b(b), o.theta_b(0), err_msg="theta_b of book %d" % b)
    batch.close()
    for o in ones:
        o.close()


def test_set_days_waits_for_the_reset_and_leaves_the_learner_alone():
    """set_days in the middle of an episode changes nothing until the next reset; the reset then changes the day and nothing
    of the learner: weights, trace count, RNG counter."""
    days = make_days([200, 330])
    lib = ol.DayLibrary(days)
    p = params(abi.ALGO_QLAMBDA)
    a, b = ol.Oracle(p, days[0][None]), ol.Oracle(p, days[0][None])
    a.reset(); b.reset()
    a.td_step(20); b.td_step(20)
    a.set_days(*lib.of([1]))
    for s in range(20):
        a.td_step(1); b.td_step(1)
        assert a.rec(0).tobytes() == b.rec(0).tobytes(), s
    th, ctr = a.theta(0).copy(), int(a.rec(0)["rng_ctr"])
    a.reset()
    np.testing.assert_array_equal(a.theta(0), th)
    assert int(a.rec(0)["rng_ctr"]) == ctr and np.count_nonzero(th) > 0
    assert a.rec(0)["book"]["time_ms"] != b.rec(0)["book"]["time_ms"] or a.rec(0)["book"]["cursor"] != b.rec(0)["book"]["cursor"]
    a.td_step(400)
    assert a.rec(0)["book"]["cursor"] > 200, "the second day is the longer one"
    # refused: a day of one event, a negative offset
    lib1 = ol.load()
    one, neg, first0 = np.array([1], np.int32), np.array([-1], np.int64), np.array([0], np.int64)
    assert lib1.oracle_set_days(a.h, ol.ptr(lib.records), ol.ptr(first0), ol.ptr(one)) == -1
    assert lib1.oracle_set_days(a.h, ol.ptr(lib.records), ol.ptr(neg), ol.ptr(np.array([50], np.int32))) == -1


# ---- c. the positive twin of test_dry_padding_is_not_the_same_day ------------------------------------------------------------------

def test_the_unpadded_day_through_set_days_is_the_same_day():
    """tests/test_days_abi.py::test_dry_padding_is_not_the_same_day pads a 300-event day to 600 rows and shows the oracle parts
    from the day itself where the data runs out.  Out of the same padded buffer, set_days with the day's TRUE length plays
    exactly like oracle_create on the day: every record byte for byte until the data has run out, and the weights."""
    p = engine.default_params()
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_PRIVATE, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 300
    day = engine.gen_stream_host(g, 5, 2, 0, 1)
    pad = np.concatenate([day[0], np.repeat(day[0, -1:], 300, axis=0)]).copy()
    pad[300:, 1] |= abi.EVT_FLAG_TAS_DRY
    o1, o2 = ol.Oracle(p, day), ol.Oracle(p, pad[None])
    o2.set_days(pad, [0], [300])
    o1.reset()
    o2.reset()
    assert o1.rec(0).tobytes() == o2.rec(0).tobytes()
    for s in range(400):
        o1.td_step(1)
        o2.td_step(1)
        assert o1.rec(0).tobytes() == o2.rec(0).tobytes(), "step %d" % s
    assert o1.rec(0)["book"]["terminal"] == 2 and o1.counters()[0] > 50
    np.testing.assert_array_equal(o1.theta(0), o2.theta(0))


# ---- b. against the unmodified reference --------------------------------------------------------------------------------------------

def harness_args(p):
    """tests/test_gpu_fuzz.py::random_case's parameters as the reference sees them: the harness's yaml keys (x), after moving
    `p` onto what the reference's configuration can express -- its depth file has 5 levels, it reads the reward's constants as
    float (base.cpp:14-60), and quoting off the book comes with the mid-price as target price (market.target_price.type: any
    name but "midprice" builds MidPrice, quirk Q5)."""
    x = {}
    p.depth = 5
    assert abi.load().lob_market_preset(b"HSBA.L", __import__("ctypes").byref(p.market)) == 0
    x["ticker"] = "HSBA.L"
    order = [int(p.vars[i]) for i in range(p.n_vars)]
    x["vars"] = ", ".join('"%s"' % VAR_OF[v] for v in order)
    x["order_size"] = p.order_size
    x["reward"] = REWARD_OF[p.reward_measure]
    x["pos_lb"], x["pos_ub"] = p.pos_lb, p.pos_ub
    p.damping_factor, p.pos_weight, p.pnl_weight = f32(p.damping_factor), f32(p.pos_weight), f32(p.pnl_weight)
    x["damping"], x["pos_weight"], x["pnl_weight"] = repr(p.damping_factor), repr(p.pos_weight), repr(p.pnl_weight)
    for name in ("lb_mpm", "lb_vlt", "lb_svl", "lb_vwap", "lb_rsi", "lb_spread", "lb_pnl", "lb_target"):
        x[name] = int(getattr(p, name))
    if p.quote_mode == abi.QUOTE_BOOK:
        p.target_price = abi.TP_MIDPRICE
        x["tp"] = "book"
    else:
        x["tp"] = "midprice" if p.target_price == abi.TP_MICROPRICE else "microprice"
    x["mem"] = p.memory_size
    for i in range(3):
        x["w%d" % i] = repr(p.group_weights[i])
    x["gamma"], x["lambda"], x["alpha"], x["beta"] = repr(p.gamma), repr(p.lambda_), repr(p.alpha), repr(p.beta)
    x["agent_seed"] = p.seed + p.book_id_offset
    return ALGOS[p.algo][0], x


def natural_steps(p, day):
    """Learner steps a fresh one-book oracle takes on `day` before it ends."""
    o = ol.Oracle(p, day[None])
    o.reset()
    o.td_step(len(day) + 2)
    n, end = int(o.counters()[0]), int(o.rec(0)["book"]["terminal"])
    o.close()
    return n, end


SEEN = {"compared": 0, "init_failed": 0, "dry": 0, "capped": 0, "close": 0, "episodes": 0}
N_CASES = max(1, int(os.environ.get("LOB_REF_SWEEP", "200")) // 4)


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref/ref_harness not built (needs the reference checkout)")
@pytest.mark.parametrize("seed", range(N_CASES))
def test_a_day_per_episode_against_the_reference(seed):
    """The reference's training loop over recorded days -- rs.sample() + LoadData + RunEpisode, src/main.cpp:53-55 -- on random
    configurations (test_gpu_fuzz.random_case), 2-3 episodes, each on a day of its own length drawn from 150-900 events:
    the first runs until its data is dry, the second is cut by a step cap at half its natural length, and a third, where the
    generator can place it (two trade slots), runs into the session's close.  A one-book oracle driven by set_days walks the
    harness's trajectory: the fields and rules of test_oracle_ref_sweep.py's multi-episode cases (replay_multi: exact), and the
    weights at the end."""
    r = np.random.default_rng(93000 + seed)
    p, g, _B = random_case(7000 + seed)
    algo, x = harness_args(p)
    episodes = int(r.integers(2, 4))
    lengths = [int(n) for n in r.choice(np.arange(150, 901), size=episodes, replace=False)]
    days = make_days(lengths, first_id=p.book_id_offset + 50, gen=g, trades=p.max_trades)
    close = episodes == 3 and p.max_trades == TRADES
    if close:
        days[2] = day_into_the_close(p, lengths[2], int(r.integers(lengths[2] // 3, lengths[2] - 20)), p.book_id_offset + 99)
    nat = [natural_steps(p, d) for d in days]
    caps = [1 << 40] * episodes
    if nat[1][0] >= 2:
        caps[1] = nat[1][0] // 2
    x["episodes"], x["steps"] = episodes, ",".join(str(c) for c in caps)
    tag = "days seed %d (%s, %s, days of %s events, caps %s)" % (seed, algo, x["reward"], lengths, x["steps"])
    lib = ol.DayLibrary(days)
    o = ol.Oracle(p, days[0][None])
    ep_of = {"next": 0}

    def reset():
        o.set_days(*lib.of([ep_of["next"]]))
        ep_of["next"] += 1
        o.reset()

    with tempfile.TemporaryDirectory() as td:
        tb = os.path.join(td, "theta_b.bin")
        if "double" in algo:
            x["theta_b_out"] = tb
        try:
            traj, info, theta = ol.run_ref_episode(days, trades=p.max_trades, algo=algo, mem=p.memory_size, seed=p.seed,
                                                   rng_stream=p.book_id_offset, eps=p.epsilon, extra=x)
        except RuntimeError as e:
            if "Initialise failed" not in str(e):
                raise
            # the data of some day ends before the look-back windows are full: the oracle takes no step on that day either
            stuck = False
            for ep in range(episodes):
                before = int(o.counters()[0])
                reset()
                o.td_step(min(caps[ep], len(days[ep]) + 2))
                stuck = stuck or int(o.counters()[0]) == before
                o.clear_inventory(); o.handle_terminal()
            assert stuck, tag + ": the reference's Initialise fails on one of these days"
            SEEN["init_failed"] += 1
            o.close()
            return
        theta_b = sparse(tb) if "double" in algo else None
    ends = list(info["ends"])
    assert len(ends) == episodes, tag
    replay_multi({"traj": traj, "ends": np.array(ends)}, reset, lambda: o.td_step(1), o.clear_inventory,
                 lambda: ol.load().oracle_handle_terminal(o.h), lambda: o.rec(0), tag)
    assert ep_of["next"] == episodes, tag
    check_sparse(o.theta(0), theta[0], theta[1], tag)
    if theta_b is not None:
        check_sparse(o.theta_b(0), theta_b[0], theta_b[1], tag + " theta_b")
    # what this case has covered: how each of its days ended in the reference (0: step cap, 1: the close, 2: out of data)
    if nat[0][1] == 2:
        assert ends[0] == 2, (tag, ends)
    if caps[1] < (1 << 40):
        assert ends[1] == 0, (tag, ends)
    SEEN["compared"] += 1
    SEEN["episodes"] += episodes
    SEEN["dry"] += ends.count(2)
    SEEN["capped"] += ends.count(0)
    SEEN["close"] += ends.count(1)
    o.close()


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref/ref_harness not built (needs the reference checkout)")
def test_zz_what_the_day_sweep_covered():
    """Over the sweep above: days that ran dry inside their episode, days cut by a step cap and -- with the default case
    count or more -- days that ran into the close were all compared with the reference."""
    print("day sweep against the reference: %s" % SEEN)
    if SEEN["compared"] + SEEN["init_failed"] < N_CASES:
        return      # (only part of the sweep ran in this process: -k, or spread over workers)
    assert SEEN["compared"] >= 1 and SEEN["dry"] >= 1 and SEEN["capped"] >= 1, SEEN
    if N_CASES >= 50:
        assert SEEN["close"] >= 1, SEEN
        assert 2 * SEEN["compared"] >= N_CASES, SEEN
