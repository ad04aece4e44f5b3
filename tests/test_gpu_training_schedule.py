"""The reference's training run against the oracle, at scale: a fresh day every episode (src/main.cpp:51-55), one shared weight
vector, and epsilon falling at every episode boundary as EpsilonGreedy::HandleTerminal moves it (src/rl/policy.cpp:79-82).  With
config/example.yaml epsilon is below 0.34 from episode 77 of 1 000 on; below 0.34 the engine sums the combined update per block
by dense slot ids (lob_engine.hip acc_blocked) for Q(lambda) and keeps every book's trace generations -- the flow that most of a
real run goes through.  tests/test_gpu_steady.py meets it in single short episodes; here it is crossed at an episode boundary,
on library days (lob_load_days: the memo / hit-list fast path that only shared theta takes), and on a stream staged while the
episode before it runs (lob_stage_events).

Every test also asserts that no step went by a hint word that had not arrived (Engine.hint_stats): the act / update path a
step takes depends on the learn kernels' hand-back count read from host-mapped memory, and the flow counters asserted here only
say which path the oracle has checked if the count decided it."""
import ctypes as C
import threading

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import days_ref
from tests import oracle_lib as ol
from tests.parity import compare_learner_step
from tests.test_gpu_days import make_days
from tests.test_gpu_steady import episode_length, fp_stats_line, light_books, make

pytestmark = pytest.mark.gpu

# config/example.yaml's schedule (policy.eps_init / eps_floor, read as float: main.cpp:149-150, lob_host.hpp Agent) with eps_T
# compressed from 800 to 4.1, so that three episodes run at eps(0), eps(1), eps(2) ~ 0.80, 0.089, 0.010: the reference's episodes
# 1-3 (HandleTerminal(0) after its episode 0 leaves eps_init), the first above the 0.34 switch, the other two below it
EPS_INIT, EPS_FLOOR, EPS_T = float(np.float32(0.8)), float(np.float32(1e-4)), 4.1
SWITCH = 0.34


def eps_after(episode):
    """EpsilonGreedy::HandleTerminal(episode) (policy.cpp:81)."""
    return EPS_INIT * pow(EPS_FLOOR / EPS_INIT, episode / EPS_T)


def set_epsilon(eng, orc, eps):
    eng.set_epsilon(eps)
    ol.load().oracle_set_epsilon(orc.h, C.c_double(eps))


def flow_delta(after, before):
    return {k: after[k] - before[k] for k in after}


def assert_hints_arrived(eng, tag):
    hs = eng.hint_stats()
    assert hs["hint_missed"] == 0, (tag, hs)
    return hs


def compare_theta(eng, orc, algo, tag, min_written, shadow=None):
    """theta (and double Q's theta_b) against the oracle's: the same non-zero pattern, rtol 1e-9.  With a `shadow` oracle (below)
    the absolute floor is 100 x how far the shadow has drifted from the oracle, as in test_gpu_steady.py's timed-kernel sweep."""
    pairs = [(eng.theta(), orc.theta(), shadow.theta() if shadow else None, "")]
    if algo == abi.ALGO_DOUBLE_Q:   # DoubleAgent::theta_b
        pairs.append((eng.theta(1), orc.theta_b(), shadow.theta_b() if shadow else None, " theta_b"))
    drifts = []
    for th, oth, sth, what in pairs:
        assert np.array_equal(th != 0, oth != 0) and np.count_nonzero(th) > (min_written if not what else 0), \
            (tag + what, np.count_nonzero(th), np.count_nonzero(oth))
        drift = float(np.abs(sth - oth).max()) if sth is not None else 0.0
        # (a shadow that has left the oracle's trajectory -- another action somewhere -- would make the floor meaningless)
        assert drift < 1e-6, (tag + what, "shadow drift", drift)
        np.testing.assert_allclose(th, oth, rtol=1e-9, atol=max(1e-12, 100.0 * drift), err_msg=tag + what)
        drifts.append(drift)
    return drifts


def td_steps(eng, orc, shadow=None):
    """One learner step of the engine and the oracle -- and of the shadow oracle beside them, in a thread of its own (ctypes
    releases the GIL: the oracles' serial update phases overlap)."""
    t = threading.Thread(target=shadow.td_step) if shadow else None
    if t:
        t.start()
    eng.td_step(1); orc.td_step(1)
    if t:
        t.join()


# The library: 6 days of one length (the batched oracle holds one length: tests/test_gpu_days.py), each from its own generator
# book id.  ~300 events would be ~145 learner steps an episode; 120 events (41 steps) keep three episodes of three algorithms
# against two 32 768-book oracles inside the suite's budget, and every step around the switch is still compared.
N_DAYS, DAY_LEN = 6, 120


@pytest.mark.parametrize("algo", [abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q, abi.ALGO_SARSA], ids=["qlambda", "double_q", "sarsa"])
def test_training_schedule_on_library_days(algo):
    """32 768 books (the smallest batch that takes the lane-per-book kernels with no switch set), D = 10, two trade slots, M = 20 M,
    one shared weight vector, a library of 6 days: three episodes of the reference's training loop -- lob_days_select(RANDOM) and
    lob_reset (a day drawn per book on the device, RandomSampler's draws: tests/days_ref.py), steps until no book is live,
    ClearInventory, HandleTerminal and the next epsilon (lob_host.hpp Agent::HandleTerminal) -- against a batched oracle whose
    record buffer is rewritten in place with each book's drawn day.  Compared: steps 0-3, every 8th step, every step of the last
    10, after ClearInventory, and theta at the end of every episode.

    The flow counters pin the combined update each episode took: Q(lambda) adds its updates in place above the switch and sums
    them by dense slot ids in every step below it; SARSA(lambda) sums by dense ids in every step; double Q is left out of
    acc_blocked (lob_engine.hip), so it adds its updates in place in every episode, at low epsilon too, while its books keep
    generations as SARSA's do.

    Below the switch this configuration amplifies rounding noise: with every book keeping its generations, TD errors of
    |delta| ~ 4 000 and one weight vector, a 1e-13 nudge to the oracle's weights after step 3 (a shadow oracle,
    test_gpu_steady.py's method) has grown to 6e-9 in the TD errors 18 steps into the second episode, and to 1e-10 - 3e-8 in
    theta by the end of the third.  The engine's f64 atomics add such noise in every step: with a plain 1e-12 floor, Q(lambda)
    failed on 32 of 20 M weights (1.9e-9 relative at most); at the first step where any weight parted, the engine missed 7 weights
    of 0.014 by 1.7e-11 and the shadow missed the same ones by 6e-12, with no action, trace count or TD error apart.
    So theta is held to 100 x the shadow's drift (rtol stays 1e-9), and the shadow must stay within 1e-6."""
    B = 32768
    days = make_days([DAY_LEN] * N_DAYS, depth=10)
    days_arr = np.stack(days)
    p = engine.default_params()
    p.depth, p.max_trades = 10, 2
    p.algo, p.theta_mode, p.memory_size = algo, abi.THETA_SHARED, 20000000
    p.epsilon = eps_after(0)
    # the first draw of 32 768 consecutive seeds is one or two neighbouring days for every book (minstd_rand0's first value is
    # 16807 x seed): drawn and replaced before the first reset, as tests/test_gpu_days.py does; the episodes play draws 2-4
    draws = np.array([days_ref.book_days(p.seed, b, N_DAYS, 4) for b in range(B)])[:, 1:]
    eng = engine.Engine(p, B)
    eng.load_days(days)
    eng.days_select(abi.DAYS_RANDOM, 0, N_DAYS)
    orc = ol.Oracle(p, days_arr[draws[:, 0]])
    shadow = ol.Oracle(p, orc.records)       # (the same record buffer)
    eps = [eps_after(k) for k in range(3)]
    assert eps[0] > SWITCH > eps[1] > eps[2], eps
    for ep in range(3):
        tag = "schedule algo %d episode %d (eps %.4g)" % (algo, ep, eps[ep])
        eng.days_select(abi.DAYS_RANDOM, 0, N_DAYS)
        eng.reset()
        d = eng.days()
        np.testing.assert_array_equal(d, draws[:, ep], err_msg=tag + " days drawn")
        assert len(np.unique(d)) == N_DAYS
        if ep:
            orc.records[...] = days_arr[d]      # (the oracle reads this buffer in place)
        orc.reset(); shadow.reset()
        T, live = episode_length(p, orc.records, B)
        assert 30 < T < 400 and live[T - 2] > 0, (tag, T)
        flow0, light0 = eng.flow_stats(), light_books(eng)
        for step in range(T):
            td_steps(eng, orc, shadow)
            if ep == 0 and step == 3:
                th = shadow.theta()
                th[th != 0] *= 1.0 + 1e-13
            n_live = int(eng.counters()[2])
            assert n_live == int(orc.counters()[2]) == live[step], (tag, step, n_live, int(orc.counters()[2]), live[step])
            if step < 4 or step % 8 == 7 or step >= T - 10:
                compare_learner_step(eng, orc, "%s step %d of %d (%d live)" % (tag, step, T, n_live), exact=False, rtol=1e-9)
        assert eng.counters()[2] == 0 and orc.counters()[2] == 0
        flow = flow_delta(eng.flow_stats(), flow0)
        served = light_books(eng) - light0
        hs = assert_hints_arrived(eng, tag)
        print("%s: %d steps, flow %s, hit-list books %d of %d live book-steps, hints %s" % (tag, T, flow, served, sum(live), hs))
        if algo == abi.ALGO_SARSA or (algo == abi.ALGO_QLAMBDA and eps[ep] < SWITCH):
            assert flow["dense_sums"] == T and flow["block_sums"] == T and flow["added_in_place"] == 0, (tag, flow)
        else:
            # (the first step of an episode acts without hit lists: act_fast_kernel, not the fused flow)
            assert flow["added_in_place"] >= T - 1 and flow["dense_sums"] == 0 and flow["block_sums"] == 0, (tag, flow)
        assert flow["every_book"] == 0, (tag, flow)
        assert served > 0, (tag, served)
        drift = compare_theta(eng, orc, algo, tag, 20000, shadow)
        print("%s: shadow drift %s" % (tag, drift))
        eng.clear_inventory(); orc.clear_inventory(); shadow.clear_inventory()
        compare_learner_step(eng, orc, tag + " after ClearInventory", exact=False, rtol=1e-9)
        eng.handle_terminal(); orc.handle_terminal(); shadow.handle_terminal()
        if ep < 2:
            set_epsilon(eng, orc, eps[ep + 1])
            ol.load().oracle_set_epsilon(shadow.h, C.c_double(eps[ep + 1]))
    assert eng.hint_stats()["hint_read"] > 0
    eng.close()
    orc.close()
    shadow.close()


def test_double_q_mostly_greedy_at_scale():
    """Double Q at epsilon 0.05 (example.yaml's default algorithm late in its schedule): acc_blocked
    leaves it out, so it adds its updates in place while its books keep SARSA-like generation counts -- 32 768 books, M = 20 M,
    40 steps against the oracle (every 4th compared), both weight vectors, and the fast path's statistics printed."""
    B = 32768
    p, eng, orc = make(B, abi.ALGO_DOUBLE_Q, n_events=200, epsilon=0.05)
    eng.reset(); orc.reset()
    flow0 = eng.flow_stats()
    for step in range(40):
        eng.td_step(1); orc.td_step(1)
        if step < 2 or step % 4 == 3:
            compare_learner_step(eng, orc, "double Q at eps 0.05, step %d" % step, exact=False, rtol=1e-9)
    flow = flow_delta(eng.flow_stats(), flow0)
    st = eng.fastpath_stats()
    deferred = eng.deferred_generations()
    hs = assert_hints_arrived(eng, "double Q at eps 0.05")
    print("double Q at eps 0.05: flow %s, fast path %s, deferred generations %d, hints %s" % (flow, fp_stats_line(st), deferred, hs))
    assert flow["added_in_place"] >= 39 and flow["dense_sums"] == 0 and flow["block_sums"] == 0, flow
    assert st["list_len_max"] is not None and st["list_len_max"] > 0, fp_stats_line(st)
    compare_theta(eng, orc, abi.ALGO_DOUBLE_Q, "double Q at eps 0.05", 20000)
    eng.close()
    orc.close()


def test_staged_stream_against_the_oracle(monkeypatch):
    """lob_stage_events against the oracle: 4 096 books (BASELINE config 2's batch and dispatch -- env_step16_kernel, no switch
    set), SARSA(lambda), shared theta.  Episode 1 runs on stream A while stream B (same length, another generator seed) is handed
    over in pieces of 1 000 records, so that the hand-over is still going on while the steps run; after ClearInventory and
    HandleTerminal, lob_reset adopts B and the oracle's records are overwritten with it.  Both episodes run until no book is
    live, every step compared."""
    monkeypatch.setenv("LOB_UPLOAD_PIECE_RECS", "1000")
    B, n_events = 4096, 120
    p, eng, orc = make(B, abi.ALGO_SARSA, n_events=n_events)
    g = engine.default_gen_params()
    g.n_events = n_events
    g.seed = 777
    rec_b = engine.gen_stream_host(g, p.depth, p.max_trades, 0, B)
    assert not np.array_equal(rec_b, orc.records)
    eng.reset(); orc.reset()
    eng.stage_events(rec_b)              # ... and the steps of episode 1 go on
    for episode in range(2):
        step = 0
        while True:
            eng.td_step(1); orc.td_step(1)
            compare_learner_step(eng, orc, "staged, episode %d step %d" % (episode, step), exact=False, rtol=1e-9)
            n_live = int(eng.counters()[2])
            assert n_live == int(orc.counters()[2]), (episode, step)
            step += 1
            if n_live == 0:
                break
            assert step < 300, "episode %d does not end" % episode
        assert step > 20, step
        compare_theta(eng, orc, abi.ALGO_SARSA, "staged, episode %d" % episode, 5000)
        eng.clear_inventory(); orc.clear_inventory()
        compare_learner_step(eng, orc, "staged, episode %d after ClearInventory" % episode, exact=False, rtol=1e-9)
        eng.handle_terminal(); orc.handle_terminal()
        if episode == 0:
            orc.records[...] = rec_b         # (the oracle reads this buffer in place)
            eng.reset(); orc.reset()         # (eng: adopts the staged stream)
    hs = assert_hints_arrived(eng, "staged")
    print("staged: flow %s, hints %s" % (eng.flow_stats(), hs))
    eng.close()
    orc.close()
