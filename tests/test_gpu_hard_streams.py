"""What vendor depth and trade files do, through the fast env-step kernels.

Every stream the other GPU files feed env_step_kernel, env_step16_kernel and the fused act / learn paths comes from
gen_stream_host: fixed cadence, a spread of one or two ticks, prices exactly on the grid, trades at the touch or the second
level, no dry time-and-sales tail.  tests/hard_streams.py turns such a batch into one whose rows share timestamps, are crossed
(singly and in runs: events of three rows and more), carry prices one float off the grid, trades deep in the book, beyond it
and inside the spread, jump by several ticks, and end in a LOB_EVT_FLAG_TAS_DRY tail -- so that one wave holds a lane inside a
three-row event beside a lane on a crossed row and a lane whose stream has gone dry.  The engine runs that batch step by step
against tests/oracle_lib, which tests/test_hard_streams.py pins on such streams against the unmodified reference and which it
proves to contain each pathology in rows the books consume.

Shapes as in tests/test_gpu_env_pass.py: 200 books (three full waves and a partial one of the lane-per-book kernel,
LOB_ENV16_MAX=0; 50 waves of the 16-lane one), 400 events, D = 10, T = 2, one shared weight vector of 1 << 20 weights, two
episodes of 60 steps.  Books, state variables, actions, rewards and RNG counters bit for bit; TD errors and weights as that file
compares them under a shared vector (rtol 1e-9)."""
import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import hard_streams as hs
from tests import oracle_lib as ol
from tests.parity import compare_env, compare_learner_step
from tests.test_gpu_steady import light_books

pytestmark = pytest.mark.gpu

B, N_EVENTS, EPISODES, STEPS = hs.B, hs.N_EVENTS, 2, 60
KERNELS = ["lane_per_book", "sixteen_lanes"]
FAST = {"LOB_Q_LANES": "1", "LOB_Q_PAIR": "1", "LOB_FUSE_ACT": "1"}


def fast_kernels(monkeypatch, kernel):
    # the fused env step and the lane learner kernels, which a batch of 200 would not select by its size
    for k, v in FAST.items():
        monkeypatch.setenv(k, v)
    if kernel == "lane_per_book":
        monkeypatch.setenv("LOB_ENV16_MAX", "0")


def params(algo=abi.ALGO_QLAMBDA, trades=hs.TRADES, theta_mode=abi.THETA_SHARED):
    p = engine.default_params()
    p.depth, p.max_trades = hs.DEPTH, trades
    p.algo, p.theta_mode, p.memory_size = algo, theta_mode, 1 << 20
    return p


def compare_theta(eng, orc, p, n_books):
    np.testing.assert_allclose(eng.theta(), orc.theta(), rtol=1e-9, atol=1e-12)
    if p.algo == abi.ALGO_DOUBLE_Q:
        np.testing.assert_allclose(eng.theta(1), orc.theta_b(), rtol=1e-9, atol=1e-12)


def run_episodes(p, rec, tag, episodes=EPISODES, steps=STEPS, exact=False, want_light=True):
    n_books = rec.shape[0]
    eng = engine.Engine(p, n_books)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    light0 = light_books(eng)
    for episode in range(episodes):
        eng.reset(); orc.reset()
        for step in range(steps):
            eng.td_step(1); orc.td_step(1)
            compare_learner_step(eng, orc, "%s, episode %d step %d" % (tag, episode, step), exact=exact, rtol=1e-9)
        eng.clear_inventory(); orc.clear_inventory()
        compare_env(eng, orc, "%s, episode %d after ClearInventory" % (tag, episode))
        eng.handle_terminal(); orc.handle_terminal()
    if want_light:
        # the fused env step was the kernel running: the books' actions came from their hit lists
        assert light_books(eng) - light0 > 0
    if exact:
        for b in range(n_books):
            np.testing.assert_array_equal(eng.theta(b), orc.theta(b), err_msg="%s theta of book %d" % (tag, b))
    else:
        compare_theta(eng, orc, p, n_books)
    eng.close()
    orc.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", list(hs.CASES))
def test_each_kind_through_the_fused_env_step(monkeypatch, case, kernel):
    fast_kernels(monkeypatch, kernel)
    rec, counts, _ = hs.batch(case)
    for k in hs.CASES[case][0] + (("dry",) if hs.CASES[case][1] else ()):
        assert counts[k] > 0, counts
    run_episodes(params(), rec, "%s / %s" % (case, kernel))


@pytest.mark.parametrize("algo,kernel", [(abi.ALGO_SARSA, "lane_per_book"), (abi.ALGO_SARSA, "sixteen_lanes"),
                                         (abi.ALGO_DOUBLE_Q, "lane_per_book")])   # (double Q never takes the 16-lane kernel)
def test_all_kinds_and_a_dry_tail_under_sarsa_and_double_q(monkeypatch, algo, kernel):
    fast_kernels(monkeypatch, kernel)
    # (the hit-list count is asserted for Q(lambda) above and for SARSA(lambda) here: the fused env step of double Q keeps no such count)
    run_episodes(params(algo), hs.batch("all+dry")[0], "all+dry, algo %d / %s" % (algo, kernel), want_light=algo != abi.ALGO_DOUBLE_Q)


@pytest.mark.parametrize("kernel", KERNELS)
def test_to_the_end_of_the_data(monkeypatch, kernel):
    """Every book to its last row: the rows next to the end (crossed ones among them: an event that never completes), the dry
    tails, books finishing at different steps of one wave.  Then ClearInventory, HandleTerminal and a second episode."""
    fast_kernels(monkeypatch, kernel)
    p = params()
    rec = hs.batch("all+dry")[0]
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    light0 = light_books(eng)
    eng.reset(); orc.reset()
    for step in range(N_EVENTS + 2):
        eng.td_step(1); orc.td_step(1)
        compare_learner_step(eng, orc, "to the end / %s, step %d" % (kernel, step), exact=False, rtol=1e-9)
        if (eng.get_terminal() != 0).all():
            break
    assert (eng.get_terminal() != 0).all()
    assert eng.counters()[0] == orc.counters()[0]
    eng.clear_inventory(); orc.clear_inventory()
    compare_env(eng, orc, "to the end / %s after ClearInventory" % kernel)
    eng.handle_terminal(); orc.handle_terminal()
    eng.reset(); orc.reset()
    for step in range(30):
        eng.td_step(1); orc.td_step(1)
        compare_learner_step(eng, orc, "to the end / %s, second episode step %d" % (kernel, step), exact=False, rtol=1e-9)
    assert light_books(eng) - light0 > 0
    compare_theta(eng, orc, p, B)
    eng.close()
    orc.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_multi_row_events_across_ring_refills(monkeypatch, kernel):
    """A 256-entry market-track ring refilled every 16 steps (the values of tests/test_gpu_replay.py); half the books have three
    crossed rows, the middle one with its predecessor's timestamp, across row 256: an event of four rows or more.  The pre-pass
    stops between track entries, never inside an event: lob_reset fills entries 0 .. 251 (the ring less its margin of four) and
    the first refill goes on from entry 252.  So half the books also have a run of crossed rows as event 251 -- the pre-pass
    stops behind a multi-row event, and the trade list of the first event after the refill is merged from that event's rows."""
    fast_kernels(monkeypatch, kernel)
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    stop = 256 - 4
    rec, counts, rows = hs.batch("all", straddle=256, straddle_entry=stop)
    run_of_three = rows["crossed"][:, 255] & rows["crossed"][:, 256] & rows["crossed"][:, 257] & rows["same_time"][:, 256]
    assert run_of_three.sum() >= B // 4
    # from the final records: event 251 spans four rows or more, and event 252's list holds trades of two rows or more
    tv = rec[:, :, 2 + 4 * hs.DEPTH + hs.TRADES:2 + 4 * hs.DEPTH + 2 * hs.TRADES]
    at_stop, first_252 = np.zeros(B, bool), np.zeros(B, np.int64)
    for b in range(B):
        first = np.flatnonzero(hs.event_firsts(rec[b], hs.DEPTH))
        if len(first) > stop + 1 and first[stop] - first[stop - 1] >= 4:
            at_stop[b] = ((tv[b, first[stop - 1] + 1:first[stop] + 1] > 0).any(axis=1).sum() >= 2)
            first_252[b] = first[stop]
    assert at_stop.sum() >= B // 4, at_stop.sum()
    p = params()
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    eng.kernel_timing(True)
    eng.reset(); orc.reset()
    for step in range(N_EVENTS + 2):
        eng.td_step(1); orc.td_step(1)
        compare_learner_step(eng, orc, "ring / %s, step %d" % (kernel, step), exact=False, rtol=1e-9)
        if (eng.get_terminal() != 0).all():
            break
    assert (eng.get_terminal() != 0).all()
    # the books with the runs went through them: their cursors ended beyond row 257, and beyond the first row of event 252
    cursor = orc.recs()["book"]["cursor"]
    assert (cursor[run_of_three] > 257).any()
    assert (cursor[at_stop] > first_252[at_stop]).sum() >= B // 4
    eng.sync()
    _, refills = eng.kernel_time_ms("prepass_extend_kernel")
    assert refills >= 3, refills
    compare_theta(eng, orc, p, B)
    eng.close()
    orc.close()


def test_general_kernel_shared_theta():
    """The same batch with four trade slots per record: env_kernel, not the fused env step."""
    from tests.test_gpu_parity import _repack_trades
    rec = _repack_trades(hs.batch("all+dry")[0], hs.DEPTH, hs.TRADES, 4)
    run_episodes(params(trades=4), rec, "all+dry, four trade slots", want_light=False)


def test_general_kernel_private_theta_bit_for_bit():
    from tests.test_gpu_parity import _repack_trades
    rec = _repack_trades(hs.batch("all+dry")[0][:8], hs.DEPTH, hs.TRADES, 4)
    p = params(trades=4, theta_mode=abi.THETA_PRIVATE)
    run_episodes(p, rec, "all+dry, four trade slots, private theta", exact=True, want_light=False)


@pytest.mark.parametrize("kernel", KERNELS)
def test_environment_face(monkeypatch, kernel):
    """lob_step with random actions, every seventh step lob_eval_step, until every stream is exhausted (the pattern of
    tests/test_gpu_fuzz.py::test_random_configuration_env_only)."""
    fast_kernels(monkeypatch, kernel)
    p = params()
    rec = hs.batch("all+dry")[0]
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    eng.reset(); orc.reset()
    compare_env(eng, orc, "env face / %s reset" % kernel)
    rng = np.random.default_rng(5)
    for step in range(N_EVENTS + 2):
        if step % 7 == 6:
            eng.eval_step(1)
            orc.eval_step(1)
        else:
            acts = rng.integers(0, 9, size=B).astype(np.int32)
            eng.step(acts)
            orc.env_step(acts)
        compare_env(eng, orc, "env face / %s step %d" % (kernel, step))
        live = eng.get_terminal() == 0
        np.testing.assert_array_equal(eng.get_reward()[live], orc.recs()["reward"][live], err_msg="env face / %s step %d reward" % (kernel, step))
        if (eng.get_terminal() != 0).all():
            break
    assert (eng.get_terminal() != 0).all()
    eng.close()
    orc.close()


def test_day_library_of_hardened_days(monkeypatch):
    """Six hardened days of unequal length (the LENGTHS of tests/test_gpu_days_shared.py, hardened one book at a time), played
    through load_days / days_set against Oracle.set_days: one episode to the end."""
    from tests.test_gpu_days import make_days
    from tests.test_gpu_days_shared import LENGTHS
    fast_kernels(monkeypatch, "lane_per_book")
    days, total = [], {k: 0 for k in hs.KINDS + ("dry",)}
    for i, d in enumerate(make_days(LENGTHS, depth=hs.DEPTH)):
        h, c = hs.harden(d[None], hs.DEPTH, hs.TRADES, hs.SEED + 1, dry=True, book0=i)
        days.append(h[0])
        for k in total:
            total[k] += c[k]
    assert all(total[k] > 0 for k in total), total
    lib = ol.DayLibrary(days)
    p = params()
    assign = np.random.default_rng(3).integers(0, len(days), size=B).astype(np.int32)
    assert len(set(assign)) == len(days)
    eng = engine.Engine(p, B)
    eng.load_days(days)
    orc = ol.Oracle(p, np.stack([days[0]] * B))
    eng.days_set(assign)
    eng.reset()
    np.testing.assert_array_equal(eng.days(), assign)
    orc.set_days(*lib.of(assign))
    orc.reset()
    for step in range(max(LENGTHS) + 2):
        eng.td_step(1); orc.td_step(1)
        compare_learner_step(eng, orc, "hardened days, step %d" % step, exact=False, rtol=1e-9)
        n_live = int(eng.counters()[2])
        assert n_live == int(orc.counters()[2]), step
        if n_live == 0:
            break
    assert int(eng.counters()[2]) == 0
    assert eng.counters()[0] == orc.counters()[0]
    eng.clear_inventory(); orc.clear_inventory()
    compare_env(eng, orc, "hardened days after ClearInventory")
    eng.handle_terminal(); orc.handle_terminal()
    compare_theta(eng, orc, p, B)
    eng.close()
    orc.close()
