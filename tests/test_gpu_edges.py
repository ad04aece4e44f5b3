"""The engine against the oracle at the edges of what lob_create accepts.

The other GPU files draw from tests/test_gpu_fuzz.py::random_case: depth 3 / 5 / 10, one, two or four trade slots, look-backs up to
100, tables of 4 099 .. 20 M weights, epsilon-greedy, seven of the nine reward measures.  lob_create takes depth 1 .. 10, 1 .. 8
trade slots, look-backs up to 256 (LOB_MAX_WINDOW), tables of 1 .. 2^31 - 1 weights, Boltzmann and all nine measures.  This file
goes to those edges, section by section:

  depth        D in {1, 2, 4, 6, 7, 8, 9} on hardened streams (tests/hard_streams.py) through the fast kernels, both env-step forms
  trade slots  T in {3, 5, 6, 7, 8} through the general kernels; a crafted batch whose merged trade lists hold exactly eight keys
  look-backs   windows of 101 .. 256 events: the pre-pass rings, the agent's own rings (pnl_ups / pnl_downs under REWARD_NORMED),
               the snapshot layout of 2 w rows, prepass_extend_kernel resuming windows of 256 across ring refills
  table size   M in {1, 2, 31 .. 33, 63 .. 65, 4 098}: the word-count edges of the written-weights bitmaps; 2^27 - 1 / 2^27 / 2^27 + 1:
               the threshold between learn_q_pair_kernel and learn_q_lane_kernel; 2^31 - 1: the end of the 32-bit modular arithmetic
  policy       Boltzmann (tau 0.5 / 5 / 50, lob_set_tau) and every reward measure -- REWARD_MM_EXP's expf and REWARD_NONE among
               them -- through the general kernels, the fused env step in both forms, and a batch that selects the fused action
               selection by its size

tests/oracle_lib is the yardstick; tests/test_oracle_ref_edges.py holds it against the unmodified reference on the same draws
(D = 5: the reference reads five-level files only; at other depths the oracle is the specification, as it is for D = 3 and 10).

Conventions (tests/test_gpu_hard_streams.py, tests/test_gpu_steady.py): two episodes of 60 steps with ClearInventory and
HandleTerminal between them.  Private theta or one book: everything for equality, weights included.  One shared vector and
several books: books, actions, rewards, state variables and RNG counters for equality, TD errors and weights at rtol 1e-9 beside
a shadow oracle whose weights are nudged by 1e-13 after step 3 -- the rule of test_random_configuration_timed_kernels: the TD
floor is 100 x the shadow's drift, and a case ends early, counted, once the shadow itself takes another action (or the engine
crosses a tie first where the shadow has blown its nudge up a thousandfold).  tests/test_edge_cases.py runs that shadow alone on
the CPU over the same cases: at most one case in ten of a sweep may end early.

Every case shows from the engine which kernels it ran: Engine.launches (lob_debug_launches), lob_get_path_stats, the hit-list
count of lob_debug_light.

The vector-env look-ahead family (lob_vec_peek, lob_vec_rollout, the branch calls) restates half of a step of its own
(rl_markets_amd/csrc/lob_peek.h): tests/test_gpu_lookahead_edges.py takes it to the same edges of depth, trade slots and window."""
import ctypes as C
import os

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import edge_cases as ec
from tests import hard_streams as hs
from tests import oracle_lib as ol
from tests.parity import compare_env, compare_learner_step
from tests.test_gpu_hard_streams import fast_kernels
from tests.test_gpu_steady import VARIANTS, light_books

pytestmark = pytest.mark.gpu

EPISODES, STEPS = 2, 60
KERNELS = list(ec.KERNELS)
ENV_KERNEL_OF = {"lane_per_book": "env_step_kernel", "sixteen_lanes": "env_step16_kernel"}
# (the two sweeps apart from the fixed-shape cases beside them: the cap on cases cut short is over a sweep's own shared-theta cases)
SECTIONS = ("depth", "slots", "lookback_sweep", "lookbacks", "table", "big_tables", "policy_general", "policy_fast", "policy")
RAN = {s: 0 for s in SECTIONS}          # shared-theta cases with more than one book, per section
CUT = {s: [] for s in SECTIONS}         # ... of which the shadow oracle ended early
SEEN = {"boltzmann": {}, "mm_exp": {}, "non_greedy": 0, "boltzmann_steps": 0}   # what the policy sweep went through, per env-step form


def oracle_q(orc, p):
    """Q(s, .) of every book's current state under the oracle's current weights: oracle_tiles, then the reference's order of
    additions (tests/test_gpu_vec_act.py cpu_sum); DoubleAgent::action averages the two vectors."""
    from tests.test_gpu_vec_act import cpu_sum
    obs = np.ascontiguousarray(orc.recs()["vars"][:, :p.n_vars], np.float32)
    private = p.theta_mode == abi.THETA_PRIVATE
    th = [orc.theta(b) for b in range(orc.B)] if private else orc.theta()
    q = cpu_sum(p, obs, th)
    if p.algo in (abi.ALGO_DOUBLE_Q, abi.ALGO_DOUBLE_R_LEARN):
        thb = [orc.theta_b(b) for b in range(orc.B)] if private else orc.theta_b()
        q = (q + cpu_sum(p, obs, thb)) / 2.0
    return q


def assert_close_in_pieces(a, b, atol, tag):
    # (tables of 2^27 weights: the comparison's temporaries a piece at a time)
    for lo in range(0, a.shape[0], 1 << 24):
        np.testing.assert_allclose(a[lo:lo + (1 << 24)], b[lo:lo + (1 << 24)], rtol=1e-9, atol=atol, err_msg=tag)


def max_abs_diff(a, b):
    return max(float(np.abs(a[lo:lo + (1 << 24)] - b[lo:lo + (1 << 24)]).max()) for lo in range(0, a.shape[0], 1 << 24))


def run_case(p, rec, tag, section, episodes=EPISODES, steps=STEPS, hook=None, count_non_greedy=False):
    """The engine beside the oracle over the schedule above -> what the engine says it ran.  `hook(episode, step, eng, oracles)` is
    called in front of every step."""
    B = rec.shape[0]
    exact = p.theta_mode == abi.THETA_PRIVATE or B == 1
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    shadow = None if exact else ol.Oracle(p, rec)
    oracles = (orc,) if exact else (orc, shadow)
    light0 = light_books(eng)
    noise, chaotic, non_greedy, looked = 0.0, False, 0, 0
    if not exact:
        RAN[section] += 1
    for episode in range(episodes):
        eng.reset()
        for o in oracles:
            o.reset()
        for step in range(steps):
            if hook is not None:
                hook(episode, step, eng, oracles)
            q = oracle_q(orc, p) if count_non_greedy and step % 4 == 1 else None
            eng.td_step(1)
            for o in oracles:
                o.td_step(1)
            where = "%s, episode %d step %d" % (tag, episode, step)
            if q is not None:
                took = orc.recs()["action"]
                live = eng.stepped().astype(bool)
                non_greedy += int((q[np.arange(B), took] < q.max(axis=1))[live].sum())
                looked += int(live.sum())
            if exact:
                compare_learner_step(eng, orc, where, exact=True)
                continue
            if episode == 0 and step == 3:
                th = shadow.theta()
                for lo in range(0, th.shape[0], 1 << 24):
                    piece = th[lo:lo + (1 << 24)]
                    piece[piece != 0] *= 1.0 + 1e-13
            a, b = orc.recs(), shadow.recs()
            if not np.array_equal(a["action"], b["action"]) or not np.array_equal(a["rng_ctr"], b["rng_ctr"]):
                chaotic = True
                CUT[section].append("%s at episode %d step %d" % (tag, episode, step))
                break
            noise = max(noise, float(np.abs(a["td"] - b["td"]).max()))
            try:
                compare_learner_step(eng, orc, where, exact=False, rtol=1e-9, td_floor=100.0 * noise)
            except AssertionError:
                if noise < 1e-10:
                    raise
                chaotic = True
                CUT[section].append("%s at episode %d step %d (the engine left first; shadow drift %.1e)" % (tag, episode, step, noise))
                break
        if chaotic:
            break
        eng.clear_inventory()
        for o in oracles:
            o.clear_inventory()
        compare_env(eng, orc, "%s, episode %d after ClearInventory" % (tag, episode))
        eng.handle_terminal()
        for o in oracles:
            o.handle_terminal()
    double = p.algo == abi.ALGO_DOUBLE_Q      # (lob_theta_get hands out the second vector of double Q alone)
    if exact:
        for b in range(B if p.theta_mode == abi.THETA_PRIVATE else 1):
            np.testing.assert_array_equal(eng.theta(b), orc.theta(b), err_msg="%s theta of book %d" % (tag, b))
            if double:
                np.testing.assert_array_equal(eng.theta(B + b if p.theta_mode == abi.THETA_PRIVATE else 1), orc.theta_b(b), err_msg="%s theta_b of book %d" % (tag, b))
    elif not chaotic:
        assert_close_in_pieces(eng.theta(), orc.theta(), max(1e-12, 100.0 * max_abs_diff(orc.theta(), shadow.theta())), tag + " theta")
        if double:
            assert_close_in_pieces(eng.theta(1), orc.theta_b(), max(1e-12, 100.0 * max_abs_diff(orc.theta_b(), shadow.theta_b())), tag + " theta_b")
    info = {"light": light_books(eng) - light0, "paths": eng.path_stats(), "flow": eng.flow_stats(), "launches": eng.launches(),
            "cut": chaotic, "non_greedy": non_greedy, "looked": looked, "env_steps": int(eng.counters()[0])}
    eng.close()
    for o in oracles:
        o.close()
    return info


def ran_the_fast_kernels(info, kernel, p, tag, steps=EPISODES * STEPS):
    """From the engine: the fused env step of the form asked for was the kernel launched at (nearly) every step, the lane learner
    kernel behind it, and books took their actions from hit lists or were evaluated in full inside the env step."""
    if info["cut"]:
        return
    n = info["launches"]
    other = {"env_step_kernel": "env_step16_kernel", "env_step16_kernel": "env_step_kernel"}[ENV_KERNEL_OF[kernel]]
    # (every step but each episode's first, which has no hit lists yet: act_fast_kernel + env_kernel)
    assert n[ENV_KERNEL_OF[kernel]] >= steps - 2 * EPISODES and n[other] == 0 and n["env_kernel_fused"] == 0, (tag, n)
    pair = p.memory_size < (1 << 27)
    assert n["learn_q_pair_kernel" if pair else "learn_q_lane_kernel"] >= steps - 2 * EPISODES, (tag, n)
    assert n["learn_q_lane_kernel" if pair else "learn_q_pair_kernel"] == 0 and n["learn_q_fast_kernel"] == 0, (tag, n)
    ps = info["paths"]
    assert ps[1] + ps[6] > 0, (tag, ps)


params, hardened, table_stream = ec.params, ec.hardened, ec.table_stream


# ---- 1a. depth ------------------------------------------------------------------------------------------------------------------------
DEPTHS = (1, 2, 4, 6, 7, 8, 9)
B_FAST = 130      # two full waves and a partial one of the lane-per-book env step; 33 waves of the 16-lane one


def depth_batch(D, T, B=B_FAST):
    rec, counts = hardened(D, T, B, dry=D % 2 == 0)     # (a dry tail at depths 2, 4, 6, 8)
    # every kind applies at every depth -- with one reservation: at D = 1 and 2 a "deep" trade cannot sit at level 3 or below; it is
    # then a trade at the last level, beyond the book or inside a two-tick spread (hard_streams._harden_book, `what`)
    for k in hs.KINDS + (("dry",) if D % 2 == 0 else ()):
        assert counts[k] > 0, (D, T, k, counts)
    assert abi.load().lob_validate_stream(rec.ctypes.data_as(C.c_void_p), D, T, rec.shape[0], rec.shape[1]) == 0
    return rec


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("D", DEPTHS)
def test_depth_q_lambda_through_the_fast_kernels(monkeypatch, D, T, kernel):
    fast_kernels(monkeypatch, kernel)
    p = params(D, T)
    tag = "D = %d T = %d / %s" % (D, T, kernel)
    info = run_case(p, depth_batch(D, T), tag, "depth")
    ran_the_fast_kernels(info, kernel, p, tag)
    assert info["cut"] or info["light"] > 0, (tag, info)


@pytest.mark.parametrize("algo,kernel", [(abi.ALGO_SARSA, "sixteen_lanes"), (abi.ALGO_DOUBLE_Q, "lane_per_book")], ids=["sarsa_16", "double_q_64"])
@pytest.mark.parametrize("D", DEPTHS)
def test_depth_sarsa_and_double_q_through_the_fast_kernels(monkeypatch, D, algo, kernel):
    fast_kernels(monkeypatch, kernel)
    T = 1 + D % 2
    p = params(D, T, algo)
    tag = "D = %d T = %d algo %d / %s" % (D, T, algo, kernel)
    info = run_case(p, depth_batch(D, T), tag, "depth")
    ran_the_fast_kernels(info, kernel, p, tag)
    # (the hit-list count is kept under SARSA(lambda) and Q(lambda): the fused env step of double Q keeps none)
    assert info["cut"] or algo == abi.ALGO_DOUBLE_Q or info["light"] > 0, (tag, info)


@pytest.mark.parametrize("D", DEPTHS)
def test_depth_private_theta_bit_for_bit(D):
    T = 1 + (D + 1) % 2
    p = params(D, T, (abi.ALGO_QLAMBDA, abi.ALGO_SARSA, abi.ALGO_DOUBLE_Q)[D % 3], abi.THETA_PRIVATE, mem=1 << 16)
    run_case(p, depth_batch(D, T)[:3], "D = %d T = %d private theta" % (D, T), "depth")


# ---- 1b. trade slots ----------------------------------------------------------------------------------------------------------------
SLOTS, SLOT_DEPTHS = ec.SLOTS, ec.SLOT_DEPTHS


def slots_batch(D, T):
    _, rec, counts = ec.slots_case(D, T)
    for k in hs.KINDS + ("dry",):
        assert counts[k] > 0, (D, T, k, counts)
    # the generator puts at most two trades on a row, so a merged list reaches T keys over several rows up to T = 3 (measured on the
    # CPU: merged_full is 0 from T = 5 on; the crafted batch below fills eight slots)
    if T <= 3:
        assert counts["merged_full"] > 0, (D, T, counts)
    assert counts["merged"] > 0, (D, T, counts)
    return rec


@pytest.mark.parametrize("T", SLOTS)
@pytest.mark.parametrize("D", SLOT_DEPTHS)
def test_trade_slots_shared_theta_general_kernels(D, T):
    p = ec.slots_case(D, T)[0]
    tag = "D = %d T = %d shared" % (D, T)
    info = run_case(p, slots_batch(D, T), tag, "slots")
    n = info["launches"]
    assert n["env_step_kernel"] == 0 and n["env_step16_kernel"] == 0, (tag, n)      # more than two slots: env_kernel


@pytest.mark.parametrize("T", SLOTS)
@pytest.mark.parametrize("D", SLOT_DEPTHS)
def test_trade_slots_private_theta_bit_for_bit(D, T):
    p = params(D, T, (abi.ALGO_SARSA, abi.ALGO_DOUBLE_Q, abi.ALGO_QLAMBDA)[T % 3], abi.THETA_PRIVATE, mem=1 << 16)
    run_case(p, slots_batch(D, T)[:3], "D = %d T = %d private" % (D, T), "slots")


@pytest.mark.parametrize("theta_mode", [abi.THETA_PRIVATE, abi.THETA_SHARED], ids=["private", "shared"])
def test_eight_keys_in_one_merged_trade_list(theta_mode):
    """The crafted batch of tests/edge_cases.py: events whose merged list holds exactly eight distinct keys (tests/test_edge_cases.py
    shows on the CPU that lob_validate_stream passes it, refuses a ninth key, and that the oracle's books consume those events)."""
    B = 3 if theta_mode == abi.THETA_PRIVATE else 70
    rec, runs = ec.crafted_eight_keys(D=5, B=B)
    assert abi.load().lob_validate_stream(rec.ctypes.data_as(C.c_void_p), 5, 8, B, rec.shape[1]) == 0
    p = params(5, 8, abi.ALGO_QLAMBDA, theta_mode, mem=1 << 16)
    info = run_case(p, rec, "eight keys, theta mode %d" % theta_mode, "slots", steps=70)
    assert info["env_steps"] > 0


# ---- 1c. look-backs -------------------------------------------------------------------------------------------------------------------
def all_lookbacks(p, w):
    for name in ec.LOOKBACKS:
        setattr(p, name, w)


def lookback_run(monkeypatch, p, g, B, kernel, tag, section="lookbacks"):
    if kernel is not None:
        fast_kernels(monkeypatch, kernel)
    rec = ec.stream(p, g, B)
    info = run_case(p, rec, tag, section)
    if kernel is not None:
        ran_the_fast_kernels(info, kernel, p, tag)
    # Initialise filled the windows and the books stepped: (nearly) every book took most of the steps asked for
    assert info["cut"] or info["env_steps"] > 0, (tag, info)
    return info


@pytest.mark.parametrize("i", range(ec.N_LOOKBACK))
def test_lookback_sweep(monkeypatch, i):
    p, g, B, kernel = ec.lookback_case(i)
    lookback_run(monkeypatch, p, g, B, kernel, "look-backs case %d %s (%s)" % (i, [getattr(p, n) for n in ec.LOOKBACKS], kernel or "private theta"),
                 section="lookback_sweep")


@pytest.mark.parametrize("kernel", KERNELS + [None])
def test_all_eight_lookbacks_at_256(monkeypatch, kernel):
    p = params(10, 2, theta_mode=abi.THETA_SHARED if kernel else abi.THETA_PRIVATE, mem=1 << 18)
    all_lookbacks(p, 256)
    g = engine.default_gen_params()
    g.n_events = 1200
    info = lookback_run(monkeypatch, p, g, B_FAST if kernel else 3, kernel, "all look-backs 256 (%s)" % (kernel or "private theta"))
    assert info["cut"] or info["env_steps"] >= (B_FAST if kernel else 3) * STEPS     # the windows filled and every book went on stepping


@pytest.mark.parametrize("kernel", KERNELS + [None])
def test_normed_reward_over_a_pnl_window_of_256(monkeypatch, kernel):
    """REWARD_NORMED reads pnl_ups / pnl_downs, the agent's own rings of lb_pnl entries (filled by its steps, not by the pre-pass):
    zero until both are full, so the run goes on until they are and the rewards have turned non-zero."""
    p = params(5, 2, theta_mode=abi.THETA_SHARED if kernel else abi.THETA_PRIVATE, mem=1 << 18)
    p.lb_pnl, p.reward_measure = 256, abi.REWARD_NORMED
    g = engine.default_gen_params()
    g.n_events = 1200
    seen = []

    def hook(episode, step, eng, oracles):
        if step:
            seen.append(bool((oracles[0].recs()["reward"] != 0).any()))
    if kernel is not None:
        fast_kernels(monkeypatch, kernel)
    B = B_FAST if kernel else 3
    tag = "lb_pnl 256, normed (%s)" % (kernel or "private theta")
    info = run_case(p, ec.stream(p, g, B), tag, "lookbacks", episodes=1, steps=330, hook=hook)
    if kernel is not None:
        ran_the_fast_kernels(info, kernel, p, tag, steps=330)
    assert info["cut"] or (not any(seen[:200]) and any(seen[280:])), "the rings fill after 256 steps of ups and downs"


def test_snapshot_with_a_pnl_window_of_256():
    """In the manner of tests/test_gpu_snapshot.py::test_masked_restore: the slot layout holds 2 w rows of the agent's rings per
    book.  Save at step 7, run on 18 steps, restore half the books, compare those with a shadow oracle replayed to step 7 and the
    others with the main oracle, to the end of the data."""
    from tests.test_gpu_snapshot import Run
    from tests.test_gpu_vec_env import make_params
    p = make_params(5, 2, 1 << 16)
    p.lb_pnl, p.reward_measure = 256, abi.REWARD_NORMED
    r = Run(65, "dry", seed=4, p=p, n_events=800)
    m = np.random.default_rng(65).integers(0, 2, size=65).astype(np.uint8)
    r.step(7)
    r.save(0)
    r.step(18)
    r.restore(0, m)
    sh = r.shadow(7)
    parts = [(sh, m != 0), (r.orc, m == 0)]
    r.check(r.observe() | {"stepped": np.zeros(65, np.int32), "reward": np.zeros(65)}, parts, "restored")
    steps = r.run_on(parts, 0, "lb_pnl 256 masked restore", every=3, to_the_end=True)
    assert steps > 256, steps       # the rings of 256 filled after the restore
    r.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_ring_mode_resumes_windows_of_256(monkeypatch, kernel):
    """LOB_TRACK_RING=256 with a refill every 8 steps (the values of tests/test_gpu_parity.py::test_long_streams_use_a_track_ring):
    prepass_extend_kernel resumes windows that are as long as the ring itself."""
    fast_kernels(monkeypatch, kernel)
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "8")
    p = params(10, 2, mem=1 << 18)
    all_lookbacks(p, 256)
    g = engine.default_gen_params()
    g.n_events = 1200
    B = B_FAST
    rec = ec.stream(p, g, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    eng.kernel_timing(True)
    eng.reset(); orc.reset()
    step = 0
    while eng.counters()[2] > 0 and step < 1300:
        n = 1 if step < 40 or step % 5 == 0 else 4
        eng.td_step(n); orc.td_step(n)
        step += n
        if n == 1:
            compare_learner_step(eng, orc, "ring of 256, windows of 256 / %s, step %d" % (kernel, step), exact=False, rtol=1e-9)
    assert eng.counters()[2] == 0 and step > 300, step
    compare_env(eng, orc, "ring of 256: end of the episode")
    eng.sync()
    _, refills = eng.kernel_time_ms("prepass_extend_kernel")
    assert refills >= 30, refills
    n = eng.launches()
    assert n[ENV_KERNEL_OF[kernel]] > 0.9 * step, (n, step)
    np.testing.assert_allclose(eng.theta(), orc.theta(), rtol=1e-9, atol=1e-12)
    eng.close()
    orc.close()


# ---- 1d. table size -------------------------------------------------------------------------------------------------------------------
SMALL_TABLES = (1, 2, 31, 32, 33, 63, 64, 65, 4098)
TABLE_FAST = [(abi.ALGO_SARSA, "lane_per_book"), (abi.ALGO_SARSA, "sixteen_lanes"), (abi.ALGO_QLAMBDA, "lane_per_book"), (abi.ALGO_QLAMBDA, "sixteen_lanes"), (abi.ALGO_DOUBLE_Q, "lane_per_book")]


@pytest.mark.parametrize("algo,kernel", TABLE_FAST, ids=["sarsa_64", "sarsa_16", "qlambda_64", "qlambda_16", "double_q_64"])
@pytest.mark.parametrize("M", SMALL_TABLES)
def test_small_tables_through_the_fast_kernels(monkeypatch, M, algo, kernel):
    """The bitmaps over the weights (theta_nzx, theta_nzd, theta_nzm, amb_bits) have M / 32 + 1 words: one word up to M = 31, two from 32,
    three from 64.  With so few weights every tile lies on a written weight after the first update: no hit list fits a record, the
    fused env step evaluates every book in full (path statistic [6]) and the lane learn kernel hands the books back ([7])."""
    fast_kernels(monkeypatch, kernel)
    p = params(10, 2, algo, mem=M)
    tag = "M = %d algo %d / %s" % (M, algo, kernel)
    info = run_case(p, table_stream(B_FAST), tag, "table")
    ran_the_fast_kernels(info, kernel, p, tag)
    ps = info["paths"]
    print("%s: path statistics %s, flow %s" % (tag, list(ps), info["flow"]))
    if M <= 65 and not info["cut"]:
        assert ps[6] > 0, (tag, list(ps))
    if M == 1 and not info["cut"]:
        # every tile index is 0.  Read from the code (lob_tiles.h tile_register_impl): the registry's table takes ONE entry for index 0
        # on its first probe, every later tile finds it there and is ambiguous with it -- one ambiguous index ([3]), no overflow ([4]);
        # every triple's 288 tiles coincide (registry_block: mk_ident[3] = 2), so the lane trace kernel takes no book: they go to the
        # wave-per-book kernels ([0] under SARSA(lambda), [7] under Q(lambda) / double Q)
        assert ps[3] >= 1 and ps[4] == 0, (tag, list(ps))
        assert (ps[0] if algo == abi.ALGO_SARSA else ps[7]) > 0, (tag, list(ps))


@pytest.mark.parametrize("algo", [abi.ALGO_SARSA, abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q], ids=["sarsa", "qlambda", "double_q"])
@pytest.mark.parametrize("M", SMALL_TABLES)
def test_small_tables_one_book_bit_for_bit(M, algo):
    p = params(10, 2, algo, mem=M)
    run_case(p, table_stream(1), "M = %d algo %d, one book" % (M, algo), "table")


@pytest.mark.parametrize("algo", ec.BIG_ALGOS, ids=["qlambda", "double_q"])
@pytest.mark.parametrize("M", ec.BIG_TABLES, ids=["2^27-1", "2^27", "2^27+1"])
def test_tables_around_the_pair_kernel_threshold(monkeypatch, M, algo):
    """learn_q_pair_kernel packs a tile index into 27 bits of its LDS rows: plan_paths gives tables of 2^27 weights and more to
    learn_q_lane_kernel.  One GiB of weights on either side (two under double Q), every one of them drawn by learning.random_init --
    a vector without exact ties, tests/edge_cases.py big_table_case -- and all of them compared after 40 steps: no case may end
    early (tests/test_edge_cases.py has run the shadow alone over the six)."""
    fast_kernels(monkeypatch, "lane_per_book")
    p, rec = ec.big_table_case(M, algo)
    tag = "M = %d algo %d" % (M, algo)
    info = run_case(p, rec, tag, "big_tables", episodes=1, steps=40)
    assert not info["cut"], tag
    n = info["launches"]
    if M < (1 << 27):
        assert n["learn_q_pair_kernel"] == 40 and n["learn_q_lane_kernel"] == 0, (tag, n)
    else:
        assert n["learn_q_lane_kernel"] == 40 and n["learn_q_pair_kernel"] == 0, (tag, n)
    assert n["env_step_kernel"] >= 38 and n["env_step16_kernel"] == 0 and n["learn_q_fast_kernel"] == 0, (tag, n)


def test_the_largest_table():
    """M = 2^31 - 1, the last size lob_create takes: lob_tiles.h's 32-bit modular arithmetic (sums of two residues below 2^32) at its
    end.  lob_features against oracle_tiles on random and non-finite state rows; 20 learner steps of Q(lambda), two books on one
    vector: actions, TD errors, RNG counters, every book's traces (indices and eligibilities); the weights through lob_q_values on the
    visited states against the oracle's sums (the vector itself is 16 GiB and stays where it is)."""
    from tests.test_gpu_vec_act import cpu_sum
    M = (1 << 31) - 1
    p = params(10, 2, abi.ALGO_QLAMBDA, mem=M)
    p.alpha = 0.05
    B = 2
    rec = table_stream(B, 200)
    try:
        eng = engine.Engine(p, B)
    except engine.LobError as e:
        if e.code != abi.LOB_ENOMEM:
            raise
        print("the largest table: lob_create returned LOB_ENOMEM for 16 GiB of weights -- skipped")
        pytest.skip("LOB_ENOMEM: no room for 2^31 - 1 weights on this device")
    r = np.random.default_rng(231)
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_nonfinite.npz"))
    rows = np.concatenate([np.ascontiguousarray(fx["vars"], np.float32), r.normal(0.0, 8.0, size=(300, 8)).astype(np.float32),
                           r.uniform(-3000.0, 3000.0, size=(100, 8)).astype(np.float32)])
    assert p.n_vars == 8 and rows.shape[1] == 8
    want = np.zeros((rows.shape[0], 9, 96), np.int32)
    ol.load().oracle_tiles(M, ol.ptr(rows), 8, rows.shape[0], ol.ptr(want))
    assert want.min() >= 0 and want.max() > (1 << 30)
    np.testing.assert_array_equal(eng.features(rows), want)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    eng.reset(); orc.reset()
    visited = []
    for step in range(20):
        eng.td_step(1); orc.td_step(1)
        compare_learner_step(eng, orc, "M = 2^31 - 1, step %d" % step, exact=False, rtol=1e-9)
        for b in range(B):
            ei, ee = eng.traces(b)
            oi, oe = orc.traces(b)
            order_e, order_o = np.argsort(ei, kind="stable"), np.argsort(oi, kind="stable")
            np.testing.assert_array_equal(ei[order_e], oi[order_o], err_msg="trace indices, book %d step %d" % (b, step))
            np.testing.assert_array_equal(ee[order_e], oe[order_o], err_msg="eligibilities, book %d step %d" % (b, step))
        visited.append(orc.recs()["vars"][:, :8].copy())
    obs = np.ascontiguousarray(np.concatenate(visited), np.float32)
    q_want = cpu_sum(p, obs, orc.theta())
    assert np.count_nonzero(q_want) > 0, "the visited states' values have moved"
    np.testing.assert_allclose(eng.q_values(obs), q_want, rtol=1e-9, atol=1e-12)
    eng.close()
    orc.close()


# ---- 1e. policy and reward --------------------------------------------------------------------------------------------------------
def note_policy_case(p, form, info):
    if info["cut"]:
        return
    SEEN["boltzmann"][form] = SEEN["boltzmann"].get(form, 0) + 1
    if p.reward_measure == abi.REWARD_MM_EXP:
        SEEN["mm_exp"][form] = SEEN["mm_exp"].get(form, 0) + 1
    SEEN["non_greedy"] += info["non_greedy"]
    SEEN["boltzmann_steps"] += info["looked"]


@pytest.mark.parametrize("i", range(ec.N_POLICY))
def test_policy_sweep_general_kernels(i):
    p, g, B = ec.policy_case(i)
    tag = "policy case %d (algo %d, reward %d, tau %g, B = %d, theta mode %d)" % (i, p.algo, p.reward_measure, p.tau, B, p.theta_mode)
    info = run_case(p, ec.stream(p, g, B), tag, "policy_general", count_non_greedy=True)
    n = info["launches"]
    assert n["env_step_kernel"] == 0 and n["env_step16_kernel"] == 0 and n["learn_q_pair_kernel"] == 0, (tag, n)
    note_policy_case(p, "general", info)


# (double Q goes with "dq_pair" alone, the other two algorithms with the other two variants)
@pytest.mark.parametrize("i,variant", [(i, v) for i in range(ec.N_POLICY) for v in ec.fast_variants(i)])
def test_policy_sweep_fast_kernels(monkeypatch, i, variant):
    p, g, B = ec.policy_case_fast(i, variant)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    kernel = "sixteen_lanes" if variant == "pair" else "lane_per_book"
    tag = "policy case %d / %s (algo %d, reward %d, tau %g, B = %d)" % (i, variant, p.algo, p.reward_measure, p.tau, B)
    info = run_case(p, ec.stream(p, g, B), tag, "policy_fast", count_non_greedy=True)
    ran_the_fast_kernels(info, kernel, p, tag)
    note_policy_case(p, kernel, info)


def test_policy_fused_action_selection_chosen_by_size():
    """1 100 books: above the 1 024 from which plan_paths puts the action selection inside the env step by itself -- no switch."""
    p, rec = ec.policy_size_case()      # (REWARD_MM_EXP; tests/test_edge_cases.py: its shadow oracle stays in step)
    tag = "policy case 9 at 1 100 books, unforced"
    info = run_case(p, rec, tag, "policy")
    n = info["launches"]
    assert not info["cut"], tag
    assert n["env_step16_kernel"] >= EPISODES * (STEPS - 2) and n["env_step_kernel"] == 0, (tag, n)


def test_zz_policy_sweep_contains_what_it_is_for():
    """(after the sweep: file order)  Boltzmann through each env-step form at least 6 times, REWARD_MM_EXP at least 3 times, and
    the oracle's Boltzmann actions are not all greedy."""
    if not SEEN["boltzmann"]:
        pytest.skip("the sweep did not run in this session")
    if os.environ.get("PYTEST_XDIST_WORKER"):
        pytest.skip("under pytest-xdist this process has seen only its share of the sweep")
    print("policy sweep: Boltzmann cases %s, MM_EXP cases %s, non-greedy actions %d of %d looked at" %
          (SEEN["boltzmann"], SEEN["mm_exp"], SEEN["non_greedy"], SEEN["boltzmann_steps"]))
    for form in ("general", "lane_per_book", "sixteen_lanes"):
        assert SEEN["boltzmann"].get(form, 0) >= 6 and SEEN["mm_exp"].get(form, 0) >= 3, (form, SEEN)
    assert SEEN["non_greedy"] > SEEN["boltzmann_steps"] // 20, SEEN


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("algo", [abi.ALGO_SARSA, abi.ALGO_QLAMBDA], ids=["sarsa", "qlambda"])
def test_set_tau(monkeypatch, algo, kernel):
    """lob_set_tau beside oracle_set_tau: halved in the middle of the first episode and again between the episodes; a zero and a
    negative temperature are refused (LOB_EINVAL) and leave the run as it was."""
    fast_kernels(monkeypatch, kernel)
    p = params(10, 2, algo, mem=1 << 18)
    p.policy, p.tau = abi.POLICY_BOLTZMANN, 20.0
    lib = ol.load()

    def hook(episode, step, eng, oracles):
        if (episode, step) in ((0, 30), (1, 0)):
            tau = 10.0 if episode == 0 else 5.0
            eng.set_tau(tau)
            for o in oracles:
                lib.oracle_set_tau(o.h, C.c_double(tau))
        if (episode, step) in ((0, 10), (0, 45)):
            for bad in (0.0, -1.0):
                with pytest.raises(engine.LobError) as err:
                    eng.set_tau(bad)
                assert err.value.code == abi.LOB_EINVAL
    tag = "set_tau, algo %d / %s" % (algo, kernel)
    info = run_case(p, table_stream(B_FAST), tag, "policy", hook=hook, count_non_greedy=True)
    ran_the_fast_kernels(info, kernel, p, tag)
    assert not info["cut"] and info["non_greedy"] > 0, (tag, info)


# ---- the shadow oracle's count ----------------------------------------------------------------------------------------------------
def test_zz_report_cases_cut_short():
    """(after everything: file order)  Per section: how many shared-theta cases the shadow oracle ended early.  In the two sweeps
    (look-backs; policy / reward through the general and through the fast kernels) at most one in ten of the sweep's own
    shared-theta cases: the cap of tests/test_gpu_steady.py, which tests/test_edge_cases.py has held on the CPU for the same
    cases; none of the tables of 2^27 weights; the other fixed-shape sections are reported."""
    lines = ["edges, %s: %d of %d shared-theta cases cut short by the shadow oracle%s" % (s, len(CUT[s]), RAN[s], (": " + "; ".join(CUT[s])) if CUT[s] else "")
             for s in SECTIONS]
    print("\n".join(lines))
    for s in ("lookback_sweep", "policy_general", "policy_fast"):
        assert len(CUT[s]) <= RAN[s] // 10, lines
    assert not CUT["big_tables"], lines
