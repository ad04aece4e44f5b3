"""TEST INFRASTRUCTURE: the case generators of tests/test_gpu_edges.py -- the edges of what lob_create accepts -- kept apart from
the GPU file so that tests/test_edge_cases.py can run the same cases on the CPU (oracle against nudged shadow oracle: the
condition on the inputs that the shared-theta sweeps rest on) and tests/test_oracle_ref_edges.py can hold the oracle against
the unmodified reference on the same draws.

Every case is a function of its index alone and is built ON TOP of tests/test_gpu_fuzz.py::random_case, which other files
import with fixed seeds and which therefore stays as it is."""
import numpy as np

from rl_markets_amd import abi, engine
from tests import oracle_lib as ol
from tests.test_gpu_fuzz import random_case

LOOKBACKS = ("lb_mpm", "lb_vlt", "lb_svl", "lb_vwap", "lb_rsi", "lb_spread", "lb_pnl", "lb_target")
LB_EDGES = (101, 128, 255, 256)          # beyond the fuzz draw's 100, up to LOB_MAX_WINDOW
KERNELS = ("lane_per_book", "sixteen_lanes")
ALL_REWARDS = (abi.REWARD_NONE, abi.REWARD_PNL, abi.REWARD_PNL_DAMPED, abi.REWARD_SPREAD, abi.REWARD_NORMED, abi.REWARD_LOVOL,
               abi.REWARD_MM_LINEAR, abi.REWARD_MM_EXP, abi.REWARD_MM_DIV)
TAUS = (0.5, 5.0, 50.0)                  # the values tests/test_oracle_ref_sweep.py pins against the reference
BETAS = (0.0, 0.005, 0.05)
FAST_ALGOS = (abi.ALGO_SARSA, abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q)

N_LOOKBACK, N_POLICY = 12, 24


def move_lookbacks(p, r):
    """Each of the eight look-backs moved, with probability 1/2, to one of LB_EDGES; otherwise it keeps its draw."""
    for name in LOOKBACKS:
        if r.integers(0, 2):
            setattr(p, name, int(r.choice(LB_EDGES)))


def lookback_case(i):
    """Case i of the look-back sweep (1c) -> (params, generator params, B, kernel form or None).  Even cases: shared theta through
    the fast kernels (T <= 2, SARSA(lambda) / Q(lambda), 130 books), the two env-step forms in turn; odd cases: private theta, three
    books, whatever algorithm and trade-slot count the fuzz draw gave.  1 200 events: Initialise fills a window of 256 and the
    episodes have rows left to step through."""
    p, g, _ = random_case(12000 + i)
    r = np.random.default_rng(12500 + i)
    move_lookbacks(p, r)
    g.n_events = 1200
    if i % 2 == 0:
        p.theta_mode = abi.THETA_SHARED
        p.algo = int(r.choice([abi.ALGO_SARSA, abi.ALGO_QLAMBDA]))
        p.max_trades = min(p.max_trades, 2)
        g.trade2_prob_q16 = g.trade2_prob_q16 if p.max_trades > 1 else 0
        return p, g, 130, KERNELS[(i // 2) % 2]
    p.theta_mode = abi.THETA_PRIVATE
    return p, g, 3, None


def policy_algo(i):
    return (i + i // 6) % 6


def fast_variants(i):
    """The variants of tests/test_gpu_steady.py VARIANTS that case i's episodic algorithm goes with."""
    return ("dq_pair",) if FAST_ALGOS[policy_algo(i) % 3] == abi.ALGO_DOUBLE_Q else ("pair", "pair_env64")


def policy_case(i):
    """Case i of the policy / reward sweep (1e) -> (params, generator params, B of the fuzz draw).  Boltzmann with tau from TAUS, the
    algorithm from all six, beta from BETAS, the reward measure from all nine (REWARD_NONE and REWARD_MM_EXP, which the fuzz draw
    leaves out, included); under MM_EXP pos_weight <= 0.2 as tests/test_oracle_ref_sweep.py draws it (exp(pos_weight * |position|)
    squared: beyond that the rewards leave the range of a double's useful digits within a few steps).  The algorithm and the
    reward measure go round their lists (the algorithm moved on by one every six cases), so that 24 cases hold every algorithm
    four times, every measure at least twice, and MM_EXP three times under algorithms whose episodic forms -- SARSA(lambda),
    Q(lambda), SARSA(lambda) -- go through both env-step forms of the fast kernels (double Q never takes the 16-lane one)."""
    p, g, B = random_case(15000 + i)
    r = np.random.default_rng(15500 + i)
    p.policy, p.tau = abi.POLICY_BOLTZMANN, float(TAUS[int(r.integers(0, 3))])
    p.algo = policy_algo(i)
    p.beta = float(BETAS[int(r.integers(0, 3))])
    p.reward_measure = int(ALL_REWARDS[(i + 7) % 9])
    if p.reward_measure == abi.REWARD_MM_EXP:
        p.pos_weight = float(np.float32(r.uniform(0.0, 0.2)))
    return p, g, B


def policy_case_fast(i, variant):
    """The same case for the fast kernels: the algorithm's episodic form (SARSA(lambda), Q(lambda), double Q: the average-reward forms
    are not served by them), one shared weight vector, T <= 2, B from {64, 130, 300}.  `variant` names the switches of
    tests/test_gpu_steady.py VARIANTS; None when the algorithm does not go with it (double Q takes "dq_pair" alone)."""
    p, g, _ = policy_case(i)
    p.algo = FAST_ALGOS[p.algo % 3]
    if (p.algo == abi.ALGO_DOUBLE_Q) != (variant == "dq_pair"):
        return None
    p.theta_mode = abi.THETA_SHARED
    p.max_trades = min(p.max_trades, 2)
    g.trade2_prob_q16 = g.trade2_prob_q16 if p.max_trades > 1 else 0
    B = (64, 130, 300)[i % 3]
    return p, g, B


def shadow_cut(p, rec, episodes=2, steps=70):
    """Oracle against a shadow oracle whose weights are nudged by 1e-13 (relative) after step 3, over the schedule of the GPU
    sweeps: -> None when the two take the same actions and draw the same random numbers throughout, else (episode, step) of
    the first difference.  What tests/test_gpu_steady.py::test_random_configuration_timed_kernels does beside the engine, alone."""
    orc, shadow = ol.Oracle(p, rec), ol.Oracle(p, rec)
    try:
        for episode in range(episodes):
            orc.reset(); shadow.reset()
            for step in range(steps):
                orc.td_step(1); shadow.td_step(1)
                if episode == 0 and step == 3:
                    th = shadow.theta()
                    th[th != 0] *= 1.0 + 1e-13
                a, b = orc.recs(), shadow.recs()
                if not np.array_equal(a["action"], b["action"]) or not np.array_equal(a["rng_ctr"], b["rng_ctr"]):
                    return episode, step
            orc.clear_inventory(); shadow.clear_inventory()
            orc.handle_terminal(); shadow.handle_terminal()
        return None
    finally:
        orc.close(); shadow.close()


def stream(p, g, B):
    return engine.gen_stream_host(g, p.depth, p.max_trades, p.book_id_offset, B)


def shared_lookback_cases():
    return [i for i in range(N_LOOKBACK) if i % 2 == 0]


def crafted_eight_keys(D=5, B=3, n_events=400, ninth=False):
    """-> (records [B, n, W] with eight trade slots, [(book, first row of the merging event, its last merged row)]).  In every book,
    at three places, four rows in a row are crossed (tests/hard_streams.py _cross: an invalid state, the event runs on through
    them); the three crossed rows behind the first and the valid row that ends the event carry two trades each at fresh prices
    a tick apart, the row after them none: the event that follows merges exactly eight distinct 1e-4 keys from four rows.
    `ninth`: in book 0's first run that last row carries one key more."""
    from tests.hard_streams import _cross
    T = 8
    g = engine.default_gen_params()
    g.n_events = n_events
    rec = np.array(engine.gen_stream_host(g, D, T, 0, B), dtype=np.uint32, copy=True)
    f = rec.view(np.float32)
    otp, otv = 2 + 4 * D, 2 + 4 * D + T
    runs = []
    for b in range(B):
        for s in (80, 140, 200):
            s += 3 * (b % 8)
            # rows s .. s + 3 crossed: row s starts an event that ends with row s + 4; the list of the event after it (first row
            # s + 5) is merged from rows s + 1 .. s + 5
            tick0 = int(round(float(f[b, s - 1, 2 + 2 * D]) * 10.0))     # the bid of the book before the run
            for i in range(s, s + 4):
                _cross(rec[b], i, D)
            rec[b, s:s + 6, otp:otv + T] = 0
            for k in range(4):
                for slot in range(2):
                    # ascending within a row, fresh from row to row: bid, bid + 1 tick, ... bid + 7 ticks
                    f[b, s + 1 + k, otp + slot] = np.float32((tick0 + 2 * k + slot) / 10.0)
                    rec[b, s + 1 + k, otv + slot] = 3 + k
            runs.append((b, s + 5, s + 5))
    if ninth:
        b, first, _ = runs[0]
        f[b, first, otp] = np.float32((int(round(float(f[b, first - 6, 2 + 2 * D]) * 10.0)) + 8) / 10.0)
        rec[b, first, otv] = 5
    return rec, runs


# ---- fixed-shape cases of tests/test_gpu_edges.py (depth, trade slots, table size) ------------------------------------------------
def params(D, T, algo=abi.ALGO_QLAMBDA, theta_mode=abi.THETA_SHARED, mem=1 << 20):
    p = engine.default_params()
    p.depth, p.max_trades = D, T
    p.algo, p.theta_mode, p.memory_size = algo, theta_mode, mem
    return p


_batches = {}


def hardened(D, T, B, dry, n_events=400, seed=None):
    """-> (records, counts): gen_stream_host's batch at depth D with T trade slots, every kind of tests/hard_streams.py applied.
    Computed once per shape, shared, read-only."""
    from tests import hard_streams as hs
    key = (D, T, B, dry, n_events, seed)
    if key not in _batches:
        g = engine.default_gen_params()
        g.n_events = n_events
        g.trade2_prob_q16 = 30000 if T > 1 else 0
        rec, counts = hs.harden(engine.gen_stream_host(g, D, T, 0, B), D, T, hs.SEED + 100 * D + T if seed is None else seed, dry=dry)
        rec.setflags(write=False)
        _batches[key] = (rec, counts)
    return _batches[key]


SLOTS = (3, 5, 6, 7, 8)
SLOT_DEPTHS = (5, 10, 7)
SLOT_ALGOS = (abi.ALGO_QLAMBDA, abi.ALGO_SARSA, abi.ALGO_DOUBLE_Q)


def slots_case(D, T):
    """-> (params, records, counts) of the shared-theta trade-slot case: 70 hardened books with a dry tail on some."""
    rec, counts = hardened(D, T, 70, dry=True)
    return params(D, T, SLOT_ALGOS[T % 3]), rec, counts


def table_stream(B, n_events=400):
    g = engine.default_gen_params()
    g.n_events = n_events
    return engine.gen_stream_host(g, 10, 2, 0, B)


BIG_TABLES = ((1 << 27) - 1, 1 << 27, (1 << 27) + 1)
BIG_ALGOS = (abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q)


def big_table_case(M, algo):
    """-> (params, records) of a case around the pair kernel's threshold: 130 books, 200 events, learning.random_init.  From an
    all-zero vector of this size hardly any two tiles share a weight, the books' symmetric first updates leave exactly equal
    non-zero Q values behind, and any rounding difference -- the shadow's nudge, the order of the engine's atomic additions --
    breaks such ties: the draws of argmax's tie-break (under Boltzmann too: Watkins's cut and the maximum go through argmax)
    differ from then on.  A dense random vector has no exact ties."""
    p = params(10, 2, algo, mem=M)
    p.random_init = 1
    return p, table_stream(130, 200)


def policy_size_case():
    """-> (params, records): policy case 9 (REWARD_MM_EXP, Boltzmann) as Q(lambda) on one shared vector at 1 100 books -- above the
    1 024 from which the action selection goes into the env step by the batch's size."""
    p, g, _ = policy_case(9)
    assert p.reward_measure == abi.REWARD_MM_EXP and p.policy == abi.POLICY_BOLTZMANN
    p.algo, p.theta_mode, p.max_trades = abi.ALGO_QLAMBDA, abi.THETA_SHARED, min(p.max_trades, 2)
    g.trade2_prob_q16 = g.trade2_prob_q16 if p.max_trades > 1 else 0
    return p, stream(p, g, 1100)
