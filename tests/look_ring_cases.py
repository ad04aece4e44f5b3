"""What tests/test_gpu_look_ring.py and its CPU backing tests/test_look_ring_cases.py share: the parameters, the records and the seeds
of the look-aheads on a ring-mode stream (include/lob_engine.h lob_look_ring).  No GPU is touched here.

The shapes are the smallest at which the ring can go wrong: a ring of 256 entries refilled every 16 steps, streams of 1 200 records so
that the books run out of data inside a test, 64 books (whole blocks) and 70 (a partial last one), depth 10 with two trade slots
(the fast pass) and depth 4 with three (the general loop), one configuration with the NORMED reward and lb_pnl = 3."""
import numpy as np

from rl_markets_amd import abi, engine

RING, REFILL = 256, 16
REACH = RING - abi.TRACK_WINDOW_MARGIN    # entries between the cursor and the window's end right behind a refill
N_EVENTS = 1200
N = abi.LOB_N_ACTIONS
K_HIST = 8
SHORT, LONG = (9, 4), (3, 64)             # (plans, steps) of the two roll-outs
SEED = 7
WALL_BUDGET = REACH + 8                   # branch steps of test 5: every completed step consumes at least one entry
# (B, depth, trades, normed)
CONFIGS = [(64, 10, 2, False), (70, 4, 3, False), (70, 10, 2, True)]


def make_params(depth, trades, normed=False):
    p = engine.default_params()
    p.depth, p.max_trades = depth, trades
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_PRIVATE, 1 << 16
    if normed:
        p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, 3
    return p


def gen(p, session_after=None, move_div=1):
    """session_after: the session's last half hour begins that many events into the stream (terminal 1 in the middle of the data);
    move_div: the midprice moves that many times less often, so a step consumes that many times more events."""
    g = engine.default_gen_params()
    g.n_events = N_EVENTS
    if session_after is not None:
        g.t0_ms = int(p.market.close_ms - 30 * 60000 - session_after * g.dt_ms)
    g.move_prob_q16 = max(1, g.move_prob_q16 // move_div)
    g.spread2_prob_q16 = max(1, g.spread2_prob_q16 // move_div)   # (a spread of two ticks moves the midprice as well)
    return g


def records(p, B, mixed=True, move_div=1):
    """[B][N_EVENTS][W]: the books of a stream that runs dry; with `mixed`, the last quarter of the books on a clock that reaches the
    session's last half hour 1 000 events in -- deep in ring mode, behind the last refill that finds anything to fill."""
    n_late = B // 4 if mixed else 0
    rec = engine.gen_stream_host(gen(p, move_div=move_div), p.depth, p.max_trades, 0, B - n_late)
    if n_late:
        late = engine.gen_stream_host(gen(p, session_after=1000, move_div=move_div), p.depth, p.max_trades, B - n_late, n_late)
        rec = np.concatenate([rec, late], axis=0)
    return np.ascontiguousarray(rec)


def step_rng(B, seed=SEED):
    return np.random.default_rng(1000 * B + seed)


def look_rng(B, seed=SEED):
    return np.random.default_rng(77000 + 1000 * B + seed)


def long_plans(rng, B):
    """(3, 64) plans padded with -1: plan p plays 64 - 20 * p steps."""
    P, H = LONG
    plans = rng.integers(0, N, size=(P, H, B)).astype(np.int32)
    for q in range(P):
        plans[q, H - 20 * q:, :] = -1
    return plans


DAY_LENGTHS = (150, 400, 900)             # the day library of test 6: a day shorter than the ring beside two longer ones


def make_days(depth, trades, lengths=DAY_LENGTHS, first_id=1000):
    """Synthetic days of the given lengths, each from its own generator book id (tests/test_gpu_days.py make_days)."""
    out = []
    for i, n in enumerate(lengths):
        g = engine.default_gen_params()
        g.n_events = int(n)
        out.append(engine.gen_stream_host(g, depth, trades, first_id + i, 1)[0])
    return out
