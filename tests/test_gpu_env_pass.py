"""The fused env step's event pass against the oracle, where its wave-uniform skips can go wrong.

pass_fast (rl_markets_amd/csrc/lob_env.h) skips the trade blocks, a side's row scan with its UpdateOrder, and the
adverse-selection block when NO lane still in the event loop needs them (each is, by its own select form, a no-op for a
lane without a trade / without that side's order / without a crossed order).  That must leave every result as it was:
the engine is run against tests/oracle_lib step by step -- books and state variables bit for bit, TD errors as
tests/test_gpu_steady.py compares them under one shared weight vector -- on streams chosen for what the pass then does
differently:

  sparse     move_prob 0.05: long steps, waves that run many passes with few books left, the stream running dry;
  dense      move_prob 1: every pass ends its step;
  no_trades  trade_prob 0: the trade blocks are skipped by every wave, always;
  two_trades trade_prob 1, trade2_prob 1: never;
  depth3     three levels: the depth mask of the row scan;
  one_sided  pos_ub = order_size: an order is switched off at almost every step (a side's scan skipped, its volume read as 0);
  above_2048 prices of 2 300 - 2 700, where neighbouring f32 are more than 1e-4 apart: the decimal an order is quoted at
             and the f32 a level carries can have different 1e-4 keys, so an order often finds no level to rest at.

200 books are three full waves and a partial one of the lane-per-book kernel (LOB_ENV16_MAX=0: what the headline batch
runs), or 50 waves of the kernel that spreads a book's levels over 16 lanes (what a batch of this size runs by itself)."""
import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import oracle_lib as ol
from tests.parity import compare_learner_step
from tests.test_gpu_steady import light_books

pytestmark = pytest.mark.gpu

B, N_EVENTS, EPISODES, STEPS = 200, 400, 2, 60


def q16(prob):
    return min(65535, int(prob * 65536))


def _sparse(p, g):
    g.move_prob_q16 = q16(0.05)


def _dense(p, g):
    g.move_prob_q16 = q16(1.0)


def _no_trades(p, g):
    g.trade_prob_q16 = 0


def _two_trades(p, g):
    g.trade_prob_q16 = q16(1.0)
    g.trade2_prob_q16 = q16(1.0)


def _depth3(p, g):
    p.depth = 3


def _one_sided(p, g):
    p.pos_ub = p.order_size
    p.pos_lb = -p.order_size


def _above_2048(p, g):
    g.start_ticks, g.min_ticks, g.max_ticks = 25000, 23000, 27000   # 2 500.0 on the 0.1 grid


CASES = {"sparse": _sparse, "dense": _dense, "no_trades": _no_trades, "two_trades": _two_trades, "depth3": _depth3,
         "one_sided": _one_sided, "above_2048": _above_2048}


@pytest.mark.parametrize("kernel", ["lane_per_book", "sixteen_lanes"])
@pytest.mark.parametrize("case", list(CASES))
def test_event_pass_against_the_oracle(monkeypatch, case, kernel):
    # the fused env step and the lane learner kernels, which a batch of 200 would not select by its size
    for k, v in {"LOB_Q_LANES": "1", "LOB_Q_PAIR": "1", "LOB_FUSE_ACT": "1"}.items():
        monkeypatch.setenv(k, v)
    if kernel == "lane_per_book":
        monkeypatch.setenv("LOB_ENV16_MAX", "0")
    p = engine.default_params()
    p.depth, p.max_trades = 10, 2
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_SHARED, 1 << 20
    g = engine.default_gen_params()
    g.n_events = N_EVENTS
    CASES[case](p, g)
    rec = engine.gen_stream_host(g, p.depth, p.max_trades, 0, B)
    if case == "above_2048":
        px = rec[:, :, 2:2 + p.depth].view(np.float32)
        assert px.min() > 2048.0
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    light0 = light_books(eng)
    for episode in range(EPISODES):
        eng.reset(); orc.reset()
        for step in range(STEPS):
            eng.td_step(1); orc.td_step(1)
            compare_learner_step(eng, orc, "%s / %s, episode %d step %d" % (case, kernel, episode, step), exact=False, rtol=1e-9)
        eng.clear_inventory(); orc.clear_inventory()
        eng.handle_terminal(); orc.handle_terminal()
    # the fused env step was the kernel running: the books' actions came from their hit lists
    assert light_books(eng) - light0 > 0
    np.testing.assert_allclose(eng.theta(), orc.theta(), rtol=1e-9, atol=1e-12)
    eng.close()
    orc.close()
