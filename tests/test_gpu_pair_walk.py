"""learn_q_pair_kernel's walk over the per-sum action masks, against the oracle, on both sides of its overflow rule.

The kernel resolves every tiling that passed the folded map with one mask look-up (theta_nzm) and emits the tiles of the set
bits; a book with more passed tilings than LOB_QD_HCAP, or more entries than its rows hold, is handed back to the general
kernel.  Forced pair path (the kernels of the timed run, for batches that would not select them by size), 40 learner steps,
every step against the oracle: actions, rewards, learner states and RNG counters exact, TD errors and theta to 1e-9.

Which side of the rule a step is on follows from how full the table is, and the oracle alone says that: with a fraction f of
the weights written, 288 f of a group's 288 tiles (32 tilings x 9 actions) lie on one, against rows of 11 (group 1) and 14
(group 2) entries and 12 passed tilings.  After 40 steps the oracle's theta holds

    memory_size 65 536,   1 book     f = 0.014-0.018   4-5 tiles a group: the walk serves the book
    memory_size  4 099,   1 book     f = 0.04 (step 10) -> 0.23 (step 40), 11 -> 67 tiles: first the walk, then hand-backs
    memory_size  4 099, 192 books    f = 1.00 from step 10 on: every list past the capacity, every book handed back
    memory_size 65 536, 192 books    f = 0.30 (step 10) -> 0.57 (step 40), 86 -> 165 tiles: handed back as well -- 192 books
                                     write some 2 k new weights a step, so a table of 65 536 is NOT sparse for this batch

    memory_size 4 194 304, 192 books f = 0.013-0.014 (step 40), 3.7-3.9 tiles a group: the walk serves the blocks (a shape added to the
                                     issue's, so that a full 128-book block with a few hits per lane is asserted to stay on the walk)

so, through lob_get_path_stats, the single book at 65 536 and the 192 books at 4 M must have been served by the walk in most of
their steps, and the three other shapes must have handed books back (a hand-back has other causes too -- no memo record to continue from, in a book's
first steps --, which is why "most", and why the dense shapes only ask for some).
192 books = one full and one partial 128-book block; 1 book = one lane pair."""
import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import oracle_lib as ol
from tests.parity import compare_learner_step

pytestmark = pytest.mark.gpu

PAIR = {"LOB_Q_LANES": "1", "LOB_Q_PAIR": "1", "LOB_FUSE_ACT": "1"}


# (192 books at 4 M weights: the hot path's own regime -- a full and a partial block with a few hits per lane, on the walk)
@pytest.mark.parametrize("B,M", [(192, 4099), (192, 65536), (1, 4099), (1, 65536), (192, 1 << 22)])
@pytest.mark.parametrize("algo", [abi.ALGO_QLAMBDA, abi.ALGO_SARSA, abi.ALGO_DOUBLE_Q], ids=["qlambda", "sarsa", "double_q"])
def test_pair_walk_forty_steps_against_the_oracle(monkeypatch, algo, B, M):
    for k, v in PAIR.items():
        monkeypatch.setenv(k, v)
    p = engine.default_params()
    p.depth, p.max_trades = 10, 2
    p.algo, p.theta_mode, p.memory_size = algo, abi.THETA_SHARED, M
    g = engine.default_gen_params()
    g.n_events = 400
    rec = engine.gen_stream_host(g, p.depth, 2, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    eng.reset(); orc.reset()
    nv = 2 if algo == abi.ALGO_DOUBLE_Q else 1
    back0 = int(eng.path_stats()[7])
    updates = 0
    for step in range(40):
        eng.td_step(1); orc.td_step(1)
        compare_learner_step(eng, orc, "M %d, %d books, step %d" % (M, B, step), exact=False, rtol=1e-9)
        updates += int(eng.stepped().astype(bool).sum())
    np.testing.assert_allclose(eng.theta(), orc.theta(), rtol=1e-9, atol=1e-12)
    written = orc.theta() != 0
    if nv == 2:
        np.testing.assert_allclose(eng.theta(1), orc.theta_b(), rtol=1e-9, atol=1e-12)
        written |= orc.theta_b() != 0
    handed_back = int(eng.path_stats()[7]) - back0
    st = eng.fastpath_stats()
    print("M %d, %d books: %d learner updates, %d handed back by the pair kernel; the oracle's theta: %d of %d weights written (%.1f of a group's 288 tiles); "
          "engine: %d written weights, %d of %d live books without a list"
          % (M, B, updates, handed_back, np.count_nonzero(written), M, 288.0 * np.count_nonzero(written) / M, st["written_weights"],
             st["books_without_list"], st["live_books"]))
    assert updates >= 30 * B
    if (M == 65536 and B == 1) or M == 1 << 22:
        assert 288.0 * np.count_nonzero(written) / M < 8.0      # (the premise: sparse to the end, by the oracle alone)
        assert 2 * handed_back < updates, "a sparse table: most steps should have been served by the walk"
    else:
        assert 288.0 * np.count_nonzero(written) / M > 40.0     # (the premise: far past the rows' capacity)
        assert handed_back > 0, "a table this dense must overflow the walk's lists"
    eng.close()
    orc.close()
