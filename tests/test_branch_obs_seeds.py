"""The seeds of tests/test_gpu_branch_obs.py::test_against_the_real_steps, replayed through the oracle on the CPU: for every shape
of tests/branch_obs_cases.py the scripted real steps and per-branch plans lead to what that test asserts its comparison has covered --
two branches of one book at different records, a window longer than the events consumed, a live own order on either side, a non-zero
position -- so the GPU test's assertion is one the streams can meet, shown without the code under test.  CPU only."""
import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import oracle_lib as ol
from tests.branch_obs_cases import H, N_EVENTS, SHAPES, reached, script
from tests.test_gpu_vec_env import gen, make_params


@pytest.mark.parametrize("B,depth,trades,N,K", SHAPES)
def test_the_chosen_seeds_reach_what_the_gpu_test_asserts(B, depth, trades, N, K):
    p = make_params(depth, trades)
    rec = engine.gen_stream_host(gen(N_EVENTS, "dry", p), p.depth, p.max_trades, 0, B)
    pre, plans = script(B, N)
    cur = np.zeros((N, H, B), np.int32)
    n_valid = np.zeros((N, H, B), np.int32)
    own = np.zeros((N, H, B, abi.VEC_OWN_WORDS), np.float32)
    for n in range(N):
        o = ol.Oracle(p, rec)
        o.reset()
        for a in pre:
            o.env_step(a)
        for h in range(H):
            o.env_step(plans[n, h])
            book = o.recs()["book"]
            # the record behind the current snapshot: cursor - 1 (include/lob_engine.h lob_vec_hist_out), the stream's last one when dry
            r = np.minimum(book["cursor"] - 1, N_EVENTS - 1)
            cur[n, h], n_valid[n, h] = r, np.minimum(K, r + 1)
            for i, f in enumerate(abi.OWN_FIELDS):
                own[n, h, :, i] = book[f].astype(np.float32)
        o.close()
    assert reached(cur, n_valid, own, N, K) == []
