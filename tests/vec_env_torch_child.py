"""Child process of tests/test_gpu_vec_env.py::test_closed_loop_through_torch_with_no_host_in_it (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  256 books,
120 steps through VecEnv; the action is an exact function of the previous observation, computed by torch on the device -- the
bits of obs[:, 0] shifted and xor-folded with those of obs[:, 1], mod 9 -- and the oracle is driven by the same function in
numpy on its own vars.  Inside the loop nothing reads the device and nothing waits: a wrong stream order between torch and the
engine, or an output that lags a step, gives other actions than the oracle's and the books part ways."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402
from tests import oracle_lib as ol  # noqa: E402
from tests.parity import compare_env  # noqa: E402

B, STEPS = 256, 120


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


def policy_numpy(vars_):
    bits = np.ascontiguousarray(vars_[:, :2], np.float32).view(np.int32)
    return np.mod((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5), 9).astype(np.int32)   # (np.mod and torch.remainder: the sign of the divisor)


def main():
    p = engine.default_params()
    p.depth, p.max_trades = 10, 2
    p.theta_mode, p.memory_size = abi.THETA_PRIVATE, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 500
    rec = engine.gen_stream_host(g, p.depth, p.max_trades, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    env = VecEnv(eng)
    obs = env.reset()
    orc.reset()
    kept = []
    for step in range(STEPS):     # no .cpu(), .item(), lob_sync or status() in here
        actions = policy_torch(obs)
        obs, reward, terminal, stepped = env.step(actions)
        if step % 40 == 39:
            kept.append((step, actions.clone(), obs.clone(), stepped.clone()))
    o_actions = {}
    for step in range(STEPS):
        a = policy_numpy(orc.recs()["vars"])
        orc.env_step(a)
        if step % 40 == 39:
            o_actions[step] = (a, orc.recs()["vars"][:, :eng.V].copy())
    assert env.status() == abi.LOB_OK and env.bad_actions == 0
    recs = orc.recs()
    compare_env(eng, orc, "closed loop, %d steps" % STEPS)
    np.testing.assert_array_equal(obs.cpu().numpy(), recs["vars"][:, :eng.V], err_msg="final obs")
    st = stepped.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(reward.cpu().numpy()[st], recs["reward"][st], err_msg="final reward")
    assert (reward.cpu().numpy()[~st] == 0.0).all()
    np.testing.assert_array_equal(terminal.cpu().numpy(), recs["book"]["terminal"], err_msg="final terminal")
    np.testing.assert_array_equal(terminal.cpu().numpy(), eng.get_terminal())
    assert int(env.n_live.item()) == int((recs["book"]["terminal"] == 0).sum())
    for step, a, o, s in kept:      # (clones taken in stream order inside the loop: the outputs of THAT step)
        np.testing.assert_array_equal(a.cpu().numpy(), o_actions[step][0], err_msg="actions of step %d" % step)
        np.testing.assert_array_equal(o.cpu().numpy(), o_actions[step][1], err_msg="obs of step %d" % step)
    c, oc = eng.counters(), orc.counters()
    assert c[0] == oc[0] and c[1] == oc[1] and oc[0] > B * STEPS // 2, (c, oc)
    eng.close()
    orc.close()
    print("closed loop OK: %d books x %d steps, %d env steps" % (B, STEPS, oc[0]))


if __name__ == "__main__":
    main()
