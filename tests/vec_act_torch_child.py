"""Child process of tests/test_gpu_vec_act.py::test_vec_env_act_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  70 books,
SARSA on learning.random_init weights shared by all books, the streams of tests/test_gpu_vec_act.py: env.step(env.act()) until no
book is live -- the engine's own greedy policy with no host in the loop but the n_live read --, then env.q_values() of the final
observation.  What was seen goes to the .npz named on the command line; the parent compares it with the oracle.  A VecEnv that never
calls act() has allocated and launched nothing for it."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402
from tests.test_gpu_vec_act import make_params, streams  # noqa: E402

B = 70


def main(out_path):
    p = make_params(abi.ALGO_SARSA, abi.THETA_SHARED, random_init=1)
    eng = engine.Engine(p, B)
    eng.load_events(streams(p, B))
    eng.kernel_timing(True)
    env = VecEnv(eng)
    obs = env.reset()
    assert env.act_out is None and env.act_actions is None and env.act_q is None, "nothing is allocated before the first act()"
    for bad in ("softmax", 0):
        try:
            env.act(bad)
            raise AssertionError("VecEnv.act accepted mode %r" % (bad,))
        except ValueError:
            pass
    for bad in (obs.double(), obs[:, :4], obs.cpu(), obs.t()):
        try:
            env.q_values(bad)
            raise AssertionError("VecEnv.q_values accepted a tensor of dtype %s, shape %s" % (bad.dtype, tuple(bad.shape)))
        except ValueError:
            pass
    eng.sync()
    assert eng.kernel_time_ms("vec_act_kernel")[1] == 0 and eng.kernel_time_ms("vec_q_kernel")[1] == 0
    actions, stepped = [], []
    while int(env.n_live) > 0:
        assert len(actions) < 300, "the episode did not end"
        a = env.act()
        assert a is env.act_actions and a.dtype == torch.int32 and a.shape == (B,) and a.is_cuda
        assert env.act_q.dtype == torch.float64 and env.act_q.shape == (B, abi.LOB_N_ACTIONS)
        obs, reward, terminal, st = env.step(a)
        actions.append(a.clone())
        stepped.append(st.clone())
    assert env.status() == abi.LOB_OK and env.bad_actions == 0
    final = obs.clone()
    q = env.q_values(final)
    assert q.dtype == torch.float64 and q.shape == (B, abi.LOB_N_ACTIONS) and q.is_cuda
    a = env.act("argmax")
    assert (a == 0).all(), "every book is over: action 0"
    assert (env.act("behaviour") == 0).all()
    eng.sync()
    n_steps = len(actions)
    assert eng.kernel_time_ms("vec_act_kernel")[1] == n_steps + 2 and eng.kernel_time_ms("vec_q_kernel")[1] == 1
    np.savez(out_path, actions=torch.stack(actions).cpu().numpy(), stepped=torch.stack(stepped).cpu().numpy(),
             books=np.frombuffer(bytes(eng.get_books()), dtype=np.uint8), obs=final.cpu().numpy(), q_values=q.cpu().numpy(),
             act_q=env.act_q.cpu().numpy())
    eng.close()
    print("vec act OK: %d books x %d steps" % (B, n_steps))


if __name__ == "__main__":
    main(sys.argv[1])
