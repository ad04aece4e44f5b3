"""Child process of tests/test_gpu_vec_book.py::test_vec_env_with_the_book_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  300 books,
depth 5, 20 steps of a random policy made by torch on the device through VecEnv(eng, book=True): after every step the three book
tensors are cloned (in stream order) and the engine's dump is taken; at the end every clone must be that dump, converted to f32.
Then a VecEnv without the flag: it has no book tensors and launches nothing new."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402
from tests.parity import dumps_to_np  # noqa: E402

B, D, STEPS = 300, 5, 20


def make_engine():
    p = engine.default_params()
    p.depth, p.max_trades = D, 2
    p.theta_mode, p.memory_size = abi.THETA_PRIVATE, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 200
    eng = engine.Engine(p, B)
    eng.load_events(engine.gen_stream_host(g, D, 2, 0, B))
    eng.kernel_timing(True)
    return eng


def expected(dump):
    lv = np.stack([dump["ask_px"][:, :D], dump["ask_vol"][:, :D], dump["bid_px"][:, :D], dump["bid_vol"][:, :D]], axis=1).astype(np.float32)
    own = np.stack([dump[f].astype(np.float32) for f in abi.OWN_FIELDS], axis=1)
    return lv, own, dump["time_ms"].astype(np.int64)


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    eng = make_engine()
    env = VecEnv(eng, book=True)
    assert env.levels.shape == (B, 4, D) and env.levels.dtype == torch.float32 and env.levels.is_cuda
    assert env.own.shape == (B, 16) and env.own.dtype == torch.float32 and env.time_ms.shape == (B,) and env.time_ms.dtype == torch.int64
    obs = env.reset()
    kept = [("reset", env.levels.clone(), env.own.clone(), env.time_ms.clone(), dumps_to_np(eng.get_books()).copy())]
    for step in range(STEPS):
        actions = torch.randint(0, abi.LOB_N_ACTIONS, (B,), generator=gen, device="cuda", dtype=torch.int32)
        ret = env.step(actions)
        assert len(ret) == 4 and ret[0] is env.obs, "step() keeps its return value; the book tensors are attributes"
        kept.append(("step %d" % step, env.levels.clone(), env.own.clone(), env.time_ms.clone(), dumps_to_np(eng.get_books()).copy()))
    eng.clear_inventory()
    env.observe()
    kept.append(("observe", env.levels.clone(), env.own.clone(), env.time_ms.clone(), dumps_to_np(eng.get_books()).copy()))
    assert env.status() == abi.LOB_OK and env.bad_actions == 0
    for tag, lv, own, tm, dump in kept:
        e_lv, e_own, e_tm = expected(dump)
        np.testing.assert_array_equal(lv.cpu().numpy(), e_lv, err_msg=tag + ": levels")
        np.testing.assert_array_equal(own.cpu().numpy(), e_own, err_msg=tag + ": own")
        np.testing.assert_array_equal(tm.cpu().numpy(), e_tm, err_msg=tag + ": time_ms")
    assert (kept[-1][2].cpu().numpy()[:, abi.OWN_TOTAL_TICKS] > 0).all()
    _, n = eng.kernel_time_ms("vec_book_kernel")
    assert n == STEPS + 2, n
    eng.close()

    eng = make_engine()
    env = VecEnv(eng)
    assert env.book_out is None and not hasattr(env, "levels") and not hasattr(env, "own") and not hasattr(env, "time_ms")
    env.reset()
    for step in range(5):
        env.step(torch.randint(0, abi.LOB_N_ACTIONS, (B,), generator=gen, device="cuda", dtype=torch.int32))
    assert env.status() == abi.LOB_OK
    _, n_obs = eng.kernel_time_ms("vec_observe_kernel")
    _, n = eng.kernel_time_ms("vec_book_kernel")
    assert n_obs == 5 and n == 0, (n_obs, n)
    eng.close()
    print("vec book OK: %d books x %d steps" % (B, STEPS))


if __name__ == "__main__":
    main()
