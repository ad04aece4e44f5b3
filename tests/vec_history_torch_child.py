"""Child process of tests/test_gpu_vec_history.py::test_vec_env_with_the_history_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  300 books,
depth 5, two trade slots, 20 steps of a random policy made by torch on the device through VecEnv(eng, history=16): after every step
the five history tensors are cloned (in stream order) and the engine's dump is taken; at the end every clone must be what
tests/vec_history_expected.py makes of the host records and the cloned `rec`, and `rec` must be the dump's cursor - 1.  Then
VecEnv(eng, history=16, book=True): the newest slot is the book.  Then a VecEnv without the option: no tensors, nothing new launched."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402
from tests.parity import dumps_to_np  # noqa: E402
from tests.vec_history_expected import NAMES, assert_record_has_dump_levels, expected_history  # noqa: E402

B, D, T, K, STEPS = 300, 5, 2, 16, 20
ATTRS = ("hist_levels", "hist_trades", "hist_time_ms", "hist_valid", "hist_rec")


def make_engine():
    p = engine.default_params()
    p.depth, p.max_trades = D, T
    p.theta_mode, p.memory_size = abi.THETA_PRIVATE, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 200
    rec = engine.gen_stream_host(g, D, T, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    eng.kernel_timing(True)
    return eng, rec


def snapshot(tag, env, eng):
    return (tag, [getattr(env, a).clone() for a in ATTRS], dumps_to_np(eng.get_books()).copy())


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    eng, rec = make_engine()
    flat, start = rec.reshape(-1, rec.shape[-1]), np.arange(B, dtype=np.int64) * rec.shape[1]
    env = VecEnv(eng, history=K)
    assert env.hist_levels.shape == (B, K, 4, D) and env.hist_levels.dtype == torch.float32 and env.hist_levels.is_cuda
    assert env.hist_trades.shape == (B, K, 2, T) and env.hist_trades.dtype == torch.float32
    assert env.hist_time_ms.shape == (B, K) and env.hist_time_ms.dtype == torch.int32
    assert env.hist_valid.shape == (B,) and env.hist_valid.dtype == torch.int32 and env.hist_rec.shape == (B,) and env.hist_rec.dtype == torch.int32
    assert env.book_out is None and not hasattr(env, "levels"), "the two options are independent"
    env.reset()
    kept = [snapshot("reset", env, eng)]
    for step in range(STEPS):
        actions = torch.randint(0, abi.LOB_N_ACTIONS, (B,), generator=gen, device="cuda", dtype=torch.int32)
        ret = env.step(actions)
        assert len(ret) == 4 and ret[0] is env.obs, "step() keeps its return value; the history tensors are attributes"
        kept.append(snapshot("step %d" % step, env, eng))
    eng.clear_inventory()
    env.observe()
    kept.append(snapshot("observe", env, eng))
    assert env.status() == abi.LOB_OK and env.bad_actions == 0
    for tag, tensors, dump in kept:
        got = dict(zip(NAMES, [t.cpu().numpy() for t in tensors]))
        r = got["rec"]
        assert (dump["terminal"] != 2).all(), "a condition on the inputs"
        np.testing.assert_array_equal(r, dump["cursor"] - 1, err_msg=tag + ": rec against cursor - 1")
        assert_record_has_dump_levels(flat, start, r, dump, D, tag)
        exp = expected_history(flat, start, rec.shape[1], r, K, D, T)
        for name in NAMES:
            np.testing.assert_array_equal(got[name], exp[name], err_msg="%s: %s" % (tag, name))
    assert not np.array_equal(kept[0][1][4].cpu().numpy(), kept[-1][1][4].cpu().numpy()), "the books moved"
    _, n = eng.kernel_time_ms("vec_hist_kernel")
    _, n_book = eng.kernel_time_ms("vec_book_kernel")
    assert n == STEPS + 2 and n_book == 0, (n, n_book)
    eng.close()

    eng, rec = make_engine()
    env = VecEnv(eng, history=K, book=True)
    env.reset()
    assert torch.equal(env.hist_levels[:, -1], env.levels), "after reset: the newest slot is the book"
    for step in range(8):
        env.step(torch.randint(0, abi.LOB_N_ACTIONS, (B,), generator=gen, device="cuda", dtype=torch.int32))
        assert torch.equal(env.hist_levels[:, -1], env.levels), "step %d: the newest slot is the book" % step
    assert env.status() == abi.LOB_OK
    _, n = eng.kernel_time_ms("vec_hist_kernel")
    _, n_book = eng.kernel_time_ms("vec_book_kernel")
    assert n == 9 and n_book == 9, (n, n_book)
    eng.close()

    eng, rec = make_engine()
    env = VecEnv(eng)
    assert env.hist_out is None and env.history == 0 and not any(hasattr(env, a) for a in ATTRS)
    env.reset()
    for step in range(5):
        env.step(torch.randint(0, abi.LOB_N_ACTIONS, (B,), generator=gen, device="cuda", dtype=torch.int32))
    assert env.status() == abi.LOB_OK
    _, n_obs = eng.kernel_time_ms("vec_observe_kernel")
    _, n = eng.kernel_time_ms("vec_hist_kernel")
    assert n_obs == 5 and n == 0, (n_obs, n)
    eng.close()
    print("vec history OK: %d books x %d steps, K = %d" % (B, STEPS, K))


if __name__ == "__main__":
    main()
