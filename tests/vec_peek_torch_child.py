"""Child process of tests/test_gpu_vec_peek.py::test_vec_env_peek_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  130 books,
depth 5, two trade slots, a random policy made by torch on the device through VecEnv.
  1. peek(): shapes, dtypes and device of the four persistent tensors; nothing of the environment moved.
  2. every plane against step() on a cloned path: save(0), step(full(a)), clone, restore(0), for each of the nine actions, at several
     points of the episode and with books that are over.
  3. peek(actions=[...]) writes the planes asked for and leaves the others as they were; bad action lists raise ValueError.
  4. the expectimax recipe of the docstring runs and gives finite targets of shape [9, B].
  5. a VecEnv that never peeks has no peek tensors and launches nothing for it."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402

B, D, T, N = 130, 5, 2, abi.LOB_N_ACTIONS


def make_engine():
    p = engine.default_params()
    p.depth, p.max_trades = D, T
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_PRIVATE, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 160
    rec = engine.gen_stream_host(g, D, T, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    eng.kernel_timing(True)
    return eng


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    eng = make_engine()
    env = VecEnv(eng)
    V = env.V
    assert env.peek_obs is None and env.peek_out is None
    env.reset()

    def random_step():
        env.step(torch.randint(0, N, (B,), generator=gen, device="cuda", dtype=torch.int32))

    checked = with_over = 0
    steps = 0
    while int(env.n_live) > 0:
        if steps % 9 == 2 or (int(env.n_live) < B and steps % 2 == 0):
            books = bytes(eng.get_books())
            o, r, t, s = env.peek()
            assert bytes(eng.get_books()) == books, "peek() moved the books"
            assert o is env.peek_obs and r is env.peek_reward and t is env.peek_terminal and s is env.peek_stepped
            assert (o.shape, o.dtype) == ((N, B, V), torch.float32) and (r.shape, r.dtype) == ((N, B), torch.float64)
            assert (t.shape, t.dtype) == ((N, B), torch.uint8) and (s.shape, s.dtype) == ((N, B), torch.int32)
            assert all(x.device == env.device and x.is_contiguous() for x in (o, r, t, s))
            o, r, t, s = o.clone(), r.clone(), t.clone(), s.clone()
            over = env.terminal != 0
            env.save(0)
            for a in range(N):
                so, sr, st, ss = env.step(torch.full((B,), a, device="cuda", dtype=torch.int32))
                assert torch.equal(o[a], so) and torch.equal(t[a], st) and torch.equal(s[a], ss), "step %d action %d" % (steps, a)
                assert torch.equal(r[a].view(torch.int64), sr.view(torch.int64)), "step %d action %d: reward" % (steps, a)
                env.restore(0)
            assert not bool(s[:, over].any()) and bool((r[:, over] == 0).all())
            checked += 1
            with_over += int(bool(over.any()))
        random_step()
        steps += 1
        assert steps < 1000
    assert checked >= 5 and with_over >= 1, (checked, with_over)

    # 3. a list of actions; what is refused
    env.reset()
    for _ in range(5):
        random_step()
    o, r, t, s = [x.clone() for x in env.peek()]
    for x in (env.peek_obs, env.peek_reward, env.peek_terminal, env.peek_stepped):
        x.fill_(7)
    env.peek(actions=[8, 0, 3])
    for a in range(N):
        if a in (0, 3, 8):
            assert torch.equal(env.peek_obs[a], o[a]) and torch.equal(env.peek_reward[a], r[a]) and torch.equal(env.peek_terminal[a], t[a]) and torch.equal(env.peek_stepped[a], s[a])
        else:
            assert bool((env.peek_obs[a] == 7).all()) and bool((env.peek_reward[a] == 7).all()) and bool((env.peek_terminal[a] == 7).all()) and bool((env.peek_stepped[a] == 7).all())
    for bad in ([9], [-1], [], [1.5], [0, 12]):
        try:
            env.peek(actions=bad)
        except ValueError:
            pass
        else:
            raise AssertionError("VecEnv.peek accepted %r" % (bad,))

    # 4. the expectimax recipe
    gamma = 0.97
    o, r, t, s = env.peek()
    q = env.q_values(o.view(9 * B, V)).view(9, B, 9).max(-1).values
    target = r + gamma * q * (t == 0)
    assert target.shape == (N, B) and target.dtype == torch.float64 and bool(torch.isfinite(target).all())
    assert env.status() == abi.LOB_OK
    _, n_peek = eng.kernel_time_ms("vec_peek_kernel")
    assert n_peek == checked + 3, (n_peek, checked)
    eng.close()

    # 5. a VecEnv that never peeks
    eng = make_engine()
    env = VecEnv(eng)
    env.reset()
    for _ in range(5):
        random_step()
    assert env.status() == abi.LOB_OK
    assert env.peek_obs is None and env.peek_reward is None and env.peek_terminal is None and env.peek_stepped is None and env.peek_out is None
    _, n_peek = eng.kernel_time_ms("vec_peek_kernel")
    assert n_peek == 0, n_peek
    eng.close()
    print("peek OK: %d books, %d points of the episode against step(), the expectimax recipe" % (B, checked))


if __name__ == "__main__":
    main()
