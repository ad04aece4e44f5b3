"""Child process of tests/test_gpu_vec_rollout.py::test_vec_env_rollout_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  130 books,
depth 5, two trade slots, plans made by torch on the device through VecEnv.
  1. rollout(): shapes, dtypes and device of the five fresh tensors; nothing of the environment moved.
  2. the plans produced by a torch op right before the call and the outputs consumed right after, no synchronise between; the results
     against the composed route through VecEnv -- save(0), H x step(plans[p, h]), clones, restore(0), for each plan -- at several points
     of the episode and with books that are over; ret against the discount loop in torch.
  3. the [P, H] form is the [P, H, B] form with the same plan for every book; what raises ValueError.
  4. ten steps of the model-predictive-control recipe of the docstring.
  5. a VecEnv that never calls rollout() launches nothing for it and holds no tensor of it."""
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
    gen.manual_seed(13)
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = make_engine()
    env = VecEnv(eng)
    V = env.V
    attrs = set(vars(env))
    env.reset()

    def random_step():
        env.step(torch.randint(0, N, (B,), generator=gen, device="cuda", dtype=torch.int32))

    P, H, gamma = 3, 4, 0.97
    checked = with_over = calls = 0
    steps = 0
    while int(env.n_live) > 0:
        if steps % 9 == 2 or (int(env.n_live) < B and steps % 3 == 0):
            books = bytes(eng.get_books())
            over = env.terminal != 0
            # made right before the call, consumed right after it: the streams order the three, no synchronise in between
            plans = torch.randint(0, N, (P, H, B), generator=gen, device="cuda", dtype=torch.int32)
            o, r, t, n, ret = env.rollout(plans, gamma)
            total = r.sum(1) + ret + n + t + o.sum(2)
            calls += 1
            assert bytes(eng.get_books()) == books, "rollout() moved the books"
            assert (o.shape, o.dtype) == ((P, B, V), torch.float32) and (r.shape, r.dtype) == ((P, H, B), torch.float64)
            assert (t.shape, t.dtype) == ((P, B), torch.uint8) and (n.shape, n.dtype) == ((P, B), torch.int32)
            assert (ret.shape, ret.dtype) == ((P, B), torch.float64)
            assert all(x.device == env.device and x.is_contiguous() for x in (o, r, t, n, ret))
            env.save(0)
            for p in range(P):
                acc, d = torch.zeros(B, dtype=torch.float64, device=dev), 1.0
                cnt = torch.zeros(B, dtype=torch.int32, device=dev)
                for h in range(H):
                    so, sr, st, ss = env.step(plans[p, h].contiguous())
                    assert torch.equal(r[p, h].view(torch.int64), sr.view(torch.int64)), "step %d plan %d step %d: reward" % (steps, p, h)
                    acc = acc + d * sr
                    d = d * gamma
                    cnt = cnt + ss
                assert torch.equal(o[p], so) and torch.equal(t[p], st) and torch.equal(n[p], cnt), "step %d plan %d" % (steps, p)
                assert torch.equal(ret[p].view(torch.int64), acc.view(torch.int64)), "step %d plan %d: ret" % (steps, p)
                env.restore(0)
            assert torch.equal(total, r.sum(1) + ret + n + t + o.sum(2)), "the outputs were read before they were written"
            assert not bool(n[:, over].any()) and bool((r[:, :, over] == 0).all())
            checked += 1
            with_over += int(bool(over.any()))
        random_step()
        steps += 1
        assert steps < 1000
    assert checked >= 5 and with_over >= 1, (checked, with_over)

    # 3. one plan for every book; what is refused
    env.reset()
    for _ in range(5):
        random_step()
    short = torch.randint(0, N, (P, H), generator=gen, device="cuda", dtype=torch.int32)
    a = env.rollout(short, gamma)
    b = env.rollout(short.unsqueeze(2).expand(P, H, B).contiguous(), gamma)
    calls += 2
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    good = torch.zeros((P, H, B), device="cuda", dtype=torch.int32)
    bad = [good.long(), good.cpu(), good[:, :, :B - 1].contiguous(), good.transpose(0, 1), good[0, 0], good.unsqueeze(0),
           torch.zeros((abi.MAX_ROLLOUT_PLANS + 1, 1, B), device="cuda", dtype=torch.int32),
           torch.zeros((1, abi.MAX_ROLLOUT_STEPS + 1, B), device="cuda", dtype=torch.int32), good.cpu().numpy()]
    for x in bad:
        try:
            env.rollout(x, gamma)
        except ValueError:
            pass
        else:
            raise AssertionError("VecEnv.rollout accepted plans of %r" % (getattr(x, "shape", None),))
    for g in (-0.1, 1.5, float("nan")):
        try:
            env.rollout(good, g)
        except ValueError:
            pass
        else:
            raise AssertionError("VecEnv.rollout accepted gamma %r" % (g,))

    # 4. ten steps of the model-predictive-control recipe
    P, H = 8, 5
    for _ in range(10):
        plans = torch.randint(0, 9, (P, H, B), dtype=torch.int32, device=dev, generator=gen)
        o, r, t, n, ret = env.rollout(plans, gamma)
        tail = env.q_values(o.view(P * B, V)).view(P, B, 9).max(-1).values
        best = (ret + gamma ** H * tail * (t == 0)).argmax(0)
        first = plans[best, 0, torch.arange(B, device=dev)].contiguous()
        assert best.shape == (B,) and first.shape == (B,) and first.dtype == torch.int32 and bool(torch.isfinite(ret).all())
        _, _, _, stepped = env.step(first)
        calls += 1
    assert bool(stepped.any()) and env.status() == abi.LOB_OK
    _, n_roll = eng.kernel_time_ms("vec_rollout_kernel")
    assert n_roll == calls, (n_roll, calls)
    assert set(vars(env)) == attrs, "rollout() keeps nothing on the VecEnv"
    eng.close()

    # 5. a VecEnv that never calls rollout()
    eng = make_engine()
    env = VecEnv(eng)
    env.reset()
    for _ in range(5):
        random_step()
    assert env.status() == abi.LOB_OK
    _, n_roll = eng.kernel_time_ms("vec_rollout_kernel")
    assert n_roll == 0 and set(vars(env)) == attrs, n_roll
    eng.close()
    print("rollout OK: %d books, %d points of the episode against step(), the MPC recipe" % (B, checked))


if __name__ == "__main__":
    main()
