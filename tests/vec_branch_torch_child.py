"""Child process of tests/test_gpu_vec_branch.py::test_vec_env_branches_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  130 books,
depth 5, two trade slots, nine branches, every action made by torch on the device from the branches' own observations.
  1. branch(9): shapes, dtypes and device of the persistent tensors; the fork's outputs; nothing of the environment moved.
  2. four closed-loop steps under q_values(obs).argmax -- the actions produced by torch ops right before each call and the outputs
     consumed right after, no synchronise between --, one select by a top-k of the returns so far, two more steps; the recorded
     actions, laid out per branch along its ancestry, go through env.rollout: rewards of every step, obs / terminal behind the last.
  3. the two recipes of the module docstring (the greedy policy's return; a beam step) against env.rollout of what they played.
  4. what raises ValueError; fork() again after real steps; close().
  5. a VecEnv that never calls branch() launches nothing for it and holds no tensor of it."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import Branches, VecEnv  # noqa: E402

B, D, T, NA = 130, 5, 2, abi.LOB_N_ACTIONS
KERNELS = ("branch_fork_kernel", "branch_step_kernel", "branch_select_kernel")


def make_engine():
    p = engine.default_params()
    p.depth, p.max_trades = D, T
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_SHARED, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 160
    rec = engine.gen_stream_host(g, D, T, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    eng.kernel_timing(True)
    return eng


def launches(eng):
    return [eng.kernel_time_ms(k)[1] for k in KERNELS]


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = make_engine()
    env = VecEnv(eng)
    V = env.V
    attrs = set(vars(env))
    env.reset()
    cols = torch.arange(B, device=dev)

    def random_step():
        env.step(torch.randint(0, NA, (B,), generator=gen, device="cuda", dtype=torch.int32))

    for _ in range(5):
        eng.td_step(1)   # (weights that are not all zero: argmax has something to choose among)
    for _ in range(6):
        random_step()

    def greedy(br):
        return env.q_values(br.obs.view(br.n * B, V)).argmax(-1).to(torch.int32).view(br.n, B)

    # 1. the fork
    N = 9
    books = bytes(eng.get_books())
    obs_now = env.obs.clone()
    br = env.branch(N)
    assert isinstance(br, Branches) and br.n == N
    assert (br.obs.shape, br.obs.dtype) == ((N, B, V), torch.float32) and (br.reward.shape, br.reward.dtype) == ((N, B), torch.float64)
    assert (br.terminal.shape, br.terminal.dtype) == ((N, B), torch.uint8) and (br.stepped.shape, br.stepped.dtype) == ((N, B), torch.int32)
    assert all(x.device == env.device and x.is_contiguous() for x in (br.obs, br.reward, br.terminal, br.stepped))
    assert torch.equal(br.obs, obs_now.unsqueeze(0).expand(N, B, V)) and torch.equal(br.terminal, env.terminal.unsqueeze(0).expand(N, B))
    assert not bool(br.reward.any()) and not bool(br.stepped.any())

    # 2. closed loop, a select, closed loop again -- against rollout() of the recorded actions
    played, rewards = [], []
    a = torch.randint(0, NA, (N, B), generator=gen, device="cuda", dtype=torch.int32)   # (a first step that sets the branches apart)
    for h in range(5):
        o, r, t, s = br.step(a)
        played.append(a)
        rewards.append(r.clone())
        a = greedy(br)   # made from the outputs right behind the call, consumed by the next call: no synchronise in between
    ret = torch.stack(rewards).sum(0)
    parent = ret.topk(N, dim=0).indices.to(torch.int32).contiguous()   # the branches of every book ordered by their return so far
    parent[N // 2:] = parent[:N - N // 2].clone()                             # ... the better half twice
    obs_before, term_before = br.obs.clone(), br.terminal.clone()
    so, st = br.select(parent)
    assert torch.equal(so, obs_before[parent.long(), cols]) and torch.equal(st, term_before[parent.long(), cols])
    first = torch.stack(played)[:, parent.long(), cols]   # [5][N][B]: the ancestors' actions
    later = []
    for h in range(2):
        a = greedy(br)
        br.step(a)
        later.append(a)
        rewards.append(br.reward.clone())
    plans = torch.cat([first, torch.stack(later)]).permute(1, 0, 2).contiguous()   # [N][7][B]
    assert bytes(eng.get_books()) == books, "the branches moved the books"
    o, r, t, n, _ = env.rollout(plans, 1.0)
    for h in range(5):
        assert torch.equal(rewards[h][parent.long(), cols].view(torch.int64), r[:, h].view(torch.int64)), "reward of step %d, along the ancestry" % h
    for h in (5, 6):
        assert torch.equal(rewards[h].view(torch.int64), r[:, h].view(torch.int64)), "reward of step %d" % h
    assert torch.equal(br.obs, o) and torch.equal(br.terminal, t)
    assert bool((torch.stack(later) != torch.stack(later)[:, :1]).any()), "the greedy actions of two branches of some book differ"
    assert bool(n.any())

    # 3. the recipes of the module docstring
    n_b, H, gamma = 4, 4, 0.97
    random_step()
    books = bytes(eng.get_books())
    br = env.branch(n_b)
    ret = torch.zeros((n_b, B), dtype=torch.float64, device=dev)
    acts = []
    for h in range(H):
        a = greedy(br)
        br.step(a)
        ret += gamma ** h * br.reward
        acts.append(a)
    o, r, t, n, _ = env.rollout(torch.stack(acts).permute(1, 0, 2).contiguous(), gamma)
    want = torch.zeros_like(ret)
    for h in range(H):
        want += gamma ** h * r[:, h]
    assert torch.equal(ret.view(torch.int64), want.view(torch.int64)) and torch.equal(br.obs, o) and torch.equal(br.terminal, t)
    assert torch.equal(o[0], o[1]) and bool(n.any()), "one policy from one state: the branches agree"
    # beam search: k beams and their nine children each in one set; a round is one select and one step
    k, H = 3, 3
    br = env.branch(k * NA)
    child_action = (torch.arange(k * NA, device=dev) % NA).to(torch.int32).unsqueeze(1).expand(k * NA, B).contiguous()
    beam = torch.zeros((k, B), dtype=torch.int64, device=dev)
    ret = torch.zeros((k, B), dtype=torch.float64, device=dev)
    a_hist = torch.zeros((k, 0, B), dtype=torch.int32, device=dev)
    r_hist = torch.zeros((k, 0, B), dtype=torch.float64, device=dev)
    for h in range(H):
        br.select(beam.repeat_interleave(NA, dim=0).to(torch.int32))
        o, r, t, s = br.step(child_action)
        total = ret.repeat_interleave(NA, dim=0) + gamma ** h * r
        value = env.q_values(o.view(k * NA * B, V)).view(k * NA, B, NA).max(-1).values * (t == 0)
        beam = (total + gamma ** (h + 1) * value).topk(k, dim=0).indices
        ret = total.gather(0, beam)
        up = (beam // NA).unsqueeze(1)   # [k][1][B]: the beam each survivor descends from
        a_hist = torch.cat([a_hist.gather(0, up.expand(k, h, B)), (beam % NA).to(torch.int32).unsqueeze(1)], 1)
        r_hist = torch.cat([r_hist.gather(0, up.expand(k, h, B)), r.gather(0, beam).unsqueeze(1)], 1)
    o, r, t, n, _ = env.rollout(a_hist.contiguous(), gamma)
    assert torch.equal(r.view(torch.int64), r_hist.view(torch.int64)), "the rewards along the surviving beams"
    assert torch.equal(br.obs.gather(0, beam.unsqueeze(2).expand(k, B, V)), o) and torch.equal(br.terminal.gather(0, beam), t)
    assert bool((a_hist != a_hist[:1]).any()), "beams of some book that differ"
    assert bytes(eng.get_books()) == books, "the branches moved the books"

    # 4. what is refused; fork() again behind real steps; close()
    good = torch.zeros((k * NA, B), device="cuda", dtype=torch.int32)
    bad = [good.long(), good.cpu(), good[:, :B - 1].contiguous(), good.t(), good[0], good[:k], good.unsqueeze(0), good.cpu().numpy()]
    for fn in (br.step, br.select):
        for x in bad:
            try:
                fn(x)
            except ValueError:
                pass
            else:
                raise AssertionError("Branches.%s accepted %r" % (fn.__name__, getattr(x, "shape", None)))
    for x in (0, abi.MAX_BRANCHES + 1, 2.5):
        try:
            env.branch(x)
        except ValueError:
            pass
        else:
            raise AssertionError("VecEnv.branch accepted n = %r" % (x,))
    for _ in range(3):
        random_step()
    fo, fr, ft, fs = br.fork()
    assert torch.equal(fo, env.obs.unsqueeze(0).expand(k * NA, B, V)) and not bool(fs.any()) and not bool(fr.any())
    n_before = launches(eng)
    assert all(x > 0 for x in n_before), n_before
    br.close()
    try:
        br.step(good)
    except engine.LobError as e:
        assert e.code == abi.LOB_ESTATE
    else:
        raise AssertionError("a step on a closed set was accepted")
    br.fork()
    br.step(good)
    assert bool(br.stepped.any()) and env.status() == abi.LOB_OK
    assert set(vars(env)) == attrs, "branch() keeps nothing on the VecEnv"
    eng.close()

    # 5. a VecEnv that never calls branch()
    eng = make_engine()
    env = VecEnv(eng)
    env.reset()
    for _ in range(5):
        random_step()
    assert env.status() == abi.LOB_OK
    assert launches(eng) == [0, 0, 0] and set(vars(env)) == attrs
    eng.close()
    print("branches OK: %d books, closed loop over a select against rollout(), the two recipes" % B)


if __name__ == "__main__":
    main()
