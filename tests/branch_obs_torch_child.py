"""Child process of tests/test_gpu_branch_obs.py::test_vec_env_branch_tensors_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  130 books,
depth 5, two trade slots.
  1. VecEnv.branch(3, book=True, history=5): shapes, dtypes and device of the eight persistent tensors; behind the fork every plane
     is the VecEnv's own book / history tensor of that name.
  2. fork / step / select / step: behind each, the tensors equal what the raw calls (Engine.branch_book / branch_history) write
     into fresh tensors on the same engine; the actions come from a torch network over br.levels / br.hist_levels / br.own -- the
     recipe of the class docstring --, produced right before each call with no synchronise between.
  3. history outside 0 .. MAX_HISTORY raises ValueError; Branches(env, n) without the flags has no .levels and launches neither
     kernel; the old call signature still works."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import Branches, VecEnv  # noqa: E402

B, D, T, NA = 130, 5, 2, abi.LOB_N_ACTIONS
N, K = 3, 5
KERNELS = ("branch_book_kernel", "branch_hist_kernel")
NAMES = ("levels", "own", "time_ms", "hist_levels", "hist_trades", "hist_time_ms", "hist_valid", "hist_rec")


def launches(eng):
    eng.sync()
    return [eng.kernel_time_ms(k)[1] for k in KERNELS]


def raw(env, br):
    """The two raw calls into fresh tensors, through the same hand-off."""
    t = {k: torch.full_like(getattr(br, k), -1 if getattr(br, k).dtype != torch.float32 else float("nan")) for k in NAMES}
    book = abi.VecBookOut(t["levels"].data_ptr(), t["own"].data_ptr(), t["time_ms"].data_ptr())
    hist = abi.VecHistOut(*[t[k].data_ptr() for k in NAMES[3:]])
    env._on_engine(env.eng.branch_book, book)
    env._on_engine(env.eng.branch_history, K, hist)
    return t


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def check(env, br, tag):
    want = raw(env, br)
    for k in NAMES:
        assert torch.equal(bits(getattr(br, k)), bits(want[k])), "%s: .%s against the raw call" % (tag, k)


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = engine.default_params()
    p.depth, p.max_trades = D, T
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_SHARED, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 160
    eng = engine.Engine(p, B)
    eng.load_events(engine.gen_stream_host(g, D, T, 0, B))
    eng.kernel_timing(True)
    env = VecEnv(eng, book=True, history=K)
    env.reset()
    for _ in range(6):
        env.step(torch.randint(0, NA, (B,), generator=gen, device="cuda", dtype=torch.int32))

    # 3 (first, while neither kernel has run). without the flags: today's attributes and launches; the old signature
    plain = env.branch(N)
    assert isinstance(plain, Branches) and not hasattr(plain, "levels") and not hasattr(plain, "hist_levels")
    plain.step(torch.zeros((N, B), device="cuda", dtype=torch.int32))
    old = Branches(env, N)
    assert not hasattr(old, "levels") and old.book_out is None and old.hist_out is None
    assert launches(eng) == [0, 0], "a branch set without the options launched the observation kernels"
    for bad in (-1, abi.MAX_HISTORY + 1, 2.5):
        try:
            env.branch(N, history=bad)
        except ValueError:
            pass
        else:
            raise AssertionError("VecEnv.branch accepted history = %r" % (bad,))

    # 1. the fork
    books = bytes(eng.get_books())
    br = env.branch(N, book=True, history=K)
    shapes = {"levels": ((N, B, 4, D), torch.float32), "own": ((N, B, 16), torch.float32), "time_ms": ((N, B), torch.int64),
              "hist_levels": ((N, B, K, 4, D), torch.float32), "hist_trades": ((N, B, K, 2, T), torch.float32),
              "hist_time_ms": ((N, B, K), torch.int32), "hist_valid": ((N, B), torch.int32), "hist_rec": ((N, B), torch.int32)}
    for k, (shape, dtype) in shapes.items():
        x = getattr(br, k)
        assert (tuple(x.shape), x.dtype) == (shape, dtype) and x.device == env.device and x.is_contiguous(), k
        assert torch.equal(bits(x), bits(getattr(env, k)).unsqueeze(0).expand(x.shape)), "behind the fork: .%s is the VecEnv's own in every plane" % k
    check(env, br, "fork")

    # 2. a network over the book and the window drives the loop
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(K * 4 * D + 4 * D + 16, 32), torch.nn.Tanh(), torch.nn.Linear(32, NA)).to(dev)

    def policy():
        x = torch.cat([br.hist_levels.flatten(2), br.levels.flatten(2), br.own], dim=2)
        x = torch.nan_to_num(x) / (1.0 + torch.nan_to_num(x).abs().amax(dim=(0, 1), keepdim=True))
        with torch.no_grad():
            return net(x.view(N * B, -1)).argmax(-1).to(torch.int32).view(N, B)

    first = torch.randint(0, NA, (N, B), generator=gen, device="cuda", dtype=torch.int32)
    first[torch.rand((N, B), generator=gen, device="cuda") < 0.3] = -1   # (a "stay" here and there sets the branches' records apart)
    br.step(first)
    check(env, br, "step 0")
    for h in range(1, 4):
        br.step(policy())
        check(env, br, "step %d" % h)
    assert bool((br.hist_rec != br.hist_rec[:1]).any()) and bool(br.stepped.any())
    before = {k: getattr(br, k).clone() for k in NAMES}
    parent = torch.randint(0, N, (N, B), generator=gen, device="cuda", dtype=torch.int32)
    br.select(parent)
    cols = torch.arange(B, device=dev)
    for k in NAMES:
        assert torch.equal(bits(getattr(br, k)), bits(before[k][parent.long(), cols])), "select: .%s is the gather" % k
    check(env, br, "select")
    br.step(policy())
    check(env, br, "a step behind the select")
    br.fork()
    check(env, br, "fork again")
    assert bytes(eng.get_books()) == books, "the branches moved the books"
    assert min(launches(eng)) >= 8 and env.status() == abi.LOB_OK
    br.close()
    eng.close()
    print("branch obs OK: %d books, %d branches, K = %d through fork / step / select against the raw calls" % (B, N, K))


if __name__ == "__main__":
    main()
