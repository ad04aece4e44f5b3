"""Child process of tests/test_gpu_look_ring.py::test_vec_env_ring_lookahead_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  70 books,
depth 10, two trade slots, streams of 1 200 records over a ring of 256 entries refilled every 16 steps; the twin's track is resident.
  1. VecEnv(eng, ring_lookahead=True) on the ring engine, a plain VecEnv on the twin; without the flag the ring engine refuses.
  2. one closed loop of 9 branches x 4 steps under q_values(br.obs.view(n * B, V)).argmax(-1), then peek() + step(), 40 times over:
     every tensor equal to the twin's.
  3. status() reports no cell outside the window, track_window() the three arrays; launch counts: the VecEnv without the flag has
     launched no refill of its own, the one with it has."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402
from tests import look_ring_cases as lc  # noqa: E402

B, D, T, N, H, ROUNDS = 70, 10, 2, abi.LOB_N_ACTIONS, 4, 40


def make_engine(ring, rec, p):
    os.environ["LOB_TRACK_RING"], os.environ["LOB_TRACK_REFILL"] = str(ring), str(lc.REFILL)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    eng.kernel_timing(True)
    return eng


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    p = lc.make_params(D, T)
    rec = lc.records(p, B, mixed=False)
    plain = VecEnv(make_engine(lc.RING, rec, p))
    plain.reset()
    try:
        plain.peek()
    except engine.LobError as e:
        assert e.code == abi.LOB_ESTATE and "ring" in str(e)
    else:
        raise AssertionError("a VecEnv without ring_lookahead peeked on a ring")
    ring, twin = VecEnv(make_engine(lc.RING, rec, p), ring_lookahead=True), VecEnv(make_engine(4096, rec, p))
    V = ring.V
    envs = (ring, twin)
    for env in envs:
        env.reset()
    brs = [env.branch(N) for env in envs]
    for rnd in range(ROUNDS):
        for env, br in zip(envs, brs):
            br.fork()
            for h in range(H):
                a = env.q_values(br.obs.view(N * B, V)).argmax(-1).to(torch.int32).view(N, B)
                br.step(a)
        for x, y in zip((brs[0].obs, brs[0].reward, brs[0].terminal, brs[0].stepped), (brs[1].obs, brs[1].reward, brs[1].terminal, brs[1].stepped)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "round %d: the closed loop" % rnd
        pa, pb = ring.peek(), twin.peek()
        for x, y in zip(pa, pb):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "round %d: peek" % rnd
        a = torch.randint(0, N, (B,), generator=gen, device="cuda", dtype=torch.int32)
        plain.step(a)
        for x, y in zip(ring.step(a), twin.step(a)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "round %d: step" % rnd
        assert torch.equal(plain.obs, ring.obs)
    assert ring.status() == abi.LOB_OK and (ring.ahead_cells, ring.behind_cells) == (0, 0)
    assert plain.status() == abi.LOB_OK and (plain.ahead_cells, plain.behind_cells) == (0, 0)
    lo, hi, comp = ring.track_window()
    assert lo.shape == hi.shape == comp.shape == (B,) and (lo < hi).all() and (hi - lo <= lc.REACH).all() and (comp == 0).all()
    # launches: the plain VecEnv's refills are the schedule's alone, ROUNDS // REFILL of them; the look-aheads have added theirs.
    # (The exact count follows maybe_refill_track's convention, lob_engine.hip: the counter goes up behind every real step and the
    # refill is launched, and the counter cleared, when it reaches LOB_TRACK_REFILL -- 40 steps at a refill every 16: two.  Another
    # convention there means another number here, not a fault of the look-aheads.)
    _, n_plain = plain.eng.kernel_time_ms("prepass_extend_kernel")
    _, n_ring = ring.eng.kernel_time_ms("prepass_extend_kernel")
    assert n_plain == ROUNDS // lc.REFILL and n_ring > n_plain, (n_plain, n_ring)
    for name in ("vec_peek_kernel", "vec_rollout_kernel", "branch_fork_kernel", "branch_step_kernel"):
        assert plain.eng.kernel_time_ms(name)[1] == 0, name
    for br in brs:
        br.close()
    for env in envs + (plain,):
        env.eng.close()
    print("look ring OK: %d books, %d rounds of a closed loop of %d branches x %d steps, peek and step against the resident twin" % (B, ROUNDS, N, H))


if __name__ == "__main__":
    main()
