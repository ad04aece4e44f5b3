"""Child process of tests/test_gpu_snapshot.py::test_vec_env_save_and_restore_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  300 books,
depth 5, two trade slots, a random policy made by torch on the device through VecEnv(eng, book=True, history=8); the yardstick is the
oracle, replayed with the action arrays the engine saw (tests/test_gpu_snapshot.py: the shadow).
  1. save(0) after reset(), 6 steps, save(1); 7 more, restore(1, mask) with a torch.bool mask, then with the same mask as
     torch.uint8 from a fresh save: obs, levels and hist_levels are refreshed by restore() -- the masked rows are those kept at the
     save, the others those of the moment before --, and 5 steps on the books follow the shadow / the main oracle.
  2. the restart recipe: to the end of the episode, restore(0, mask=env.terminal != 0), n_live == B, and the day again against a
     fresh oracle.
  3. a wrong dtype / shape / device raises ValueError.
  4. a VecEnv that never saves launches nothing new."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402
from tests import oracle_lib as ol  # noqa: E402
from tests.parity import assert_books_equal, dumps_to_np  # noqa: E402

B, D, T, K = 300, 5, 2, 8


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
    return eng, p, rec


def check(env, eng, parts, tag):
    """obs, terminal and the dump of every book against the oracle it follows."""
    obs, term = env.obs.cpu().numpy(), env.terminal.cpu().numpy()
    eb = dumps_to_np(eng.get_books())
    cover = np.zeros(B, int)
    for orc, m in parts:
        cover += m
        recs = orc.recs()
        np.testing.assert_array_equal(obs[m], recs["vars"][m][:, :env.V], err_msg=tag + ": obs")
        np.testing.assert_array_equal(term[m], recs["book"]["terminal"][m], err_msg=tag + ": terminal")
        assert_books_equal(eb[m], recs["book"][m], tag)
    assert (cover == 1).all()


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    eng, p, rec = make_engine()
    env = VecEnv(eng, book=True, history=K)
    hist = []

    def shadow(s):
        o = ol.Oracle(p, rec)
        o.reset()
        for a in hist[:s]:
            o.env_step(a)
        return o

    def step(oracles):
        actions = torch.randint(0, abi.LOB_N_ACTIONS, (B,), generator=gen, device="cuda", dtype=torch.int32)
        env.step(actions)
        a = actions.cpu().numpy()
        hist.append(a)
        for o in oracles:
            o.env_step(a)

    orc = ol.Oracle(p, rec)
    orc.reset()
    env.reset()
    env.save(0)
    for _ in range(6):
        step([orc])
    env.save(1)
    kept = [t.clone() for t in (env.obs, env.levels, env.hist_levels, env.own)]
    for _ in range(7):
        step([orc])
    mask = torch.rand(B, generator=gen, device="cuda") < 0.5
    m = mask.cpu().numpy()
    assert 0 < m.sum() < B
    for dtype in (torch.bool, torch.uint8):
        # (the second round finds the masked books five steps past the save and the others five steps further on: slot 1 still holds
        # step 6, so the masked books go back to it once more; the uint8 mask selects with the byte 3 -- nonzero selects)
        mk = mask if dtype is torch.bool else mask.to(torch.uint8) * torch.tensor(3, dtype=torch.uint8, device="cuda")
        assert mk.dtype is dtype
        before = [t.clone() for t in (env.obs, env.levels, env.hist_levels, env.own)]
        ret = env.restore(1, mk)
        assert ret is env.obs
        for now, at_save, prev, name in zip((env.obs, env.levels, env.hist_levels, env.own), kept, before, ("obs", "levels", "hist_levels", "own")):
            assert torch.equal(now[mask], at_save[mask]), name + ": the masked rows are those of the save"
            assert torch.equal(now[~mask], prev[~mask]), name + ": the other rows are untouched"
        assert not torch.equal(env.own[mask], before[3][mask]), "the restored books moved back"
        assert int(env.n_live) == int((env.terminal == 0).sum())
        sh = shadow(6)
        parts = [(sh, m), (orc, ~m)]
        check(env, eng, parts, "restored (%s mask)" % dtype)
        for k in range(5):
            step([orc, sh])
            check(env, eng, parts, "%s mask, step +%d" % (dtype, k))
        sh.close()
    assert env.status() == abi.LOB_OK

    # 2. the restart recipe
    steps = 0
    while int(env.n_live) > 0:
        step([])
        steps += 1
        assert steps < 1000
    term = env.terminal.clone()
    assert bool((term != 0).all()) and bool((term == 2).any())
    obs = env.restore(0, mask=env.terminal != 0)
    assert int(env.n_live) == B and bool((env.terminal == 0).all())
    fresh = ol.Oracle(p, rec)
    fresh.reset()
    np.testing.assert_array_equal(obs.cpu().numpy(), fresh.recs()["vars"][:, :env.V])
    everyone = np.ones(B, bool)
    check(env, eng, [(fresh, everyone)], "restarted")
    n = 0
    while int(env.n_live) > 0:
        step([fresh])
        n += 1
        if n % 8 == 0:
            check(env, eng, [(fresh, everyone)], "second run, step %d" % n)
        assert n < 1000
    check(env, eng, [(fresh, everyone)], "second run, the end")
    assert n > 10

    # 3. masks that are refused
    good = torch.ones(B, dtype=torch.uint8, device="cuda")
    for bad in (good.to(torch.int32), good.to(torch.float32), good[:-1], torch.ones((B, 1), dtype=torch.uint8, device="cuda"), good.cpu(),
                torch.ones(2 * B, dtype=torch.uint8, device="cuda")[::2], [1] * B):
        for fn in (env.save, env.restore):
            try:
                fn(0, bad)
            except ValueError:
                pass
            else:
                raise AssertionError("VecEnv.%s accepted a bad mask: %r" % (fn.__name__, getattr(bad, "dtype", type(bad))))
    _, n_masked = eng.kernel_time_ms("snapshot_masked_kernel")
    _, n_all = eng.kernel_time_ms("snapshot_all_kernel")
    assert n_masked == 3 and n_all == 2, (n_masked, n_all)
    orc.close()
    fresh.close()
    eng.close()

    # 4. a VecEnv that never saves launches nothing new
    eng, p, rec = make_engine()
    env = VecEnv(eng)
    env.reset()
    for _ in range(5):
        env.step(torch.randint(0, abi.LOB_N_ACTIONS, (B,), generator=gen, device="cuda", dtype=torch.int32))
    assert env.status() == abi.LOB_OK
    _, n_obs = eng.kernel_time_ms("vec_observe_kernel")
    _, n_masked = eng.kernel_time_ms("snapshot_masked_kernel")
    _, n_all = eng.kernel_time_ms("snapshot_all_kernel")
    assert n_obs == 5 and n_masked == 0 and n_all == 0, (n_obs, n_masked, n_all)
    eng.close()
    print("snapshot OK: %d books, bool and uint8 masks, the restart recipe" % B)


if __name__ == "__main__":
    main()
