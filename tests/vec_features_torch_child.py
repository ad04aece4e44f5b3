"""Child process of tests/test_gpu_vec_features.py::test_vec_env_features_and_update_through_torch (not collected by pytest).

torch is imported FIRST, so that the engine library resolves to the HIP runtime torch has loaded (rl_markets_amd/abi.py).  70 books,
SARSA on one weight vector shared by all books, the streams of tests/test_gpu_vec_act.py.
  1. VecEnv.features() / tile_index(): the persistent .feat_sums, a fresh tensor for given rows, (sums, idx) with actions; idx equals
     tile_index(sums, actions) and Engine.features' plane of the action; tile_terms is int64 [3, 9].
  2. update(): weights made of dyadic steps only, so every sum below is exact.  The group weights are (1, 0, 1): the reference's value
     is 32 x w0 over group 0, 32 x w1 over group 1 and 64 x w2 over groups 1 AND 2 (quirk Q3), which with these weights is the plain
     sum over the 96 tiles -- q_values(obs)[s, a] == theta[tile_index(sums, a)].sum(-1), for all nine actions, and theta is
     lob_theta_get's.
  3. env.act("argmax") changes after an update that lifts one action's tiles.
  4. a wrong dtype / shape / device raises ValueError.
  5. a VecEnv that never calls the new methods allocates nothing for them and adds no launch."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


from rl_markets_amd import abi, engine  # noqa: E402
from rl_markets_amd.vec_env import VecEnv  # noqa: E402
from tests.test_gpu_vec_act import make_params, streams  # noqa: E402

B = 70
NA = abi.LOB_N_ACTIONS


def make_engine():
    p = make_params(abi.ALGO_SARSA, abi.THETA_SHARED, mem=1 << 20)
    p.group_weights[0], p.group_weights[1], p.group_weights[2] = 1.0, 0.0, 1.0
    eng = engine.Engine(p, B)
    eng.load_events(streams(p, B))
    eng.kernel_timing(True)
    return eng, p


def counts(eng):
    eng.sync()
    return eng.kernel_time_ms("vec_features_kernel")[1], eng.kernel_time_ms("vec_update_kernel")[1]


def main():
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    eng, p = make_engine()
    M = p.memory_size
    env = VecEnv(eng)
    obs = env.reset()
    assert env.feat_sums is None and env._tile_terms is None, "nothing is allocated before the first use"
    assert counts(eng) == (0, 0)
    for _ in range(4):
        obs, _, _, _ = env.step(torch.randint(0, NA, (B,), generator=gen, device="cuda", dtype=torch.int32))

    # 1. features / tile_index
    terms = env.tile_terms
    assert terms.dtype == torch.int64 and terms.shape == (3, NA) and terms.is_cuda and env.tile_terms is terms
    assert terms.cpu().tolist() == eng.vec_terms()
    sums = env.features()
    assert sums is env.feat_sums and sums.dtype == torch.int32 and sums.shape == (B, abi.N_TILES) and sums.is_cuda
    cube = torch.from_numpy(eng.features(obs.cpu().numpy())).cuda().long()          # [B, 9, 96]: lob_features of the same rows
    for a in range(NA):
        acts = torch.full((B,), a, dtype=torch.int32, device="cuda")
        ti = env.tile_index(sums, acts)
        assert ti.dtype == torch.int64 and ti.shape == (B, abi.N_TILES)
        assert torch.equal(ti, cube[:, a]), "tile_index against lob_features, action %d" % a
    acts = torch.randint(0, NA, (B,), generator=gen, device="cuda", dtype=torch.int32)
    s2, idx = env.features(obs, acts)
    assert s2 is not env.feat_sums and torch.equal(s2, sums), "given rows: a fresh tensor, the same sums for the same rows"
    assert idx.dtype == torch.int32 and torch.equal(idx.long(), env.tile_index(sums, acts))
    assert torch.equal(idx.long(), cube[torch.arange(B, device="cuda"), acts.long()])
    s3, idx3 = env.features(actions=acts)
    assert s3 is env.feat_sums and torch.equal(idx3, idx)
    s4 = env.features(obs[:5].contiguous())
    assert s4.shape == (5, abi.N_TILES) and torch.equal(s4, sums[:5])
    assert counts(eng) == (4, 0)

    # 2. update: dyadic weights, then Q is the plain sum over the tiles
    assert (eng.theta() == 0).all()
    rows = (torch.rand((200, eng.V), generator=gen, device="cuda") * 8 - 4).float()
    rsteps = torch.randint(-1000, 1001, (200,), generator=gen, device="cuda").double() / 1024
    racts = torch.randint(0, NA, (200,), generator=gen, device="cuda", dtype=torch.int32)
    env.update(rsteps, racts, vars=rows)                                           # free-standing rows
    step = torch.randint(-1000, 1001, (B,), generator=gen, device="cuda").double() / 1024
    env.update(step, acts)                                                         # the books
    theta = torch.from_numpy(eng.theta()).cuda()
    want = torch.zeros(M, dtype=torch.float64, device="cuda")
    want.index_put_((env.tile_index(env.features(rows), racts).reshape(-1),), rsteps.repeat_interleave(abi.N_TILES), accumulate=True)
    want.index_put_((env.tile_index(sums, acts).reshape(-1),), step.repeat_interleave(abi.N_TILES), accumulate=True)
    assert torch.equal(theta, want), "lob_theta_get after the two updates"
    q = env.q_values(obs)
    for a in range(NA):
        ti = env.tile_index(sums, torch.full((B,), a, dtype=torch.int32, device="cuda"))
        assert torch.equal(q[:, a], theta[ti].sum(-1)), "q_values against the sum over the tiles, action %d" % a
    assert (q != 0).any()
    assert counts(eng) == (5, 2)

    # 3. act("argmax") follows an update that lifts one action's tiles: the same action for every book, so that tiles the books share
    # are all lifted for that action and no other (two books on one group-0 triple with different targets would lift each other's)
    before = env.act("argmax").clone()
    live = env.terminal == 0
    c = int(torch.bincount(before[live].long(), minlength=NA).argmin())           # the action the fewest live books take now
    target = torch.full((B,), c, dtype=torch.int32, device="cuda")
    lift = torch.full((B,), 1024.0, dtype=torch.float64, device="cuda")   # (96 x 1 024 on one action: far above any value the unit steps have made)
    env.update(lift, target)
    after = env.act("argmax")
    assert live.any() and (before[live] != c).any() and (after[live] == c).all(), (c, before.tolist(), after.tolist())

    # 4. arguments
    bad_calls = [lambda: env.update(step.float(), acts), lambda: env.update(step, acts.long()), lambda: env.update(step[:5], acts),
                 lambda: env.update(step.cpu(), acts), lambda: env.update(step, acts, vars=obs.double()), lambda: env.update(step, acts, vars=obs[:5].contiguous()),
                 lambda: env.features(obs[:, :4]), lambda: env.features(obs.cpu()), lambda: env.features(obs, acts[:5]), lambda: env.features(actions=acts.long())]
    for k, call in enumerate(bad_calls):
        try:
            call()
            raise AssertionError("bad call %d was accepted" % k)
        except ValueError:
            pass
    # an action out of range is skipped and counted
    acts_bad = acts.clone()
    acts_bad[3] = NA
    env.update(step, acts_bad)
    assert env.status() == abi.LOB_EINVAL and env.bad_actions == 1 and env.status() == abi.LOB_OK
    eng.close()

    # 5. a VecEnv that never calls the new methods launches nothing new
    eng, p = make_engine()
    env = VecEnv(eng)
    env.reset()
    for _ in range(5):
        env.step(env.act())
    assert env.status() == abi.LOB_OK
    _, n_obs = eng.kernel_time_ms("vec_observe_kernel")
    assert n_obs == 5 and counts(eng) == (0, 0), (n_obs, counts(eng))
    assert env.feat_sums is None and env._tile_terms is None
    eng.close()
    print("vec features OK: %d books" % B)


if __name__ == "__main__":
    main()
