"""What a branch set costs (lob_branch_*): synthetic 10-level books on one GPU, two trade slots, the books `--mid`
random steps into the episode; every timed window starts from a fresh fork of the same books --
  a  the HIP-event time of branch_step_kernel (lob_kernel_time_ms) for N = 1, 9, 32, random per-book actions, beside
     vec_rollout_kernel (P, H) = (9, 1): the same step with the state taken from the engine and nothing stored -- the difference is what
     loading and storing the set costs; with it the set's traffic, bytes per branch-step as laid out (lob_branch.h) against the bytes
     per second the kernel's time implies;
  b  branch_fork_kernel and branch_select_kernel (random per-book parents) for N = 9;
  c  Branches.step() for the same N as a caller sees it: host clock around `--calls` calls plus one synchronise;
  d  the closed-loop route N = 9, H = 4 replaces, through the same VecEnv: save(1), then nine times (four step()s under a policy in
     torch with a clone of the reward behind each, a clone of the other outputs, restore(1)) -- 1 + 9 x (3 x 4 + 2) launches plus the
     clones and the policy --, against fork() + four (policy, Branches.step()) rounds; host clock around one route plus one synchronise.
All legs are taken in turn, once per round, in this one process; median, min and max over `--rounds` rounds (after `--warm` untimed
ones).  Before the rounds the outputs of the two closed-loop routes are compared for equality.
    python tools/exp_vec_branch.py [books ...] [--rounds 21] [--warm 3] [--calls 5] [--mid 30] [--trades 2] [--out profiles/vec_branch.json]"""
import json
import os
import sys
import time

import torch   # before the engine library is loaded: one HIP runtime per process (rl_markets_amd/abi.py)
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rl_markets_amd import abi, engine
from rl_markets_amd.vec_env import VecEnv


def take(flag, default=None, cast=str):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        v = cast(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


out_path = take("--out")
ROUNDS, WARM, CALLS, MID = take("--rounds", 21, int), take("--warm", 3, int), take("--calls", 5, int), take("--mid", 30, int)
TRADES = take("--trades", 2, int)   # 2: the kernels of two trade slots (<true>); 3: the general ones (<false>)
BATCHES = [int(x) for x in sys.argv[1:]] or [65536, 4096]
DEPTH, NA = 10, abi.LOB_N_ACTIONS
SIZES = [1, 9, 32]
ROUTE = (9, 4)
BYTES_PER_LANE = 416   # lob_branch.h: 288 of LOB_ENV_FIELDS + 2 x 32 of the windows' running state + 64 of the observation (no rings: PnL reward)


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[..., 0] >> 3) ^ (bits[..., 1] >> 5)).remainder(9).to(torch.int32)


def stat(t):
    return {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": len(t), "all": t}


def measure(B):
    p = engine.default_params()
    p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
    g = engine.default_gen_params()
    g.n_events = 64 + 6 * (MID + CALLS + ROUTE[1] + 16)
    eng = engine.Engine(p, B)
    eng.gen_events(g)
    env = VecEnv(eng)
    dev = env.device
    env.reset()
    for _ in range(MID):
        env.step(policy_torch(env.obs))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    acts = {n: torch.randint(0, NA, (CALLS, n, B), generator=gen, device=dev, dtype=torch.int32) for n in SIZES}
    parents = torch.randint(0, 9, (9, B), generator=gen, device=dev, dtype=torch.int32)
    plan91 = acts[9][0].unsqueeze(1).contiguous()   # [9][1][B]
    roll_ts = (torch.empty((9, B, env.V), dtype=torch.float32, device=dev), torch.empty((9, 1, B), dtype=torch.float64, device=dev),
               torch.empty((9, B), dtype=torch.uint8, device=dev), torch.empty((9, B), dtype=torch.int32, device=dev),
               torch.empty((9, B), dtype=torch.float64, device=dev))
    roll_out = abi.VecRolloutOut(*[x.data_ptr() for x in roll_ts])

    def sync():
        eng.sync()
        torch.cuda.synchronize()

    def composed():
        N, H = ROUTE
        env.save(1)
        kept = []
        for q in range(N):
            rewards = []
            o = env.obs
            for h in range(H):
                o, r, t, s = env.step(policy_torch(o))
                rewards.append(r.clone())
            kept.append((o.clone(), rewards, t.clone()))
            env.restore(1)
        return kept

    def closed_loop(br):
        N, H = ROUTE
        o = br.fork()[0]
        rewards = []
        for h in range(H):
            o, r, t, s = br.step(policy_torch(o))
            rewards.append(r.clone())
        return o, rewards, t

    # the same results both ways, at this size (one policy from one state: every branch is the composed route's one trajectory)
    br9 = env.branch(9)
    o, rewards, t = closed_loop(br9)
    kept = composed()
    equal = all(torch.equal(o[q], kept[q][0]) and torch.equal(t[q], kept[q][2])
                and all(torch.equal(rewards[h][q].view(torch.int64), kept[q][1][h].view(torch.int64)) for h in range(ROUTE[1])) for q in range(ROUTE[0]))
    live = int((env.terminal == 0).sum())
    sync()

    def step_kernel_ms(n):
        br = env.branch(n)
        sync()
        eng.kernel_timing(1)             # (clears the timers)
        for c in range(CALLS):
            eng.branch_step(acts[n][c].data_ptr(), br.out)
        eng.sync()
        ms, k = eng.kernel_time_ms("branch_step_kernel")
        assert k == CALLS, k
        eng.kernel_timing(0)
        return ms

    def rollout_kernel_ms():
        sync()
        eng.kernel_timing(1)
        for _ in range(CALLS):
            eng.vec_rollout(plan91.data_ptr(), 9, 1, 1.0, roll_out)
        eng.sync()
        ms, k = eng.kernel_time_ms("vec_rollout_kernel")
        assert k == CALLS, k
        eng.kernel_timing(0)
        return ms

    def fork_select_ms(which):
        br = env.branch(9)
        br.step(acts[9][0])
        br.select(parents)               # (the second buffer is there before the clock starts)
        sync()
        eng.kernel_timing(1)
        for _ in range(CALLS):
            if which == "fork":
                eng.branch_fork(9, br.out)
            else:
                eng.branch_select(parents.data_ptr(), br.out)
        eng.sync()
        ms, k = eng.kernel_time_ms("branch_%s_kernel" % which)
        assert k == CALLS, k
        eng.kernel_timing(0)
        return ms

    def step_ms(n):
        br = env.branch(n)
        sync()
        t0 = time.perf_counter()
        for c in range(CALLS):
            br.step(acts[n][c])
        sync()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    def composed_ms():
        sync()
        t0 = time.perf_counter()
        composed()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def closed_loop_ms():
        br = env.branch(9)
        sync()
        t0 = time.perf_counter()
        closed_loop(br)
        sync()
        return (time.perf_counter() - t0) * 1e3

    legs = {"vec_rollout_kernel P=9 H=1 (HIP events)": rollout_kernel_ms}
    for n in SIZES:
        legs["branch_step_kernel N=%d (HIP events)" % n] = lambda n=n: step_kernel_ms(n)
    legs["branch_fork_kernel N=9 (HIP events)"] = lambda: fork_select_ms("fork")
    legs["branch_select_kernel N=9 (HIP events)"] = lambda: fork_select_ms("select")
    for n in SIZES:
        legs["Branches.step() N=%d (host clock, per call)" % n] = lambda n=n: step_ms(n)
    route_key = "composed closed-loop route N=%d H=%d: save + N x (H x (policy + step + clone) + clones + restore) (host clock, per route)" % ROUTE
    loop_key = "branch closed-loop route N=%d H=%d: fork + H x (policy + Branches.step() + clone) (host clock, per route)" % ROUTE
    legs[route_key] = composed_ms
    legs[loop_key] = closed_loop_ms
    times = {k: [] for k in legs}
    for rnd in range(WARM + ROUNDS):
        for k, fn in legs.items():
            ms = fn()
            if rnd >= WARM:
                times[k].append(ms)
    rc = env.status()
    res = {"books": B, "live_books": live, "closed_loop_equals_composed_route": equal, "lob_vec_status": rc,
           "legs_ms": {k: stat(v) for k, v in times.items()}}
    Bpad = (B + 63) // 64 * 64
    res["state_traffic"] = {}
    for n in SIZES:
        ms = res["legs_ms"]["branch_step_kernel N=%d (HIP events)" % n]["median"]
        moved = 2 * BYTES_PER_LANE * n * B   # loaded and stored, every lane live
        res["state_traffic"]["N=%d" % n] = {"bytes_per_branch_step_loaded_plus_stored": 2 * BYTES_PER_LANE, "set_bytes": BYTES_PER_LANE * n * Bpad,
                                            "state_bytes_moved_per_launch": moved, "implied_GB_per_s_of_state_alone": moved / (ms * 1e-3) / 1e9}
    res["composed_route_over_branch_route"] = res["legs_ms"][route_key]["median"] / res["legs_ms"][loop_key]["median"]
    print("%d books (%d live), closed loop == composed route: %s, lob_vec_status %d" % (B, live, equal, rc))
    for k in legs:
        v = res["legs_ms"][k]
        print("  %-125s %.4f ms (min %.4f, max %.4f)" % (k, v["median"], v["min"], v["max"]))
    for n in SIZES:
        print("  N=%d: %d state bytes per launch, %.1f GB/s of state alone" % (n, res["state_traffic"]["N=%d" % n]["state_bytes_moved_per_launch"],
                                                                              res["state_traffic"]["N=%d" % n]["implied_GB_per_s_of_state_alone"]))
    print("  composed route / branch route = %.1f" % res["composed_route_over_branch_route"])
    eng.close()
    return res


results = [measure(B) for B in BATCHES]
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"depth": DEPTH, "max_trades": TRADES, "algo": "qlambda", "theta": "shared", "mid_episode_steps": MID, "rounds": ROUNDS,
                   "warm_rounds": WARM, "calls_per_window": CALLS, "sizes": SIZES, "route": ROUTE, "bytes_per_lane": BYTES_PER_LANE,
                   "batches": results}, fh, indent=1)
