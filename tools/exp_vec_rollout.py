"""What the multi-step look-ahead costs (lob_vec_rollout): synthetic 10-level books on one GPU, two trade slots, the
books `--mid` random steps into the episode (kept in snapshot slot 0 and put back before every timed window, so that every window
starts from the same books) --
  a  the HIP-event time of vec_rollout_kernel (lob_kernel_time_ms) for (P, H) = (9, 1), (9, 4), (9, 8), (32, 8), random per-book plans,
     beside vec_peek_kernel with all nine actions: (9, 1) against the peek shows what the loop and the per-lane actions cost;
  b  VecEnv.rollout() for the same shapes as a caller sees it: host clock around `--calls` calls plus one synchronise;
  c  the route (9, 4) replaces, through the same VecEnv: save(1), then nine times (four step()s with a clone of the reward behind each, a
     clone of the other outputs, restore(1)) -- 1 + 9 x (3 x 4 + 2) launches plus the clones; host clock around one route plus one
     synchronise.
All legs are taken in turn, once per round, in this one process; median, min and max over `--rounds` rounds (after `--warm` untimed
ones).  Before the rounds the outputs of rollout(9, 4) are compared with the route's clones for equality.
    python tools/exp_vec_rollout.py [books ...] [--rounds 21] [--warm 3] [--calls 5] [--mid 30] [--trades 2] [--out profiles/vec_rollout.json]"""
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
DEPTH, N, GAMMA = 10, abi.LOB_N_ACTIONS, 0.97
SHAPES = [(9, 1), (9, 4), (9, 8), (32, 8)]
ROUTE = (9, 4)


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


def stat(t):
    return {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": len(t), "all": t}


def measure(B):
    p = engine.default_params()
    p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
    g = engine.default_gen_params()
    g.n_events = 64 + 6 * (MID + max(H for _, H in SHAPES) + 16)
    eng = engine.Engine(p, B)
    eng.gen_events(g)
    env = VecEnv(eng)
    dev = env.device
    env.reset()
    for _ in range(MID):
        env.step(policy_torch(env.obs))
    env.save(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    plans = {s: torch.randint(0, N, (s[0], s[1], B), generator=gen, device=dev, dtype=torch.int32) for s in SHAPES}

    def sync():
        eng.sync()
        torch.cuda.synchronize()

    def composed():
        P, H = ROUTE
        pl = plans[ROUTE]
        env.save(1)
        kept = []
        for q in range(P):
            rewards = []
            for h in range(H):
                o, r, t, s = env.step(pl[q, h])
                rewards.append(r.clone())
            kept.append((o.clone(), rewards, t.clone()))
            env.restore(1)
        return kept

    # the same results both ways, at this size
    env.restore(0)
    o, r, t, n, ret = env.rollout(plans[ROUTE], GAMMA)
    kept = composed()
    equal = all(torch.equal(o[q], kept[q][0]) and torch.equal(t[q], kept[q][2])
                and all(torch.equal(r[q, h].view(torch.int64), kept[q][1][h].view(torch.int64)) for h in range(ROUTE[1])) for q in range(ROUTE[0]))
    live = int((env.terminal == 0).sum())
    steps_done = float(n.double().mean())
    peek_out = [x for x in env.peek()]
    peek_out = abi.VecPeekOut(*[x.data_ptr() for x in peek_out])
    outs = {}
    for (P, H) in SHAPES:
        ts = (torch.empty((P, B, env.V), dtype=torch.float32, device=dev), torch.empty((P, H, B), dtype=torch.float64, device=dev),
              torch.empty((P, B), dtype=torch.uint8, device=dev), torch.empty((P, B), dtype=torch.int32, device=dev),
              torch.empty((P, B), dtype=torch.float64, device=dev))
        outs[(P, H)] = (ts, abi.VecRolloutOut(*[x.data_ptr() for x in ts]))
    sync()

    def kernel_ms(shape):
        env.restore(0)
        sync()
        eng.kernel_timing(1)             # (clears the timers)
        for _ in range(CALLS):
            if shape is None:
                eng.vec_peek(abi.PEEK_ALL, peek_out)
            else:
                eng.vec_rollout(plans[shape].data_ptr(), shape[0], shape[1], GAMMA, outs[shape][1])
        eng.sync()
        ms, k = eng.kernel_time_ms("vec_peek_kernel" if shape is None else "vec_rollout_kernel")
        assert k == CALLS, k
        eng.kernel_timing(0)
        return ms

    def rollout_ms(shape):
        env.restore(0)
        sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            env.rollout(plans[shape], GAMMA)
        sync()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    def composed_ms():
        env.restore(0)
        sync()
        t0 = time.perf_counter()
        composed()
        sync()
        return (time.perf_counter() - t0) * 1e3

    legs = {"vec_peek_kernel, all nine actions (HIP events)": lambda: kernel_ms(None)}
    for s in SHAPES:
        legs["vec_rollout_kernel P=%d H=%d (HIP events)" % s] = lambda s=s: kernel_ms(s)
    for s in SHAPES:
        legs["VecEnv.rollout() P=%d H=%d (host clock, per call)" % s] = lambda s=s: rollout_ms(s)
    route_key = "composed route P=%d H=%d: save + P x (H x (step + clone) + clones + restore) (host clock, per route)" % ROUTE
    legs[route_key] = composed_ms
    times = {k: [] for k in legs}
    for rnd in range(WARM + ROUNDS):
        for k, fn in legs.items():
            ms = fn()
            if rnd >= WARM:
                times[k].append(ms)
    rc = env.status()
    res = {"books": B, "live_books": live, "mean_steps_completed_P9_H4": steps_done, "rollout_equals_composed_route": equal, "lob_vec_status": rc,
           "legs_ms": {k: stat(v) for k, v in times.items()}}
    roll_key = "VecEnv.rollout() P=%d H=%d (host clock, per call)" % ROUTE
    res["composed_route_over_rollout"] = res["legs_ms"][route_key]["median"] / res["legs_ms"][roll_key]["median"]
    res["rollout_faster_than_composed_route"] = res["legs_ms"][roll_key]["max"] < res["legs_ms"][route_key]["min"]
    print("%d books (%d live, %.2f of 4 steps complete), rollout == composed route: %s, lob_vec_status %d" % (B, live, steps_done, equal, rc))
    for k in legs:
        v = res["legs_ms"][k]
        print("  %-100s %.4f ms (min %.4f, max %.4f)" % (k, v["median"], v["min"], v["max"]))
    print("  composed route / rollout(9, 4) = %.1f" % res["composed_route_over_rollout"])
    eng.close()
    return res


results = [measure(B) for B in BATCHES]
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"depth": DEPTH, "max_trades": TRADES, "algo": "qlambda", "theta": "shared", "mid_episode_steps": MID, "rounds": ROUNDS,
                   "warm_rounds": WARM, "calls_per_window": CALLS, "gamma": GAMMA, "shapes": SHAPES, "route": ROUTE, "batches": results}, fh, indent=1)
