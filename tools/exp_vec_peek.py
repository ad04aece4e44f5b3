"""What the one-step look-ahead costs (lob_vec_peek): synthetic 10-level books on one GPU, two trade slots, the books
`--mid` random steps into the episode (kept in snapshot slot 0 and put back before every timed window, so that every window starts from
the same books) --
  a  the HIP-event time of vec_peek_kernel (lob_kernel_time_ms) for mask = all nine actions and for mask = one action;
  b  VecEnv.peek() as a caller sees it: host clock around `--calls` calls plus one synchronise;
  c  the route it replaces, through the same VecEnv: save(1), then nine times step(full(a)), a clone of the four outputs and
     restore(1) -- 1 + 9 x (three step launches, a restore and an observe) launches; host clock around one route plus one synchronise;
  d  env.step() under a torch policy with and without a peek() in front: host clock around `--steps` steps plus one synchronise.
All legs are taken in turn, once per round, in this one process; median, min and max over `--rounds` rounds (after `--warm` untimed
ones).  Before the rounds the nine planes of peek() are compared with the route's clones for equality.
    python tools/exp_vec_peek.py [books ...] [--rounds 21] [--warm 3] [--steps 20] [--calls 5] [--mid 30] [--trades 2] [--out profiles/vec_peek.json]"""
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
ROUNDS, WARM, STEPS, CALLS, MID = take("--rounds", 21, int), take("--warm", 3, int), take("--steps", 20, int), take("--calls", 5, int), take("--mid", 30, int)
TRADES = take("--trades", 2, int)   # 2: the kernels of two trade slots (<true>); 3: the general ones (<false>)
BATCHES = [int(x) for x in sys.argv[1:]] or [65536, 4096]
DEPTH, N, ONE = 10, abi.LOB_N_ACTIONS, 4


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


def stat(t):
    return {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": len(t), "all": t}


def measure(B):
    p = engine.default_params()
    p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
    g = engine.default_gen_params()
    g.n_events = 64 + 6 * (MID + STEPS + 16)
    eng = engine.Engine(p, B)
    eng.gen_events(g)
    env = VecEnv(eng)
    dev = env.device
    env.reset()
    for _ in range(MID):
        env.step(policy_torch(env.obs))
    env.save(0)
    fulls = [torch.full((B,), a, dtype=torch.int32, device=dev) for a in range(N)]
    one_out = None

    def sync():
        eng.sync()
        torch.cuda.synchronize()

    def composed():
        env.save(1)
        kept = []
        for a in range(N):
            o, r, t, s = env.step(fulls[a])
            kept.append((o.clone(), r.clone(), t.clone(), s.clone()))
            env.restore(1)
        return kept

    # the same results both ways, at this size
    env.restore(0)
    pk = [x.clone() for x in env.peek()]
    kept = composed()
    equal = all(torch.equal(pk[0][a], kept[a][0]) and torch.equal(pk[1][a].view(torch.int64), kept[a][1].view(torch.int64))
                and torch.equal(pk[2][a], kept[a][2]) and torch.equal(pk[3][a], kept[a][3]) for a in range(N))
    live = int((env.terminal == 0).sum())
    stepped_books = int(pk[3][0].sum())
    one_out = abi.VecPeekOut(env.peek_obs.data_ptr(), env.peek_reward.data_ptr(), env.peek_terminal.data_ptr(), env.peek_stepped.data_ptr())
    sync()

    def kernel_ms(mask):
        env.restore(0)
        sync()
        eng.kernel_timing(1)             # (clears the timers)
        for _ in range(CALLS):
            eng.vec_peek(mask, one_out)
        eng.sync()
        ms, n = eng.kernel_time_ms("vec_peek_kernel")
        assert n == CALLS, n
        eng.kernel_timing(0)
        return ms

    def peek_ms():
        env.restore(0)
        sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            env.peek()
        sync()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    def composed_ms():
        env.restore(0)
        sync()
        t0 = time.perf_counter()
        composed()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def steps_ms(with_peek):
        env.restore(0)
        sync()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            if with_peek:
                env.peek()
            env.step(policy_torch(env.obs))
        sync()
        return (time.perf_counter() - t0) * 1e3 / STEPS

    legs = {"vec_peek_kernel, all nine actions (HIP events)": lambda: kernel_ms(abi.PEEK_ALL),
            "vec_peek_kernel, one action (HIP events)": lambda: kernel_ms(1 << ONE),
            "VecEnv.peek(), all nine (host clock, per call)": peek_ms,
            "composed route: save + 9 x (step + clone + restore) (host clock, per route)": composed_ms,
            "VecEnv.step() (host clock, per step)": lambda: steps_ms(False),
            "VecEnv.peek() + VecEnv.step() (host clock, per step)": lambda: steps_ms(True)}
    times = {k: [] for k in legs}
    for r in range(WARM + ROUNDS):
        for k, fn in legs.items():
            ms = fn()
            if r >= WARM:
                times[k].append(ms)
    rc = env.status()
    res = {"books": B, "live_books": live, "books_that_step": stepped_books, "peek_equals_composed_route": equal, "lob_vec_status": rc,
           "legs_ms": {k: stat(v) for k, v in times.items()}}
    ks = list(legs)
    res["composed_route_over_peek"] = res["legs_ms"][ks[3]]["median"] / res["legs_ms"][ks[2]]["median"]
    res["peek_faster_than_composed_route"] = res["legs_ms"][ks[2]]["max"] < res["legs_ms"][ks[3]]["min"]
    print("%d books (%d live, %d step), peek == composed route: %s, lob_vec_status %d" % (B, live, stepped_books, equal, rc))
    for k in ks:
        v = res["legs_ms"][k]
        print("  %-80s %.4f ms (min %.4f, max %.4f)" % (k, v["median"], v["min"], v["max"]))
    print("  composed route / peek = %.1f" % res["composed_route_over_peek"])
    eng.close()
    return res


results = [measure(B) for B in BATCHES]
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"depth": DEPTH, "max_trades": TRADES, "algo": "qlambda", "theta": "shared", "mid_episode_steps": MID, "rounds": ROUNDS,
                   "warm_rounds": WARM, "calls_per_window": CALLS, "steps_per_window": STEPS, "one_action": ONE, "batches": results}, fh, indent=1)
