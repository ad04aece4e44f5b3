"""What the look-aheads cost on a ring-mode stream (lob_look_ring) beside the same calls on a resident track: synthetic
10-level books on one GPU, two trade slots, the books `--mid` random steps into the episode.  Two streams per batch size --
  ring      the shape of `bench.py --replay 61200 --events 50000`: every book replays one recorded stream of 61 200 events from its own
            phase, 50 000 events each, so the market track is a ring (default LOB_TRACK_RING / LOB_TRACK_REFILL), lob_look_ring on;
  resident  2 000 generated events per book, the whole track in memory, the switch off: the path as it was --
and on each the legs
  a  vec_peek_kernel, all nine actions (HIP events, lob_kernel_time_ms);
  b  vec_rollout_kernel, 9 plans x 4 steps, random per-book actions;
  c  branch_step_kernel, 9 branches, random per-book actions, every timed window behind a fresh fork;
  d  (ring) the prepass_extend_kernel launch that the host puts in front of a look-ahead, when it has ONE real step's worth of events
     to fill: an untimed roll-out of `LOB_TRACK_REFILL` steps first, whose depth reaches past the next scheduled refill and so forces
     one (the other legs have stepped the books since the last), then one VecEnv.step(), then the same roll-out timed; the launch is
     counted, so a round in which the schedule's own refill came instead shows as an assertion;
  e  VecEnv.step() as a caller sees it, and VecEnv.peek() + VecEnv.step(): host clock around `--calls` rounds plus one synchronise.
All legs are taken in turn, once per round, in this one process; median, min and max over `--rounds` rounds (after `--warm` untimed
ones).  lob_vec_status is read at the end: a run whose look-aheads left the window says so (ahead / behind cells).
    python tools/exp_look_ring.py [books ...] [--rounds 21] [--warm 3] [--calls 5] [--mid 30] [--out profiles/look_ring.json]"""
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
BATCHES = [int(x) for x in sys.argv[1:]] or [65536, 4096]
DEPTH, TRADES, NA = 10, 2, abi.LOB_N_ACTIONS
REPLAY, EVENTS, RESIDENT_EVENTS = 61200, 50000, 2000
PLANS, STEPS, BRANCHES = 9, 4, 9
REFILL = int(os.environ.get("LOB_TRACK_REFILL", "64"))   # the engine's default schedule, unless the caller has set another


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[..., 0] >> 3) ^ (bits[..., 1] >> 5)).remainder(9).to(torch.int32)


def stat(t):
    return {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": len(t), "all": t}


def make_engine(B, ring):
    p = engine.default_params()
    p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
    eng = engine.Engine(p, B)
    if ring:
        g = engine.default_gen_params()
        g.n_events = REPLAY
        day = engine.gen_stream_host(g, DEPTH, TRADES, 0, 1)[0]
        phase = np.random.default_rng(1994).integers(0, REPLAY - EVENTS + 1, size=B)
        eng.load_events_shared(day, phase, EVENTS)
    else:
        g = engine.default_gen_params()
        g.n_events = RESIDENT_EVENTS
        eng.gen_events(g)
    return eng


def measure(B, ring):
    eng = make_engine(B, ring)
    env = VecEnv(eng, ring_lookahead=ring)
    dev = env.device
    env.reset()
    for _ in range(MID):
        env.step(policy_torch(env.obs))
    lo, hi, comp = env.track_window()
    is_ring = bool((comp == 0).any())
    assert is_ring == ring, "the stream's track is %s" % ("a ring" if is_ring else "resident")
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    plans = torch.randint(0, NA, (PLANS, STEPS, B), generator=gen, device=dev, dtype=torch.int32)
    deep = torch.randint(0, NA, (1, REFILL, B), generator=gen, device=dev, dtype=torch.int32)
    acts = torch.randint(0, NA, (CALLS, BRANCHES, B), generator=gen, device=dev, dtype=torch.int32)

    def roll_buffers(P, H):
        ts = (torch.empty((P, B, env.V), dtype=torch.float32, device=dev), torch.empty((P, H, B), dtype=torch.float64, device=dev),
              torch.empty((P, B), dtype=torch.uint8, device=dev), torch.empty((P, B), dtype=torch.int32, device=dev),
              torch.empty((P, B), dtype=torch.float64, device=dev))
        return ts, abi.VecRolloutOut(*[x.data_ptr() for x in ts])

    roll_ts, roll_out = roll_buffers(PLANS, STEPS)
    deep_ts, deep_out = roll_buffers(1, REFILL)
    env.peek()   # (the peek tensors are there before a clock starts)
    br = env.branch(BRANCHES)

    def sync():
        eng.sync()
        torch.cuda.synchronize()

    def timed(name, launch, n=CALLS):
        sync()
        eng.kernel_timing(1)             # (clears the timers)
        for c in range(n):
            launch(c)
        eng.sync()
        ms, k = eng.kernel_time_ms(name)
        assert k == n, (name, k, n)
        eng.kernel_timing(0)
        return ms

    def peek_kernel_ms():
        return timed("vec_peek_kernel", lambda c: eng.vec_peek(abi.PEEK_ALL, env.peek_out))

    def rollout_kernel_ms():
        return timed("vec_rollout_kernel", lambda c: eng.vec_rollout(plans.data_ptr(), PLANS, STEPS, 1.0, roll_out))

    def branch_kernel_ms():
        br.fork()
        return timed("branch_step_kernel", lambda c: eng.branch_step(acts[c].data_ptr(), br.out))

    def forced_refill_ms():
        # the other legs have stepped the real books since the last refill: an untimed forced refill first (the same roll-out, whose
        # depth reaches past the schedule as soon as one real step has been taken), so that the ring is full up to the cursor ...
        eng.vec_rollout(deep.data_ptr(), 1, REFILL, 1.0, deep_out)
        env.step(policy_torch(env.obs))   # ... then ONE real step: steps_since_fill == 1, one step's worth of entries to fill
        return timed("prepass_extend_kernel", lambda c: eng.vec_rollout(deep.data_ptr(), 1, REFILL, 1.0, deep_out), n=1)

    def step_ms(with_peek):
        sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            if with_peek:
                env.peek()
            env.step(policy_torch(env.obs))
        sync()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    legs = {"vec_peek_kernel, nine actions (HIP events)": peek_kernel_ms,
            "vec_rollout_kernel P=%d H=%d (HIP events)" % (PLANS, STEPS): rollout_kernel_ms,
            "branch_step_kernel N=%d (HIP events)" % BRANCHES: branch_kernel_ms}
    if ring:
        legs["prepass_extend_kernel forced in front of a roll-out, one step's worth to fill (HIP events)"] = forced_refill_ms
    legs["VecEnv.step() (host clock, per step)"] = lambda: step_ms(False)
    legs["VecEnv.peek() + VecEnv.step() (host clock, per step)"] = lambda: step_ms(True)
    times = {k: [] for k in legs}
    for rnd in range(WARM + ROUNDS):
        for k, fn in legs.items():
            ms = fn()
            if rnd >= WARM:
                times[k].append(ms)
    rc = env.status()
    live = int((env.terminal == 0).sum())
    res = {"books": B, "track": "ring" if ring else "resident", "live_books_at_the_end": live, "lob_vec_status": rc,
           "ahead_cells": env.ahead_cells, "behind_cells": env.behind_cells, "legs_ms": {k: stat(v) for k, v in times.items()}}
    print("%d books, %s track (%d live at the end), lob_vec_status %d, ahead %d, behind %d" % (B, res["track"], live, rc, env.ahead_cells, env.behind_cells))
    for k in legs:
        v = res["legs_ms"][k]
        print("  %-100s %.4f ms (min %.4f, max %.4f)" % (k, v["median"], v["min"], v["max"]))
    br.close()
    eng.close()
    return res


results = [measure(B, ring) for B in BATCHES for ring in (True, False)]
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"depth": DEPTH, "max_trades": TRADES, "algo": "qlambda", "theta": "shared", "mid_episode_steps": MID, "rounds": ROUNDS,
                   "warm_rounds": WARM, "calls_per_window": CALLS, "ring_stream": {"replay": REPLAY, "events": EVENTS},
                   "resident_events": RESIDENT_EVENTS, "track_refill": REFILL, "plans": PLANS, "steps": STEPS, "branches": BRANCHES,
                   "runs": results}, fh, indent=1)
