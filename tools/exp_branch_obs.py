"""What the book and the event window of a branch set cost (lob_branch_book / lob_branch_history): synthetic 10-level
books on one GPU, two trade slots, the books `--mid` random steps into the episode, the branches four random steps apart --
  a  the HIP-event time (lob_kernel_time_ms) of branch_book_kernel for N = 1, 9, 32 and of branch_hist_kernel for N = 9 at K = 8 and
     32, beside the project's own yardstick taken in the same process on the real books of the same engine: N x the time of
     vec_book_kernel, resp. of vec_hist_kernel at the same K -- the same bytes per row;
  b  Branches.step() for N = 9 with and without book=True, history=8 as a caller sees it: host clock around `--calls` calls plus one
     synchronise;
  c  the closed loop of 7l (N = 9, H = 4) with the book and an 8-record window kept at every step: fork + H x (policy,
     Branches.step(), clones), beside the composed snapshot route that produces the same tensors through the same VecEnv: save(1),
     then nine times (H x (policy, step(), clones) and restore(1)); host clock around one route plus one synchronise.
All legs are taken in turn, once per round, in this one process; median, min and max over `--rounds` rounds (after `--warm` untimed
ones).  Before the rounds the tensors of the two routes are compared for equality.
    python tools/exp_branch_obs.py [books ...] [--rounds 5] [--warm 1] [--calls 5] [--mid 30] [--out profiles/branch_obs.json]"""
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
ROUNDS, WARM, CALLS, MID = take("--rounds", 5, int), take("--warm", 1, int), take("--calls", 5, int), take("--mid", 30, int)
BATCHES = [int(x) for x in sys.argv[1:]] or [65536, 4096]
DEPTH, TRADES, NA = 10, 2, abi.LOB_N_ACTIONS
BOOK_SIZES = [1, 9, 32]
HIST = [(9, 8), (9, 32)]
ROUTE = (9, 4)
ROUTE_K = 8
KEPT = ("levels", "own", "time_ms", "hist_levels", "hist_trades", "hist_time_ms", "hist_valid", "hist_rec")


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
    env = VecEnv(eng, book=True, history=ROUTE_K)
    dev = env.device
    env.reset()
    for _ in range(MID):
        env.step(policy_torch(env.obs))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    n_max = max(BOOK_SIZES)
    apart = torch.randint(0, NA, (4, n_max, B), generator=gen, device=dev, dtype=torch.int32)
    acts9 = torch.randint(0, NA, (CALLS, 9, B), generator=gen, device=dev, dtype=torch.int32)

    def sync():
        eng.sync()
        torch.cuda.synchronize()

    def book_tensors(n):
        t = (torch.empty((n, B, 4, DEPTH), dtype=torch.float32, device=dev), torch.empty((n, B, abi.VEC_OWN_WORDS), dtype=torch.float32, device=dev),
             torch.empty((n, B), dtype=torch.int64, device=dev))
        return t, abi.VecBookOut(*[x.data_ptr() for x in t])

    def hist_tensors(n, K):
        t = (torch.empty((n, B, K, 4, DEPTH), dtype=torch.float32, device=dev), torch.empty((n, B, K, 2, TRADES), dtype=torch.float32, device=dev),
             torch.empty((n, B, K), dtype=torch.int32, device=dev), torch.empty((n, B), dtype=torch.int32, device=dev),
             torch.empty((n, B), dtype=torch.int32, device=dev))
        return t, abi.VecHistOut(*[x.data_ptr() for x in t])

    bufs_book = {n: book_tensors(n) for n in BOOK_SIZES}
    bufs_hist = {(n, K): hist_tensors(n, K) for n, K in HIST}
    real_book = book_tensors(1)
    real_hist = {K: hist_tensors(1, K) for K in sorted({K for _, K in HIST})}

    def apart_set(n):
        """a fresh set of n branches, four random steps apart"""
        br = env.branch(n)
        for h in range(4):
            br.step(apart[h, :n].contiguous())
        return br

    def timed(name, fn):
        sync()
        eng.kernel_timing(1)             # (clears the timers)
        for _ in range(CALLS):
            fn()
        eng.sync()
        ms, k = eng.kernel_time_ms(name)
        assert k == CALLS, (name, k)
        eng.kernel_timing(0)
        return ms

    def branch_book_ms(n):
        apart_set(n)
        return timed("branch_book_kernel", lambda: eng.branch_book(bufs_book[n][1]))

    def branch_hist_ms(n, K):
        apart_set(n)
        return timed("branch_hist_kernel", lambda: eng.branch_history(K, bufs_hist[(n, K)][1]))

    def step_ms(**kw):
        br = env.branch(9, **kw)
        sync()
        t0 = time.perf_counter()
        for c in range(CALLS):
            br.step(acts9[c])
        sync()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    def composed():
        N, H = ROUTE
        env.save(1)
        kept = []
        for q in range(N):
            o = env.obs
            for h in range(H):
                o, r, t, s = env.step(policy_torch(o))
                kept.append({k: getattr(env, k).clone() for k in KEPT})
            env.restore(1)
        return kept   # [q * H + h]

    def closed_loop(br):
        N, H = ROUTE
        o = br.fork()[0]
        kept = []
        for h in range(H):
            o, r, t, s = br.step(policy_torch(o))
            kept.append({k: getattr(br, k).clone() for k in KEPT})
        return kept   # [h]

    br9 = env.branch(ROUTE[0], book=True, history=ROUTE_K)
    a, b = closed_loop(br9), composed()
    equal = all(torch.equal(a[h][k][q].view(torch.uint8), b[q * ROUTE[1] + h][k].view(torch.uint8))
                for q in range(ROUTE[0]) for h in range(ROUTE[1]) for k in KEPT)
    del a, b
    live = int((env.terminal == 0).sum())
    sync()

    def composed_ms():
        sync()
        t0 = time.perf_counter()
        composed()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def closed_loop_ms():
        br = env.branch(ROUTE[0], book=True, history=ROUTE_K)
        sync()
        t0 = time.perf_counter()
        closed_loop(br)
        sync()
        return (time.perf_counter() - t0) * 1e3

    legs = {"vec_book_kernel, the real books (HIP events)": lambda: timed("vec_book_kernel", lambda: eng.vec_book(real_book[1]))}
    for K in real_hist:
        legs["vec_hist_kernel K=%d, the real books (HIP events)" % K] = lambda K=K: timed("vec_hist_kernel", lambda: eng.vec_history(K, real_hist[K][1]))
    for n in BOOK_SIZES:
        legs["branch_book_kernel N=%d (HIP events)" % n] = lambda n=n: branch_book_ms(n)
    for n, K in HIST:
        legs["branch_hist_kernel N=%d K=%d (HIP events)" % (n, K)] = lambda n=n, K=K: branch_hist_ms(n, K)
    legs["Branches.step() N=9 (host clock, per call)"] = lambda: step_ms()
    legs["Branches.step() N=9 book=True history=8 (host clock, per call)"] = lambda: step_ms(book=True, history=8)
    route_key = "composed snapshot route N=%d H=%d, book + K=8 window kept at every step (host clock, per route)" % ROUTE
    loop_key = "branch closed loop N=%d H=%d, book + K=8 window kept at every step (host clock, per route)" % ROUTE
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
    L = res["legs_ms"]
    row_book = 4 * (4 * DEPTH + abi.VEC_OWN_WORDS) + 8          # bytes written per (branch, book)
    res["against_the_yardstick"] = {}
    yb = L["vec_book_kernel, the real books (HIP events)"]
    for n in BOOK_SIZES:
        v = L["branch_book_kernel N=%d (HIP events)" % n]
        res["against_the_yardstick"]["branch_book_kernel N=%d" % n] = {
            "yardstick_ms_N_x_vec_book_kernel": {"median": n * yb["median"], "min": n * yb["min"], "max": n * yb["max"]},
            "ratio_of_medians": v["median"] / (n * yb["median"]), "bytes_written": n * B * row_book,
            "implied_GB_per_s_written": n * B * row_book / (v["median"] * 1e-3) / 1e9}
    for n, K in HIST:
        v, yh = L["branch_hist_kernel N=%d K=%d (HIP events)" % (n, K)], L["vec_hist_kernel K=%d, the real books (HIP events)" % K]
        row = 4 * (4 * DEPTH + 2 * TRADES + 1)
        res["against_the_yardstick"]["branch_hist_kernel N=%d K=%d" % (n, K)] = {
            "yardstick_ms_N_x_vec_hist_kernel": {"median": n * yh["median"], "min": n * yh["min"], "max": n * yh["max"]},
            "ratio_of_medians": v["median"] / (n * yh["median"]), "bytes_written": n * B * (K * row + 8),
            "implied_GB_per_s_written": n * B * (K * row + 8) / (v["median"] * 1e-3) / 1e9}
    res["composed_route_over_branch_route"] = L[route_key]["median"] / L[loop_key]["median"]
    print("%d books (%d live), closed loop == composed route: %s, lob_vec_status %d" % (B, live, equal, rc))
    for k in legs:
        v = L[k]
        print("  %-110s %.4f ms (min %.4f, max %.4f)" % (k, v["median"], v["min"], v["max"]))
    for k, v in res["against_the_yardstick"].items():
        y = list(v.values())[0]
        print("  %-32s / yardstick %.4f ms (%.4f - %.4f) = %.3f; %.0f GB/s written" % (k, y["median"], y["min"], y["max"], v["ratio_of_medians"],
                                                                                      v["implied_GB_per_s_written"]))
    print("  composed route / branch route = %.1f" % res["composed_route_over_branch_route"])
    eng.close()
    return res


results = [measure(B) for B in BATCHES]
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"depth": DEPTH, "max_trades": TRADES, "algo": "qlambda", "theta": "shared", "mid_episode_steps": MID, "rounds": ROUNDS,
                   "warm_rounds": WARM, "calls_per_window": CALLS, "book_sizes": BOOK_SIZES, "hist": HIST, "route": ROUTE, "route_K": ROUTE_K,
                   "batches": results}, fh, indent=1)
