"""What saving and restoring the books on the device costs (lob_snapshot_save / lob_snapshot_restore): 65 536 synthetic
10-level books on one GPU, mid-episode --
  a  the HIP-event time (lob_kernel_time_ms, mean of 50 launches) of a save, of a restore with a NULL mask and of a restore with a
     mask of every second book, beside the bytes the call moves and the time those bytes take at the copy bandwidth of DESIGN.md 7e
     (6.3 TB/s);
  b  per-step host time of lob_vec_step + lob_snapshot_save against lob_vec_step alone, the actions made by a torch op enqueued on the
     engine's own stream: `steps` steps after 20 warm ones, host clock around the loop plus one final synchronise, the two legs taken
     in turn over several rounds (median, min, max) -- tools/exp_vec_env.py's method;
  c  the route one kernel replaces for the NULL-mask case: one hipMemcpyAsync per saved array on the engine's stream.  The engine's
     arrays are not exported, so the copies run between scratch buffers of the same number and sizes (the strided records -- the
     step header's five words, slot 2 of the state vectors -- counted as one plain copy each, which flatters the route); timed with
     events on that stream, mean of 50.
    python tools/exp_snapshot.py [books] [--steps 200] [--rounds 5] [--out profiles/snapshot.json]"""
import ctypes as C
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
STEPS, ROUNDS = take("--steps", 200, int), take("--rounds", 5, int)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
DEPTH, TRADES, WARM, CALLS, MID = 10, 2, 20, 50, 30
COPY_TBS = 6.3   # what a copy reaches

p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
g = engine.default_gen_params()
g.n_events = 64 + 6 * (STEPS + WARM)
# The arrays of a snapshot (lob_tu_host_vec.hip snap_prepare): 20 + 2 x 2 arrays of 4-byte and 26 + 2 x 3 of 8-byte elements [B] (the fields
# of LOB_ENV_FIELDS; cnt / head and sum / mean / s of the two rolling means), two rings [lb_pnl][B] of 8 bytes, and the per-book
# records: four 4-byte words and one 8-byte word of the step header, 64 bytes of state vector.
W = int(p.lb_pnl)
ARRAYS = [4 * B] * 24 + [8 * B] * 32 + [8 * B * W] * 2 + [4 * B] * 4 + [8 * B] + [64 * B]
PER_BOOK = sum(ARRAYS) // B


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


def start(eng, env):
    eng.reset()
    eng.vec_observe(env.out)
    eng.sync()
    torch.cuda.synchronize()


def run(eng, env, n, save):
    with torch.cuda.stream(env.stream):
        for _ in range(n):
            a = policy_torch(env.obs)
            eng.vec_step(a.data_ptr(), env.out)
            if save:
                eng.snapshot_save(0)
    eng.sync()


eng = engine.Engine(p, B)
eng.gen_events(g)
env = VecEnv(eng)     # (for its tensors and the stream handle only: the calls below go to the engine)

# ---- b: the step with and without a save behind it ----
legs = [("lob_vec_step", False), ("lob_vec_step + lob_snapshot_save", True)]
times = {name: [] for name, _ in legs}
for r in range(ROUNDS):
    for name, save in legs:
        start(eng, env)
        if save:
            eng.snapshot_save(0)   # (the slot's buffer exists from the first round on; lob_reset has voided its content)
        run(eng, env, WARM, save)
        t0 = time.perf_counter()
        run(eng, env, STEPS, save)
        times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)

# ---- a: the kernels alone, HIP events, mid-episode ----
start(eng, env)
run(eng, env, MID, False)
live = int((eng.get_terminal() == 0).sum())
half = (torch.arange(B, device="cuda") % 2 == 0).to(torch.uint8)
torch.cuda.synchronize()
eng.snapshot_save(0)
calls = [("save, NULL mask", "snapshot_all_kernel", lambda: eng.snapshot_save(0), 1.0),
         ("restore, NULL mask", "snapshot_all_kernel", lambda: eng.snapshot_restore(0), 1.0),
         ("restore, every second book", "snapshot_masked_kernel", lambda: eng.snapshot_restore(0, half.data_ptr()), 0.5)]
kern = []
for name, kernel, fn, share in calls:
    for _ in range(5):
        fn()
    eng.kernel_timing(1)          # (clears the timers)
    for _ in range(CALLS):
        fn()
    eng.sync()
    ms, n = eng.kernel_time_ms(kernel)
    moved = int(2 * PER_BOOK * B * share + (B if share < 1 else 0))    # read + written, and the mask bytes
    kern.append({"call": name, "kernel": kernel, "avg_ms": ms, "launches": n, "bytes_moved": moved,
                 "ms_at_copy_bandwidth": moved / (COPY_TBS * 1e9), "TB_per_s": moved / (ms * 1e9) if ms > 0 else None})
eng.kernel_timing(0)

# ---- c: one hipMemcpyAsync per array ----
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
src = [torch.zeros(max(n, 16), dtype=torch.uint8, device="cuda") for n in ARRAYS]
dst = [torch.zeros(max(n, 16), dtype=torch.uint8, device="cuda") for n in ARRAYS]
torch.cuda.synchronize()
stream = C.c_void_p(eng.lob_stream())
D2D = 3


def copies():
    for s, d, n in zip(src, dst, ARRAYS):
        assert hip.hipMemcpyAsync(d.data_ptr(), s.data_ptr(), n, D2D, stream) == 0


route = []
with torch.cuda.stream(env.stream):
    for _ in range(5):
        copies()
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        copies()
        e1.record()
        route.append((e0, e1))
eng.sync()
route_ms = [a.elapsed_time(b) for a, b in route]
rc = env.status()
eng.close()

rows = []
for name, _ in legs:
    t = times[name]
    rows.append({"leg": name, "step_ms": {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": ROUNDS, "all": t}})
    print("%-36s per step %.4f ms (min %.4f, max %.4f)" % (name, rows[-1]["step_ms"]["median"], min(t), max(t)))
for k in kern:
    print("%-28s %-24s %.4f ms x %d launches; %.1f MB moved = %.4f ms at %.1f TB/s; reached %.2f TB/s"
          % (k["call"], k["kernel"], k["avg_ms"], k["launches"], k["bytes_moved"] / 1e6, k["ms_at_copy_bandwidth"], COPY_TBS, k["TB_per_s"] or 0))
print("%d x hipMemcpyAsync, NULL-mask case: %.4f ms per call (min %.4f, max %.4f)" % (len(ARRAYS), float(np.mean(route_ms)), min(route_ms), max(route_ms)))
print("%d bytes per book, %.1f MB per slot; live books mid-episode: %d of %d; lob_vec_status %d" % (PER_BOOK, PER_BOOK * B / 1e6, live, B, rc))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "max_trades": TRADES, "lb_pnl": W, "steps": STEPS, "warm": WARM, "bytes_per_book": PER_BOOK,
                   "legs": rows, "kernel_hip_events": kern, "copy_bandwidth_TB_per_s": COPY_TBS,
                   "memcpy_route_ms": {"copies": len(ARRAYS), "mean": float(np.mean(route_ms)), "min": min(route_ms), "max": max(route_ms), "calls": CALLS},
                   "live_books_mid_episode": live, "lob_vec_status": rc}, fh, indent=1)
