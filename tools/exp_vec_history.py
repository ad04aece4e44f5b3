"""What the event-record window of the vector-env interface costs (lob_vec_history): 65 536 synthetic 10-level books
with two trade slots on one GPU --
  a  the HIP-event time of vec_hist_kernel (lob_kernel_time_ms) for K = 8, 32 and 100, with all five outputs and with `levels`
     only, beside the bytes the call moves and the time those bytes take at the copy bandwidth of DESIGN.md 7e (6.3 TB/s);
  b  per-step host time of lob_vec_step + lob_vec_history(32) against lob_vec_step alone, the actions made by a torch op enqueued on
     the engine's own stream: `steps` steps after 20 warm ones, host clock around the loop plus one final synchronise, the two legs
     taken in turn over several rounds (median, min, max) -- tools/exp_vec_env.py's method;
  c  the only previous route to the same tensors, on a second engine whose streams are short enough for a host copy: lob_get_books
     for the cursor, an index into the host copy of the streams, a numpy re-pack and an upload, K = 32.  Its tensors are compared
     with the kernel's.
    python tools/exp_vec_history.py [books] [--steps 200] [--rounds 5] [--out profiles/vec_history.json]"""
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
DEPTH, TRADES, WARM, KERNEL_CALLS, BASELINE_CALLS, K_STEP = 10, 2, 20, 50, 3, 32
KS = (8, 32, 100)
COPY_TBS = 6.3   # what a copy reaches
Wd = 4 + 4 * ((DEPTH + 3) // 4 * 4) + (2 * TRADES + 3) // 4 * 4

p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
g = engine.default_gen_params()
g.n_events = 64 + 6 * (STEPS + WARM)
BOOK_DTYPE = np.dtype([(n, np.dtype(t._type_), (t._length_,)) if issubclass(t, C.Array) else (n, np.dtype(t)) for n, t in abi.BookDump._fields_], align=True)
assert BOOK_DTYPE.itemsize == C.sizeof(abi.BookDump)


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


def start(eng, env):
    eng.reset()
    eng.vec_observe(env.out)
    eng.sync()
    torch.cuda.synchronize()


def run(eng, env, n, hist):
    with torch.cuda.stream(env.stream):
        for _ in range(n):
            a = policy_torch(env.obs)
            eng.vec_step(a.data_ptr(), env.out)
            if hist is not None:
                eng.vec_history(K_STEP, hist)
    eng.sync()


eng = engine.Engine(p, B)
eng.gen_events(g)
env = VecEnv(eng, history=K_STEP)     # (for its tensors and the stream handle only: the calls below go to the engine)

# ---- b: the step with and without the window ----
legs = [("lob_vec_step", None), ("lob_vec_step + lob_vec_history(%d)" % K_STEP, env.hist_out)]
times = {name: [] for name, _ in legs}
for r in range(ROUNDS):
    for name, hist in legs:
        start(eng, env)
        run(eng, env, WARM, hist)
        t0 = time.perf_counter()
        run(eng, env, STEPS, hist)
        times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
live = int((eng.get_terminal() == 0).sum())

# ---- a: the kernel alone, HIP events ----
kern = []
for K in KS:
    lv = torch.zeros((B, K, 4, DEPTH), dtype=torch.float32, device="cuda")
    tr = torch.zeros((B, K, 2, TRADES), dtype=torch.float32, device="cuda")
    tm = torch.zeros((B, K), dtype=torch.int32, device="cuda")
    nv, rc_ = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    variants = {"all five outputs": abi.VecHistOut(lv.data_ptr(), tr.data_ptr(), tm.data_ptr(), nv.data_ptr(), rc_.data_ptr()),
                "levels only": abi.VecHistOut(lv.data_ptr(), None, None, None, None)}
    for name, out in variants.items():
        for _ in range(5):
            eng.vec_history(K, out)
        eng.kernel_timing(1)          # (clears the timers)
        for _ in range(KERNEL_CALLS):
            eng.vec_history(K, out)
        eng.sync()
        ms, n = eng.kernel_time_ms("vec_hist_kernel")
        n_valid = int(nv.sum().item())
        rows = B * K
        b_in = n_valid * Wd * 4 + B * 4                      # the records of the valid slots, whole; rec_cur
        b_out = rows * 4 * DEPTH * 4 + (rows * (2 * TRADES + 1) * 4 + B * 8 if name == "all five outputs" else 0)
        kern.append({"K": K, "outputs": name, "avg_ms": ms, "launches": n, "valid_slots": n_valid, "bytes_in": b_in, "bytes_out": b_out,
                     "ms_at_copy_bandwidth": (b_in + b_out) / (COPY_TBS * 1e9), "TB_per_s": (b_in + b_out) / (ms * 1e9) if ms > 0 else None})
    del lv, tr, tm, nv, rc_
eng.kernel_timing(0)
rc = env.status()
eng.close()

# ---- c: the previous route, K_STEP, on streams short enough to keep a host copy of ----
g2 = engine.default_gen_params()
g2.n_events = 160
eng2 = engine.Engine(p, B)
eng2.gen_events(g2)
host = engine.gen_stream_host(g2, DEPTH, TRADES, int(p.book_id_offset), B)     # [B][n][W]: the copy the route needs
env2 = VecEnv(eng2, history=K_STEP)
start(eng2, env2)
run(eng2, env2, 12, None)
kk = np.arange(K_STEP)
o = 2 + 4 * DEPTH


def previous_route():
    dump = np.frombuffer(bytes(eng2.get_books(0, B)), dtype=BOOK_DTYPE)
    r = dump["cursor"].astype(np.int64) - 1                                    # (every book is live here: cursor - 1 is the record)
    idx = r[:, None] - (K_STEP - 1 - kk)[None, :]
    have = idx >= 0
    rows = np.where(have[:, :, None], host[np.arange(B)[:, None], np.maximum(idx, 0)], np.uint32(0))
    lvw = rows[:, :, 2:o].reshape(B, K_STEP, 4, DEPTH)
    lv = np.empty((B, K_STEP, 4, DEPTH), np.float32)
    lv[:, :, 0::2] = lvw[:, :, 0::2].view(np.float32)
    lv[:, :, 1::2] = lvw[:, :, 1::2].view(np.int32)
    tr = np.stack([np.ascontiguousarray(rows[:, :, o:o + TRADES]).view(np.float32),
                   np.ascontiguousarray(rows[:, :, o + TRADES:o + 2 * TRADES]).view(np.int32).astype(np.float32)], axis=2)
    tm = np.ascontiguousarray(rows[:, :, 0]).view(np.int32)
    out = (torch.from_numpy(lv).cuda(), torch.from_numpy(tr).cuda(), torch.from_numpy(tm).cuda(),
           torch.from_numpy(np.minimum(K_STEP, r + 1).astype(np.int32)).cuda(), torch.from_numpy(r.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    return out


assert (eng2.get_terminal() == 0).all()
previous_route()
base = []
for _ in range(BASELINE_CALLS):
    t0 = time.perf_counter()
    prev = previous_route()
    base.append((time.perf_counter() - t0) * 1e3)
eng2.vec_history(K_STEP, env2.hist_out)
eng2.sync()
torch.cuda.synchronize()
same = all(bool(torch.equal(a, b)) for a, b in zip(prev, (env2.hist_levels, env2.hist_trades, env2.hist_time_ms, env2.hist_valid, env2.hist_rec)))
eng2.close()

rows = []
for name, _ in legs:
    t = times[name]
    rows.append({"leg": name, "step_ms": {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": ROUNDS, "all": t}})
    print("%-40s per step %.4f ms (min %.4f, max %.4f)" % (name, rows[-1]["step_ms"]["median"], min(t), max(t)))
for k in kern:
    print("vec_hist_kernel K=%3d %-17s %.4f ms x %d launches; %.1f MB in + %.1f MB out = %.4f ms at %.1f TB/s; reached %.2f TB/s"
          % (k["K"], k["outputs"], k["avg_ms"], k["launches"], k["bytes_in"] / 1e6, k["bytes_out"] / 1e6, k["ms_at_copy_bandwidth"], COPY_TBS, k["TB_per_s"] or 0))
print("previous route, K = %d: %.1f ms per call (min %.1f, max %.1f); tensors equal to the kernel's: %s" % (K_STEP, float(np.median(base)), min(base), max(base), same))
print("live books at the end of (b): %d of %d; lob_vec_status %d" % (live, B, rc))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "max_trades": TRADES, "steps": STEPS, "warm": WARM, "legs": rows, "kernel_hip_events": kern,
                   "copy_bandwidth_TB_per_s": COPY_TBS,
                   "previous_route_ms": {"K": K_STEP, "n_events": g2.n_events, "median": float(np.median(base)), "min": min(base), "max": max(base),
                                         "calls": BASELINE_CALLS, "all": base},
                   "tensors_equal_previous_route": bool(same), "live_books_at_end": live, "lob_vec_status": rc}, fh, indent=1)
