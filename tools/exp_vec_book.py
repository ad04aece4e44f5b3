"""What the order-book observation of the vector-env interface costs (lob_vec_book): 65 536 synthetic 10-level books on
one GPU, one engine --
  a  the HIP-event time of vec_book_kernel (lob_kernel_time_ms) with all three outputs, and with each output NULLed in turn;
  b  per-step host time of lob_vec_step + lob_vec_book against lob_vec_step alone, the actions made by a torch op enqueued on the
     engine's own stream: `steps` steps after 20 warm ones, host clock around the loop plus one final synchronise, the two legs taken
     in turn over several rounds (median, min, max) -- tools/exp_vec_env.py's method;
  c  the only previous route to the same tensors: lob_get_books(0, B) + numpy re-pack + upload.
The bytes the kernel has to move are computed from the shapes; the tensors of (a) are compared with those of (c).
    python tools/exp_vec_book.py [books] [--steps 200] [--rounds 5] [--out profiles/vec_book.json]"""
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
DEPTH, TRADES, WARM, KERNEL_CALLS, BASELINE_CALLS = 10, 2, 20, 100, 5

p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
g = engine.default_gen_params()
g.n_events = 64 + 6 * (STEPS + WARM)
BOOK_DTYPE = np.dtype([(n, np.dtype(t._type_), (t._length_,)) if issubclass(t, C.Array) else (n, np.dtype(t)) for n, t in abi.BookDump._fields_], align=True)
assert BOOK_DTYPE.itemsize == C.sizeof(abi.BookDump)


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


eng = engine.Engine(p, B)
eng.gen_events(g)
env = VecEnv(eng, book=True)     # (for its tensors and the stream handle only: the calls below go to the engine)
book_all = env.book_out


def start():
    eng.reset()
    eng.vec_observe(env.out)
    eng.sync()
    torch.cuda.synchronize()


def run(n, with_book):
    with torch.cuda.stream(env.stream):
        for _ in range(n):
            a = policy_torch(env.obs)
            eng.vec_step(a.data_ptr(), env.out)
            if with_book:
                eng.vec_book(book_all)
    eng.sync()


# ---- b: the step with and without the book ----
legs = [("lob_vec_step", False), ("lob_vec_step + lob_vec_book", True)]
times = {name: [] for name, _ in legs}
for r in range(ROUNDS):
    for name, with_book in legs:
        start()
        run(WARM, with_book)
        t0 = time.perf_counter()
        run(STEPS, with_book)
        times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)

# ---- a: the kernel alone, HIP events ----
variants = {"all three outputs": book_all,
            "levels NULL": abi.VecBookOut(None, book_all.own, book_all.time_ms),
            "own NULL": abi.VecBookOut(book_all.levels, None, book_all.time_ms),
            "time_ms NULL": abi.VecBookOut(book_all.levels, book_all.own, None)}
kern = {}
for name, out in variants.items():
    for _ in range(10):
        eng.vec_book(out)
    eng.kernel_timing(1)          # (clears the timers)
    for _ in range(KERNEL_CALLS):
        eng.vec_book(out)
    eng.sync()
    ms, n = eng.kernel_time_ms("vec_book_kernel")
    kern[name] = {"avg_ms": ms, "launches": n}
eng.kernel_timing(0)


# ---- c: the previous route ----
def previous_route():
    d = np.frombuffer(bytes(eng.get_books(0, B)), dtype=BOOK_DTYPE)
    lv = np.stack([d["ask_px"][:, :DEPTH], d["ask_vol"][:, :DEPTH], d["bid_px"][:, :DEPTH], d["bid_vol"][:, :DEPTH]], axis=1).astype(np.float32)
    own = np.stack([d[f].astype(np.float32) for f in abi.OWN_FIELDS], axis=1)
    out = torch.from_numpy(lv).cuda(), torch.from_numpy(own).cuda(), torch.from_numpy(d["time_ms"].astype(np.int64)).cuda()
    torch.cuda.synchronize()
    return out


previous_route()
base = []
for _ in range(BASELINE_CALLS):
    t0 = time.perf_counter()
    prev = previous_route()
    base.append((time.perf_counter() - t0) * 1e3)
eng.vec_book(book_all)
eng.sync()
same = all(bool(torch.equal(a, b)) for a, b in zip(prev, (env.levels, env.own, env.time_ms)))
live = int((eng.get_terminal() == 0).sum())
rc = env.status()

Wd = 4 + 4 * ((DEPTH + 3) // 4 * 4) + (2 * TRADES + 3) // 4 * 4
bytes_in = {"record_rows": B * Wd * 4, "level_words_used": B * 4 * DEPTH * 4, "field_arrays": B * (7 * 8 + 5 * 4 + 7 * 8), "rec_cur": B * 4}
bytes_out = {"levels": B * 4 * DEPTH * 4, "own": B * 64, "time_ms": B * 8}
rows = []
for name, _ in legs:
    t = times[name]
    rows.append({"leg": name, "step_ms": {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": ROUNDS, "all": t}})
    print("%-32s per step %.4f ms (min %.4f, max %.4f)" % (name, rows[-1]["step_ms"]["median"], min(t), max(t)))
for k, v in kern.items():
    print("vec_book_kernel, %-18s %.4f ms x %d launches" % (k, v["avg_ms"], v["launches"]))
moved = sum(bytes_out.values()) + bytes_in["record_rows"] + bytes_in["field_arrays"] + bytes_in["rec_cur"]
print("bytes per call: %.1f MB (whole record rows counted); previous route %.1f ms per call (min %.1f, max %.1f)"
      % (moved / 1e6, float(np.median(base)), min(base), max(base)))
print("tensors equal to the previous route's: %s; live books at the end: %d of %d; lob_vec_status %d" % (same, live, B, rc))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "max_trades": TRADES, "steps": STEPS, "warm": WARM, "legs": rows, "kernel_hip_events": kern,
                   "bytes_in": bytes_in, "bytes_out": bytes_out,
                   "previous_route_ms": {"median": float(np.median(base)), "min": min(base), "max": max(base), "calls": BASELINE_CALLS, "all": base},
                   "tensors_equal_previous_route": bool(same), "live_books_at_end": live, "lob_vec_status": rc}, fh, indent=1)
eng.close()
