"""The day library at batch scale (lob_load_days): 65 536 books draw a day per episode on the device from ~20 synthetic days
of unequal length (1 500-2 600 events, and two of 5 000-6 000: longer than the default track ring of 4 096, so the engine
runs in ring mode).  Per episode: whole-episode env-steps/s including the draw and the reset, and days_draw_kernel's time.
An episode's calls (lob_days_select, lob_reset, lob_td_step) take no host buffer: the library's bytes cross the link once, at
lob_load_days, and that figure is printed.
    python tools/exp_days.py [books] [episodes] [--out profiles/days.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rl_markets_amd import abi, engine

out_path = None
if "--out" in sys.argv:
    i = sys.argv.index("--out")
    out_path = sys.argv[i + 1]
    del sys.argv[i:i + 2]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
EPISODES = int(sys.argv[2]) if len(sys.argv) > 2 else 4
DEPTH, TRADES = 10, 2
rng = np.random.default_rng(2024)
lengths = list(rng.integers(1500, 2601, size=18)) + [5200, 5900]
days = []
for i, n in enumerate(lengths):
    g = engine.default_gen_params()
    g.n_events = int(n)
    days.append(engine.gen_stream_host(g, DEPTH, TRADES, 50000 + i, 1)[0])
p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
eng = engine.Engine(p, B)
t0 = time.perf_counter()
eng.load_days(days)
eng.sync()
lib_bytes = sum(d.nbytes for d in days)
print("library: %d days, %d-%d events, %.1f MB uploaded once in %.3f s" % (len(days), min(lengths), max(lengths), lib_bytes / 1e6,
                                                                           time.perf_counter() - t0))
eng.kernel_timing(True)
rows = []
for ep in range(EPISODES):
    c0 = eng.counters()
    a0, n0 = eng.kernel_time_ms("days_draw_kernel")   # (average over the launches so far, and their number)
    t0 = time.perf_counter()
    eng.days_select(abi.DAYS_RANDOM, 0, len(days))
    eng.reset()
    steps = 0
    while True:
        eng.td_step(64)
        steps += 64
        if eng.counters()[2] == 0 or steps >= 8192:
            break
    eng.sync()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    a1, n1 = eng.kernel_time_ms("days_draw_kernel")
    draw_ms = a1 * n1 - a0 * n0
    env_steps = int(c1[0] - c0[0])
    row = {"episode": ep, "books": B, "learner_steps": steps, "env_steps": env_steps, "seconds": dt,
           "env_steps_per_s": env_steps / dt, "days_draw_ms": draw_ms,
           "days_drawn": np.bincount(eng.days(), minlength=len(days)).tolist()}
    rows.append(row)
    print("episode %d: %d learner steps, %.3e env-steps in %.3f s = %.1f M env-steps/s (draw + reset included); days_draw_kernel %.3f ms; "
          "no host buffer handed over" % (ep, steps, env_steps, dt, env_steps / dt / 1e6, draw_ms))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"lengths": [int(x) for x in lengths], "episodes": rows}, fh, indent=1)
