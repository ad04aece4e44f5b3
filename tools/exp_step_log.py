"""What the step log (lob_step_log_*) costs the step: the headline configuration (65 536 synthetic 10-level books, Q(lambda), one
shared weight vector) stepped in three states -- log off, 64 books logged, all books logged -- on engines built alike.  Per
state: the per-step time of lob_td_step(steps) by the host clock around call + synchronise, warm, the states taken in turn over
several rounds (median, min, max), and in a run of its own with kernel timing on the average time of step_log_kernel.
    python tools/exp_step_log.py [books] [--steps 200] [--rounds 5] [--off-only] [--out profiles/step_log.json]
--off-only: the log-off state alone, through nothing but the calls the engine had before the log existed (to time a build
without it beside this one)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rl_markets_amd import abi, engine


def take(flag, default=None, cast=str):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        v = cast(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


out_path = take("--out")
STEPS, ROUNDS = take("--steps", 200, int), take("--rounds", 5, int)
off_only = "--off-only" in sys.argv
if off_only:
    sys.argv.remove("--off-only")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
DEPTH, TRADES, WARM = 10, 2, 20

p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
g = engine.default_gen_params()
g.n_events = 64 + 6 * (STEPS + WARM)

states = [("off", 0)] if off_only else [("off", 0), ("64 books", 64), ("all books", B)]
engines = {}
for name, n_sel in states:
    eng = engine.Engine(p, B)
    eng.gen_events(g)
    if n_sel:
        eng.step_log_enable(None if n_sel == B else np.arange(0, B, B // n_sel, dtype=np.int32)[:n_sel], STEPS + WARM)
    engines[name] = eng

times = {name: [] for name, _ in states}
for r in range(ROUNDS):
    for name, _ in states:
        eng = engines[name]
        eng.reset()
        eng.td_step(WARM)
        eng.sync()
        t0 = time.perf_counter()
        eng.td_step(STEPS)
        eng.sync()
        times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)

rows = []
for name, n_sel in states:
    eng = engines[name]
    eng.kernel_timing(1)
    eng.reset()
    eng.td_step(WARM + 40)
    eng.sync()
    k_ms, k_n = eng.kernel_time_ms("step_log_kernel")
    eng.kernel_timing(0)
    live = int(eng.counters()[2])
    row = {"state": name, "books_logged": n_sel, "step_ms": {"median": float(np.median(times[name])), "min": min(times[name]),
                                                            "max": max(times[name]), "rounds": ROUNDS, "all": times[name]},
           "step_log_kernel": {"avg_ms": k_ms, "launches": k_n}, "bytes_per_step": n_sel * 96, "live_books_at_end": live}
    if n_sel:
        n_rows, n_lost = eng.step_log_counts()
        row["rows_stored"], row["rows_lost"] = int(n_rows.sum()), int(n_lost.sum())
    rows.append(row)
    eng.close()
base = rows[0]["step_ms"]["median"]
for row in rows:
    row["ratio_to_off"] = row["step_ms"]["median"] / base
    print("%-10s per step %.4f ms (min %.4f, max %.4f) x%.3f of off; step_log_kernel %.4f ms x %d launches" % (
        row["state"], row["step_ms"]["median"], row["step_ms"]["min"], row["step_ms"]["max"], row["ratio_to_off"],
        row["step_log_kernel"]["avg_ms"], row["step_log_kernel"]["launches"]))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "steps": STEPS, "warm": WARM, "states": rows}, fh, indent=1)
