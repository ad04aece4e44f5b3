"""What a look at the whole batch costs: lob_episode_stats (the reduction on the device, one 408-byte record per group back)
beside lob_get_books(0, B) (a dump per book to the host: what a caller had to do before), on the same engine and state.
65 536 books, the headline configuration, mid-episode; by_day off, and on with libraries of 22 and of 300 days.  Host clock
around each call (both end in a stream synchronise), warm, median of the repeats.
    python tools/exp_episode_stats.py [books] [--out profiles/episode_stats.json]"""
import ctypes as C
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
DEPTH, TRADES, REPEATS, DUMP_REPEATS = 10, 2, 30, 7


def median_ms(fn, repeats, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def measure(eng, by_day, label):
    lib = eng.lib
    n_rec = len(eng.episode_stats(by_day))
    out = np.zeros(n_rec, dtype=engine.EPISODE_STATS_DTYPE)
    n = C.c_int32(0)
    dumps = (abi.BookDump * eng.B)()

    def stats():
        assert lib.lob_episode_stats(eng.h, 1 if by_day else 0, out.ctypes.data_as(C.c_void_p), n_rec, C.byref(n)) == 0

    def books():
        assert lib.lob_get_books(eng.h, 0, eng.B, C.cast(dumps, C.c_void_p)) == 0

    s_med, s_min, s_max = median_ms(stats, REPEATS)
    b_med, b_min, b_max = median_ms(books, DUMP_REPEATS, warm=1)
    row = {"case": label, "books": eng.B, "records": n_rec, "bytes_to_host": n_rec * out.itemsize,
           "episode_stats_ms": {"median": s_med, "min": s_min, "max": s_max, "repeats": REPEATS},
           "get_books_ms": {"median": b_med, "min": b_min, "max": b_max, "repeats": DUMP_REPEATS},
           "get_books_bytes_to_host": eng.B * C.sizeof(abi.BookDump), "get_books_over_episode_stats": b_med / s_med,
           "n_live": int(out["n_live"][0]), "groups_with_books": int((out["n_books"][1:] > 0).sum())}
    print("%-12s %5d records: lob_episode_stats %.3f ms (min %.3f, max %.3f); lob_get_books(0, %d) %.1f ms; ratio %.0f" % (
        label, n_rec, s_med, s_min, s_max, eng.B, b_med, b_med / s_med))
    return row


p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
rows = []
for n_days in (0, 22, 300):
    eng = engine.Engine(p, B)
    if n_days:
        rng = np.random.default_rng(n_days)
        days = []
        for i, length in enumerate(rng.integers(500, 700, size=n_days)):
            g = engine.default_gen_params()
            g.n_events = int(length)
            days.append(engine.gen_stream_host(g, DEPTH, TRADES, 50000 + i, 1)[0])
        eng.load_days(days)
        eng.days_select(abi.DAYS_RANDOM, 0, n_days)
    else:
        g = engine.default_gen_params()
        g.n_events = 600
        eng.gen_events(g)
    eng.reset()
    eng.td_step(64)
    eng.sync()
    if n_days == 0:
        rows.append(measure(eng, False, "whole batch"))
    else:
        rows.append(measure(eng, True, "%d days" % n_days))
    eng.close()
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "cases": rows}, fh, indent=1)
