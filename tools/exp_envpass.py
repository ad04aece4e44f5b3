"""The event passes of the env step as the WAVES run them, from the instrumented build (-DLOB_PROF; lob_env.h
EnvCtx::pass_top / pass_flush): passes per wave-step and the largest count in every launch, and the clocks of a pass's two
phases (23: loop top, next entry / row requested; 24: the pass) split by how many lanes were still in the loop.
Headline configuration (bench.py's: C3, 65 536 books, Q(lambda), shared theta, memory_size 20 M), one launch per td_step.
    python tools/exp_envpass.py [--steps N] [--warmup W] [--books B] [--out FILE] [--lib LIBRARY]"""
import argparse
import ctypes
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--books", type=int, default=65536)
ap.add_argument("--out", default=None)
ap.add_argument("--lib", default=None, help="an instrumented library built elsewhere, e.g. with -DLOB_PASS_RANGE=0 -DLOB_PASS_SKIPS=0 beside -DLOB_PROF")
args = ap.parse_args()

csrc = os.path.join(root, "rl_markets_amd", "csrc")
lib = args.lib or os.path.join(csrc, "_prof", "liblob_engine.so")
if not os.path.exists(lib):
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    import __graft_entry__ as ge
    ge.build_engine(lib, ("-DLOB_PROF",), os.path.join(csrc, "_prof", "_obj"))

from rl_markets_amd import abi
abi.LIB_PATH = lib
from rl_markets_amd import engine

N = 80  # LOB_PROF_N
p = engine.default_params(); p.depth, p.max_trades = 10, 2; p.algo = abi.ALGO_QLAMBDA; p.theta_mode = abi.THETA_SHARED; p.memory_size = 20000000
g = engine.default_gen_params(); g.n_events = max(64 + 2048, 64 + 6 * (args.steps + args.warmup))
eng = engine.Engine(p, args.books); eng.gen_events(g); eng.reset()
eng.lib.lob_debug_prof.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]


def read():
    out = (ctypes.c_int64 * N)()
    assert eng.lib.lob_debug_prof(eng.h, out) == 0
    return list(out)


eng.td_step(args.warmup); eng.sync()
first = prev = read()
launch_max, launch_mean = [], []
for _ in range(args.steps):
    eng.td_step(1); eng.sync()
    cur = read()
    d = [y - x for x, y in zip(prev, cur)]
    prev = cur
    if d[32]:
        launch_max.append(max(n for n in range(1, 25) if d[33 + n]))
        launch_mean.append(d[33] / d[32])
d = [y - x for x, y in zip(first, prev)]
lines = []
w = lines.append
w("env step, event passes per wave (%d books, %d launches after %d warm-up steps; clocks = clock64 ticks)" % (args.books, args.steps, args.warmup))
w("wave-steps %d, passes %d: %.2f passes per wave-step; %d of them took the general path" % (d[32], d[33], d[33] / max(d[32], 1), d[76]))
w("largest pass count of a launch: mean %.2f, min %d, max %d (24 = 24 or more)" % (sum(launch_max) / max(len(launch_max), 1), min(launch_max), max(launch_max)))
w("mean pass count of a launch's waves: %.2f .. %.2f" % (min(launch_mean), max(launch_mean)))
w("")
w("wave-steps by pass count:")
for n in range(1, 25):
    if d[33 + n]:
        w("  %2d%s passes  %9d  %6.2f %%" % (n, "+" if n == 24 else " ", d[33 + n], 100.0 * d[33 + n] / d[32]))
w("")
w("fast passes by lanes still in the loop (clocks per pass):")
w("  lanes     passes   share   phase 23   phase 24")
tot = sum(d[58:64])
for i, nm in enumerate(("64-33", "32-17", "16-9", "8-5", "4-2", "1")):
    c = d[58 + i]
    w("  %-6s %9d  %5.1f %%  %9.1f  %9.1f" % (nm, c, 100.0 * c / max(tot, 1), d[64 + i] / max(c, 1), d[70 + i] / max(c, 1)))
w("  all    %9d           %9.1f  %9.1f" % (tot, sum(d[64:70]) / max(tot, 1), sum(d[70:76]) / max(tot, 1)))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")
