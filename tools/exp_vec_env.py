"""What one agent step of an EXTERNAL policy costs through the two environment faces: 65 536 synthetic 10-level books, the action an
exact function of the previous observation, three legs on engines built alike --
  a  the host-bound face: lob_step + lob_get_state + lob_get_reward + lob_get_terminal, the actions made on the host (numpy);
  b  lob_vec_step on raw device addresses, the actions made by a torch op enqueued on the engine's own stream;
  c  the same through rl_markets_amd.vec_env.VecEnv (torch's current stream and the engine's, ordered by events on the device).
Per leg: the per-step host time of `steps` steps, host clock around the loop plus one final synchronise, warm, the legs taken in
turn over several rounds (median, min, max) -- tools/exp_step_log.py's method.  In a run of its own with kernel timing on, the
HIP-event times of vec_actions_kernel, env_kernel and vec_observe_kernel.
    python tools/exp_vec_env.py [books] [--steps 200] [--rounds 5] [--out profiles/vec_env.json]"""
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
DEPTH, TRADES, WARM = 10, 2, 20

p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
g = engine.default_gen_params()
g.n_events = 64 + 6 * (STEPS + WARM)
V = p.n_vars


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


def policy_numpy(obs):
    bits = obs.view(np.int32)
    return np.mod((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5), 9).astype(np.int32)


class LegA:
    name = "a: lob_step + getters, host actions"

    def __init__(self):
        self.eng = engine.Engine(p, B)
        self.eng.gen_events(g)

    def start(self):
        self.eng.reset()
        self.obs = self.eng.get_state()

    def run(self, n):
        eng, obs = self.eng, self.obs
        for _ in range(n):
            eng.step(policy_numpy(obs))
            obs = eng.get_state()
            eng.get_reward()
            eng.get_terminal()
        self.obs = obs
        eng.sync()


class LegB:
    name = "b: lob_vec_step, torch actions on the engine's stream"

    def __init__(self):
        self.eng = engine.Engine(p, B)
        self.eng.gen_events(g)
        self.env = VecEnv(self.eng)      # (for its tensors and the stream handle only: the calls below go to the engine)
        self.stream = self.env.stream

    def start(self):
        self.env.reset()
        torch.cuda.synchronize()

    def run(self, n):
        eng, env = self.eng, self.env
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                a = policy_torch(env.obs)
                eng.vec_step(a.data_ptr(), env.out)
        eng.sync()


class LegC:
    name = "c: VecEnv.step"

    def __init__(self):
        self.eng = engine.Engine(p, B)
        self.eng.gen_events(g)
        self.env = VecEnv(self.eng)

    def start(self):
        self.obs = self.env.reset()
        torch.cuda.synchronize()

    def run(self, n):
        env, obs = self.env, self.obs
        for _ in range(n):
            obs, _, _, _ = env.step(policy_torch(obs))
        torch.cuda.synchronize()
        self.eng.sync()


legs = [LegA(), LegB(), LegC()]
times = {leg.name: [] for leg in legs}
for r in range(ROUNDS):
    for leg in legs:
        leg.start()
        leg.run(WARM)
        t0 = time.perf_counter()
        leg.run(STEPS)
        times[leg.name].append((time.perf_counter() - t0) * 1e3 / STEPS)

# the three legs have played the same episode: same actions from the same observations
finals = [np.frombuffer(bytes(leg.eng.get_books()), dtype=np.uint8) for leg in legs]
same = all(np.array_equal(finals[0], f) for f in finals[1:])
live = int((legs[0].eng.get_terminal() == 0).sum())

kern = {}
leg = legs[2]
leg.eng.kernel_timing(1)
leg.start()
leg.run(WARM + 40)
for k in ("vec_actions_kernel", "env_kernel", "vec_observe_kernel"):
    ms, n = leg.eng.kernel_time_ms(k)
    kern[k] = {"avg_ms": ms, "launches": n}
leg.eng.kernel_timing(0)
rc = leg.env.status()

rows = []
for leg in legs:
    t = times[leg.name]
    rows.append({"leg": leg.name, "step_ms": {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": ROUNDS, "all": t}})
    print("%-55s per step %.4f ms (min %.4f, max %.4f)" % (leg.name, rows[-1]["step_ms"]["median"], min(t), max(t)))
for k, v in kern.items():
    print("%-22s %.4f ms x %d launches" % (k, v["avg_ms"], v["launches"]))
print("final books of the three legs identical: %s; live books at the end: %d of %d; lob_vec_status %d" % (same, live, B, rc))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "steps": STEPS, "warm": WARM, "n_vars": V, "legs": rows, "kernels_hip_events": kern,
                   "bytes_over_pcie_per_step_leg_a": B * 4 + B * V * 4 + B * 8 + 2 * B * 4,
                   "legs_end_in_identical_books": bool(same), "live_books_at_end": live, "lob_vec_status": rc}, fh, indent=1)
for leg in legs:
    leg.eng.close()
