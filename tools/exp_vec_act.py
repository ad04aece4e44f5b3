"""What the engine's own policy costs on the vector-env interface (lob_vec_act): 65 536 synthetic 10-level books on one
GPU, Q(lambda), one weight vector shared by all books, the weights as `--train` learner steps leave them --
  a  the HIP-event time of vec_act_kernel (lob_kernel_time_ms), mode greedy, for q only, action only and both;
  b  per-step host time of lob_vec_act + lob_vec_step against lob_vec_step alone (there the actions are made by a torch op enqueued on
     the engine's own stream): `steps` steps after 20 warm ones, host clock around the loop plus one final synchronise, the two legs
     taken in turn over several rounds (median, min, max) -- tools/exp_vec_env.py's method;
  c  the route it replaces: D2H of obs, lob_q_values, argmax on the host, upload of the actions;
  d  the act_kernel time of lob_eval_step on a second engine created under LOB_NO_MEMO=1 in this process, with the same weights: the
     existing wave-per-book kernel doing the same Q evaluation (whole batch, one block per four books).  Not code under test.
(a) and (d) are taken in turn, once per round, so that both see the same clocks; the spread reported is (max - min) / median of the
rounds' averages.
    python tools/exp_vec_act.py [books] [--steps 100] [--rounds 5] [--train 200] [--out profiles/vec_act.json]"""
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
STEPS, ROUNDS, TRAIN = take("--steps", 100, int), take("--rounds", 5, int), take("--train", 200, int)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
DEPTH, TRADES, WARM, KERNEL_CALLS, EVAL_STEPS, BASELINE_CALLS = 10, 2, 20, 100, 40, 5

p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
g = engine.default_gen_params()
g.n_events = 64 + 6 * max(TRAIN, STEPS + WARM, ROUNDS * EVAL_STEPS + WARM)


def policy_torch(obs):
    bits = obs.view(torch.int32)
    return ((bits[:, 0] >> 3) ^ (bits[:, 1] >> 5)).remainder(9).to(torch.int32)


eng = engine.Engine(p, B)
eng.gen_events(g)
eng.reset()
eng.td_step(TRAIN)
eng.sync()
theta = eng.theta()
written = int((theta != 0).sum())
os.environ["LOB_NO_MEMO"] = "1"          # (the switches are read by lob_create)
ref = engine.Engine(p, B)
del os.environ["LOB_NO_MEMO"]
ref.gen_events(g)
ref.set_theta(theta)
env = VecEnv(eng)                        # (for its tensors and the stream handle only: the calls below go to the engine)
act_actions = torch.zeros(B, dtype=torch.int32, device=env.device)
act_q = torch.zeros((B, abi.LOB_N_ACTIONS), dtype=torch.float64, device=env.device)
torch.cuda.synchronize()
outs = {"action + q": abi.VecActOut(act_actions.data_ptr(), act_q.data_ptr()), "q only": abi.VecActOut(None, act_q.data_ptr()),
        "action only": abi.VecActOut(act_actions.data_ptr(), None)}


def start():
    eng.reset()
    eng.vec_observe(env.out)
    eng.sync()
    torch.cuda.synchronize()


def run(n, own_policy):
    with torch.cuda.stream(env.stream):
        for _ in range(n):
            if own_policy:
                eng.vec_act(abi.ACT_GREEDY, outs["action + q"])
                eng.vec_step(act_actions.data_ptr(), env.out)
            else:
                a = policy_torch(env.obs)
                eng.vec_step(a.data_ptr(), env.out)
    eng.sync()


# ---- b: the step with the engine's own policy in front, and alone ----
legs = [("lob_vec_step (torch policy)", False), ("lob_vec_act + lob_vec_step", True)]
times = {name: [] for name, _ in legs}
for r in range(ROUNDS):
    for name, own in legs:
        start()
        run(WARM, own)
        t0 = time.perf_counter()
        run(STEPS, own)
        times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)

# ---- a and d: the kernels alone, HIP events, in turn ----
start()
run(WARM, True)                          # (the books a few steps into the episode, as in b)
ref.reset()
ref.eval_step(WARM)
ref.sync()
kern = {k: [] for k in outs}
kern_ref = []
for r in range(ROUNDS):
    for name, out in outs.items():
        for _ in range(10):
            eng.vec_act(abi.ACT_GREEDY, out)
        eng.kernel_timing(1)             # (clears the timers)
        for _ in range(KERNEL_CALLS):
            eng.vec_act(abi.ACT_GREEDY, out)
        eng.sync()
        ms, n = eng.kernel_time_ms("vec_act_kernel")
        assert n == KERNEL_CALLS
        kern[name].append(ms)
        eng.kernel_timing(0)
    ref.kernel_timing(1)
    ref.eval_step(EVAL_STEPS)
    ref.sync()
    ms, n = ref.kernel_time_ms("act_kernel")
    assert n == EVAL_STEPS, (n, "lob_eval_step under LOB_NO_MEMO=1 runs act_kernel once per step")
    kern_ref.append(ms)
    ref.kernel_timing(0)
live_ref = int((ref.get_terminal() == 0).sum())


# ---- c: the route it replaces ----
def previous_route():
    obs = env.obs.cpu().numpy()
    q = eng.q_values(obs)
    a = torch.from_numpy(q.argmax(axis=1).astype(np.int32)).to(env.device)
    torch.cuda.synchronize()
    return q, a


previous_route()
base = []
for _ in range(BASELINE_CALLS):
    t0 = time.perf_counter()
    prev_q, prev_a = previous_route()
    base.append((time.perf_counter() - t0) * 1e3)
eng.vec_act(abi.ACT_ARGMAX, outs["action + q"])
eng.sync()
torch.cuda.synchronize()
term = eng.get_terminal()
same_q = bool(np.array_equal(act_q.cpu().numpy().view(np.uint64), prev_q.view(np.uint64)))
same_a = bool(np.array_equal(act_actions.cpu().numpy(), np.where(term == 0, prev_a.cpu().numpy(), 0)))
live = int((term == 0).sum())
rc = env.status()


def stat(t):
    return {"median": float(np.median(t)), "min": min(t), "max": max(t), "spread": (max(t) - min(t)) / float(np.median(t)), "rounds": len(t), "all": t}


rows = []
for name, _ in legs:
    rows.append({"leg": name, "step_ms": stat(times[name])})
    print("%-32s per step %.4f ms (min %.4f, max %.4f)" % (name, rows[-1]["step_ms"]["median"], min(times[name]), max(times[name])))
kernel = {k: dict(stat(v), launches_per_round=KERNEL_CALLS) for k, v in kern.items()}
for k, v in kernel.items():
    print("vec_act_kernel, %-12s %.4f ms (min %.4f, max %.4f, spread %.1f %%)" % (k, v["median"], v["min"], v["max"], 100 * v["spread"]))
kref = dict(stat(kern_ref), launches_per_round=EVAL_STEPS)
print("act_kernel of lob_eval_step, LOB_NO_MEMO=1: %.4f ms (min %.4f, max %.4f, spread %.1f %%); live books at the end %d" % (
    kref["median"], kref["min"], kref["max"], 100 * kref["spread"], live_ref))
ratio = kernel["action + q"]["median"] / kref["median"]
verdict = "no slower" if kernel["action + q"]["median"] <= kref["median"] * (1 + max(kref["spread"], kernel["action + q"]["spread"])) else "SLOWER"
print("vec_act_kernel (action + q) / act_kernel = %.3f: %s than the existing kernel, within the spread of the rounds" % (ratio, verdict))
print("previous route %.1f ms per call (min %.1f, max %.1f); q equal to lob_q_values: %s; action its first maximum: %s" % (
    float(np.median(base)), min(base), max(base), same_q, same_a))
print("weights written by %d learner steps: %d of %d; live books at the end: %d of %d; lob_vec_status %d" % (TRAIN, written, theta.size, live, B, rc))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "max_trades": TRADES, "algo": "qlambda", "theta": "shared", "memory_size": int(p.memory_size),
                   "train_steps": TRAIN, "weights_nonzero": written, "steps": STEPS, "warm": WARM, "legs": rows,
                   "vec_act_kernel_hip_events_ms": kernel, "act_kernel_eval_step_no_memo_hip_events_ms": kref,
                   "vec_act_over_act_kernel": ratio, "verdict": verdict + " than act_kernel within the rounds' spread",
                   "previous_route_ms": {"median": float(np.median(base)), "min": min(base), "max": max(base), "calls": BASELINE_CALLS, "all": base},
                   "q_equal_lob_q_values": same_q, "action_is_first_maximum": same_a, "live_books_at_end": live, "lob_vec_status": rc}, fh, indent=1)
ref.close()
eng.close()
