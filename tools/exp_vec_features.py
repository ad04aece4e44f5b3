"""What the tile features and the external weight updates cost on the vector-env interface (lob_vec_features / lob_vec_update, DESIGN.md
7i): 65 536 synthetic 10-level books on one GPU, Q(lambda), one weight vector shared by all books, the weights as `--train` learner
steps leave them --
  a  the HIP-event time of vec_feat_kernel's features form (lob_kernel_time_ms "vec_features_kernel") in the books' form, a few steps into
     the episode, for sums only, idx only and both;
  b  the yardstick, taken in turn in the same process: vec_act_kernel, q only -- the same hashing plus the weight gathers;
  c  the update form ("vec_update_kernel") right after lob_reset, where every book stands on the same few tiles and the atomics of the
     whole batch queue on them, and a few steps into the episode; the memo_kernel launch lob_vec_update puts behind it is not in the
     figure;
  d  the route (a) replaces: D2H of obs, lob_features, upload of the [n, 9, 96] cube.
(a), (b) and (c) are taken in turn, once per round; the spread reported is (max - min) / median of the rounds' averages.
    python tools/exp_vec_features.py [books] [--rounds 5] [--train 200] [--out profiles/vec_features.json]"""
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
ROUNDS, TRAIN = take("--rounds", 5, int), take("--train", 200, int)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
DEPTH, TRADES, WARM, KERNEL_CALLS, UPDATE_CALLS, BASELINE_CALLS = 10, 2, 20, 100, 20, 3

p = engine.default_params()
p.depth, p.max_trades, p.algo, p.theta_mode = DEPTH, TRADES, abi.ALGO_QLAMBDA, abi.THETA_SHARED
g = engine.default_gen_params()
g.n_events = 64 + 6 * max(TRAIN, 2 * WARM)

eng = engine.Engine(p, B)
eng.gen_events(g)
eng.reset()
eng.td_step(TRAIN)
eng.sync()
written = int((eng.theta() != 0).sum())
env = VecEnv(eng)                        # (for its tensors and the stream handle only: the calls below go to the engine)
dev = env.device
sums = torch.zeros((B, abi.N_TILES), dtype=torch.int32, device=dev)
idx = torch.zeros((B, abi.N_TILES), dtype=torch.int32, device=dev)
act_actions = torch.zeros(B, dtype=torch.int32, device=dev)
act_q = torch.zeros((B, abi.LOB_N_ACTIONS), dtype=torch.float64, device=dev)
actions = (torch.arange(B, device=dev) % abi.LOB_N_ACTIONS).to(torch.int32)
step = torch.full((B,), 2.0 ** -30, dtype=torch.float64, device=dev)   # (small: the weights stay what the training left)
torch.cuda.synchronize()
feat_outs = {"sums": abi.VecFeatOut(sums.data_ptr(), None), "idx": abi.VecFeatOut(None, idx.data_ptr()), "sums + idx": abi.VecFeatOut(sums.data_ptr(), idx.data_ptr())}
q_only = abi.VecActOut(None, act_q.data_ptr())
both = abi.VecActOut(act_actions.data_ptr(), act_q.data_ptr())


def start(steps):
    eng.reset()
    eng.vec_observe(env.out)
    for _ in range(steps):
        eng.vec_act(abi.ACT_GREEDY, both)
        eng.vec_step(act_actions.data_ptr(), env.out)
    eng.sync()
    torch.cuda.synchronize()


def timed(name, calls, fn):
    for _ in range(3):
        fn()
    eng.kernel_timing(1)                 # (clears the timers)
    for _ in range(calls):
        fn()
    eng.sync()
    ms, n = eng.kernel_time_ms(name)
    assert n == calls, (name, n, calls)
    eng.kernel_timing(0)
    return ms


kern = {k: [] for k in feat_outs}
kern_q, upd_reset, upd_mid = [], [], []
distinct = {}
for r in range(ROUNDS):
    start(0)
    upd_reset.append(timed("vec_update_kernel", UPDATE_CALLS, lambda: eng.vec_update(None, B, actions.data_ptr(), step.data_ptr())))
    if r == 0:
        eng.vec_features(None, B, actions.data_ptr(), feat_outs["sums + idx"])
        eng.sync()
        distinct["after reset"] = int(torch.unique(idx).numel())
    start(WARM)
    for name, out in feat_outs.items():
        kern[name].append(timed("vec_features_kernel", KERNEL_CALLS, lambda: eng.vec_features(None, B, actions.data_ptr(), out)))
    kern_q.append(timed("vec_act_kernel", KERNEL_CALLS, lambda: eng.vec_act(abi.ACT_GREEDY, q_only)))
    upd_mid.append(timed("vec_update_kernel", UPDATE_CALLS, lambda: eng.vec_update(None, B, actions.data_ptr(), step.data_ptr())))
    if r == 0:
        eng.sync()
        distinct["mid-episode"] = int(torch.unique(idx).numel())


# ---- d: the route it replaces ----
def previous_route():
    obs = env.obs.cpu().numpy()
    cube = eng.features(obs)
    t = torch.from_numpy(cube).to(dev)
    torch.cuda.synchronize()
    return cube, t


previous_route()
base = []
for _ in range(BASELINE_CALLS):
    t0 = time.perf_counter()
    cube, _ = previous_route()
    base.append((time.perf_counter() - t0) * 1e3)
eng.vec_features(None, B, actions.data_ptr(), feat_outs["sums + idx"])
eng.sync()
torch.cuda.synchronize()
terms = np.repeat(np.array(eng.vec_terms(), np.int64).T, 32, axis=1)            # [9][96]
same = bool(np.array_equal((sums.cpu().numpy().astype(np.int64)[:, None, :] + terms[None]) % p.memory_size, cube))
same_idx = bool(np.array_equal(idx.cpu().numpy(), cube[np.arange(B), actions.cpu().numpy()]))
rc = env.status()


def stat(t):
    return {"median": float(np.median(t)), "min": min(t), "max": max(t), "spread": (max(t) - min(t)) / float(np.median(t)), "rounds": len(t), "all": t}


kernel = {k: dict(stat(v), launches_per_round=KERNEL_CALLS) for k, v in kern.items()}
for k, v in kernel.items():
    print("vec_feat_kernel features, %-10s %.4f ms (min %.4f, max %.4f, spread %.1f %%)" % (k, v["median"], v["min"], v["max"], 100 * v["spread"]))
kq = dict(stat(kern_q), launches_per_round=KERNEL_CALLS)
print("vec_act_kernel, q only:              %.4f ms (min %.4f, max %.4f, spread %.1f %%)" % (kq["median"], kq["min"], kq["max"], 100 * kq["spread"]))
ratio = kernel["sums + idx"]["median"] / kq["median"]
verdict = "no slower" if kernel["sums + idx"]["median"] <= kq["median"] * (1 + max(kq["spread"], kernel["sums + idx"]["spread"])) else "SLOWER"
print("features (sums + idx) / vec_act_kernel (q only) = %.3f: %s than the yardstick, within the spread of the rounds" % (ratio, verdict))
ur, um = dict(stat(upd_reset), launches_per_round=UPDATE_CALLS), dict(stat(upd_mid), launches_per_round=UPDATE_CALLS)
print("vec_feat_kernel update, after reset: %.4f ms (min %.4f, max %.4f); distinct weights among %d x 96: %d" % (ur["median"], ur["min"], ur["max"], B, distinct["after reset"]))
print("vec_feat_kernel update, mid-episode: %.4f ms (min %.4f, max %.4f); distinct weights among %d x 96: %d" % (um["median"], um["min"], um["max"], B, distinct["mid-episode"]))
print("previous route %.1f ms per call (min %.1f, max %.1f); sums + terms equal to lob_features: %s; idx its plane: %s" % (
    float(np.median(base)), min(base), max(base), same, same_idx))
print("weights written by %d learner steps: %d of %d; lob_vec_status %d" % (TRAIN, written, p.memory_size, rc))
if out_path:
    with open(out_path, "w") as fh:
        json.dump({"books": B, "depth": DEPTH, "max_trades": TRADES, "algo": "qlambda", "theta": "shared", "memory_size": int(p.memory_size),
                   "train_steps": TRAIN, "weights_nonzero": written, "warm_steps": WARM,
                   "vec_features_kernel_hip_events_ms": kernel, "vec_act_kernel_q_only_hip_events_ms": kq,
                   "features_both_over_vec_act_q": ratio, "verdict": verdict + " than vec_act_kernel (q only) within the rounds' spread",
                   "vec_update_kernel_after_reset_hip_events_ms": ur, "vec_update_kernel_mid_episode_hip_events_ms": um,
                   "distinct_weights_of_the_batch": distinct,
                   "previous_route_ms": {"median": float(np.median(base)), "min": min(base), "max": max(base), "calls": BASELINE_CALLS, "all": base},
                   "sums_plus_terms_equal_lob_features": same, "idx_is_the_actions_plane": same_idx, "lob_vec_status": rc}, fh, indent=1)
eng.close()
