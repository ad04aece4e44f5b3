"""The shapes and the scripted actions of tests/test_gpu_branch_obs.py, shared with tests/test_branch_obs_seeds.py, which replays them
through the oracle on the CPU: the same generator, drawn from in the same order, gives the engine's test and the oracle's check the
same real steps in front of the fork and the same per-branch plans behind it (not collected by pytest)."""
import numpy as np

from rl_markets_amd import abi

N_EVENTS = 160   # tests/test_gpu_snapshot.py Run's default stream
PRE, H = 8, 6    # real steps in front of the fork, branch steps behind it

# (B, depth, trade slots, N, K): B in {3, 65, 130} -- less than a wave, a wave + 1, two waves + 2 --, depth in {5, 10} and one case each
# of 1 and 7 (quads partly masked), 2 and 3 trade slots, N in {1, 3, 9}, K in {1, 5, 128}; every value of every axis with every B
SHAPES = [(3, 5, 2, 1, 1), (3, 10, 3, 9, 128), (3, 5, 3, 3, 5),
          (65, 5, 3, 3, 5), (65, 10, 2, 9, 1), (65, 10, 3, 1, 128), (65, 1, 2, 3, 5),
          (130, 10, 2, 3, 128), (130, 5, 3, 1, 5), (130, 5, 2, 9, 1), (130, 7, 3, 9, 128)]
SEED = 80


def rng_of(B, seed=SEED):
    return np.random.default_rng(1000 * B + seed)   # (Run's own generator for this seed)


def random_actions(rng, B):
    return rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)


def holey(rng, N, n_steps, B, p_skip=0.15):
    """tests/test_gpu_vec_branch.py holey_plans, restated so that the CPU check imports no GPU test module: random per-book plans
    [N][n_steps][B] with actions out of range in them (-1 mostly, 9 and INT32_MIN now and then): those steps are skipped."""
    plans = rng.integers(0, abi.LOB_N_ACTIONS, size=(N, n_steps, B)).astype(np.int32)
    holes = rng.random((N, n_steps, B)) < p_skip
    plans[holes] = rng.choice(np.array([-1, -1, -1, 9, np.iinfo(np.int32).min], np.int32), size=int(holes.sum()))
    return plans


def script(B, N, pre=PRE, n_steps=H, seed=SEED):
    """-> (the action arrays of the real steps in front of the fork, the plans [N][n_steps][B] behind it)"""
    rng = rng_of(B, seed)
    return [random_actions(rng, B) for _ in range(pre)], holey(rng, N, n_steps, B)


def reached(rec, n_valid, own, N, K):
    """What the comparison of case 2 must have covered, from a yardstick's output -- rec / n_valid [N][H][B], own [N][H][B][16]:
    two branches of one book with different rec (N > 1), a history slot of zeros (K = 128), a live own order on either side and a
    non-zero position.  -> the names of what is missing"""
    missing = []
    if N > 1 and not (rec != rec[:1]).any():
        missing.append("two branches of one book with different rec")
    if K == 128 and not (n_valid < K).any():
        missing.append("a history slot of zeros")
    if not (own[..., abi.OWN_ASK_HAS_ORDER] != 0).any() or not (own[..., abi.OWN_BID_HAS_ORDER] != 0).any():
        missing.append("a live own order on either side")
    if not (own[..., abi.OWN_POSITION] != 0).any():
        missing.append("a non-zero position")
    return missing
