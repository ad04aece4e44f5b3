"""lob_branch_fork / _step / _select / _close: N private copies of every book's environment state that stay on the device between
launches, stepped one step at a time with actions from device memory and rearranged within every book, with nothing of the engine
changed.

Yardsticks, every comparison for equality of every element of every book (rewards as uint64 views, no tolerance anywhere: both sides
run the same arithmetic):
  * lob_vec_rollout under the plan that the h calls' actions make up (tests/test_gpu_vec_rollout.py DevRoll): the rewards of every
    step, obs / terminal behind the last, the sum of the stepped words;
  * the real steps from a snapshot: lob_snapshot_save, h x lob_vec_step with a download behind each, lob_snapshot_restore, per branch --
    every output of every step;
  * for lob_branch_select: the roll-out of each branch's ancestor's actions followed by its own, and numpy's gather for `out`;
  * the oracle under the same actions, when branch calls stand in front of every real step (they leave nothing behind).
The device buffers are plain hipMalloc memory with one guard plane in front of the N and one behind (DevBranch); the torch face runs in
a process of its own (tests/vec_branch_torch_child.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi
from rl_markets_amd.engine import LobError
from tests.test_gpu_days import make_days
from tests.test_gpu_snapshot import Run
from tests.test_gpu_vec_env import DevArray, check_step, hip, make_params
from tests.test_gpu_vec_rollout import DevRoll, random_plans

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA = abi.LOB_N_ACTIONS
KEYS = ("obs", "reward", "terminal", "stepped")
SLOT = 3   # the snapshot slot the real-step yardstick uses


class DevBranch:
    """The [N][B] input words and the four output tensors of the branch calls for one N, each output with a guard plane in front and
    behind (N + 2 planes, the calls are given the address of the second): read() checks that both still hold the fill."""

    def __init__(self, B, V, N, want=KEYS):
        self.B, self.V, self.N = B, V, N
        self.words = DevArray((N, B), np.int32)
        self.arr = {"obs": DevArray((N + 2, B, V), np.float32), "reward": DevArray((N + 2, B), np.float64),
                    "terminal": DevArray((N + 2, B), np.uint8), "stepped": DevArray((N + 2, B), np.int32)}
        self.out = abi.BranchOut(*[self.arr[k].ptr + self.arr[k].host[0].nbytes if k in want else None for k in KEYS])

    def fill(self):
        for v in self.arr.values():
            assert hip().hipMemset(v.ptr, 0xAB, max(v.host.nbytes, 16)) == 0

    def read(self, eng):
        eng.sync()
        got = {}
        for k, v in self.arr.items():
            a = v.download()
            assert (a[0].view(np.uint8) == 0xAB).all() and (a[-1].view(np.uint8) == 0xAB).all(), k + ": a guard plane was written"
            got[k] = a[1:-1]
        return got

    def fork(self, eng):
        eng.branch_fork(self.N, self.out)
        return self.read(eng)

    def step(self, eng, actions):
        self.words.upload(actions)
        eng.branch_step(self.words.ptr, self.out)
        return self.read(eng)

    def select(self, eng, parent):
        self.words.upload(parent)
        eng.branch_select(self.words.ptr, self.out)
        return self.read(eng)

    def free(self):
        self.words.free()
        for v in self.arr.values():
            v.free()


class Bufs:
    """DevBranch by N and DevRoll by (N, H), made on first use."""

    def __init__(self, B, V):
        self.B, self.V, self.b, self.r = B, V, {}, {}

    def branch(self, N):
        if N not in self.b:
            self.b[N] = DevBranch(self.B, self.V, N)
        return self.b[N]

    def roll(self, N, H):
        if (N, H) not in self.r:
            self.r[(N, H)] = DevRoll(self.B, self.V, N, H)
        return self.r[(N, H)]

    def free(self):
        for v in list(self.b.values()) + list(self.r.values()):
            v.free()


def holey_plans(rng, N, H, B, p_skip=0.15):
    """Random per-book plans with actions out of range in them (-1 mostly, 9 and INT32_MIN now and then): those steps are skipped."""
    plans = random_plans(rng, N, H, B)
    holes = rng.random((N, H, B)) < p_skip
    plans[holes] = rng.choice(np.array([-1, -1, -1, 9, np.iinfo(np.int32).min], np.int32), size=int(holes.sum()))
    return plans


def bits(a):
    return a.view(np.uint64)


def check_fork(r, got, tag):
    """lob_branch_fork's out: in every plane the books' latest observation and terminal word, reward +0.0, stepped 0."""
    now = r.observe()
    for n in range(got["obs"].shape[0]):
        np.testing.assert_array_equal(got["obs"][n], now["obs"], err_msg="%s: fork obs, plane %d" % (tag, n))
        np.testing.assert_array_equal(got["terminal"][n], now["terminal"], err_msg="%s: fork terminal, plane %d" % (tag, n))
    assert (bits(got["reward"]) == 0).all() and (got["stepped"] == 0).all(), tag + ": fork reward / stepped"


def steps_against_the_rollout(r, bufs, N, H, tag, seen, plans=None, fork=True):
    """fork, then H branch steps under `plans` [N][H][B], against one lob_vec_rollout of the same plans from the same present."""
    plans = holey_plans(r.rng, N, H, r.B) if plans is None else plans
    ref = bufs.roll(N, H).rollout(r.eng, plans, 1.0)
    db = bufs.branch(N)
    if fork:
        check_fork(r, db.fork(r.eng), tag)
    term0 = r.eng.get_terminal()
    stepped = np.zeros((N, r.B), np.int32)
    for h in range(H):
        got = db.step(r.eng, plans[:, h])
        np.testing.assert_array_equal(bits(got["reward"]), bits(ref["reward"][:, h]), err_msg="%s: reward of step %d" % (tag, h))
        assert set(np.unique(got["stepped"])) <= {0, 1}
        assert (bits(got["reward"])[got["stepped"] == 0] == 0).all(), tag
        stepped += got["stepped"]
    np.testing.assert_array_equal(got["obs"], ref["obs"], err_msg=tag + ": obs behind the last step")
    np.testing.assert_array_equal(got["terminal"], ref["terminal"], err_msg=tag + ": terminal behind the last step")
    np.testing.assert_array_equal(stepped, ref["stepped"], err_msg=tag + ": the sum of the stepped words")
    live = term0 == 0
    seen["checked"] += 1
    seen["stepped"] |= bool(stepped.any())
    seen["nonzero"] |= bool((ref["reward"] != 0.0).any())
    seen["ends_inside"] |= bool((live[None] & (ref["terminal"] != 0) & (stepped > 0)).any())
    seen["dry"] |= bool((live[None] & (ref["terminal"] == 2)).any())
    seen["terminal_1"] |= bool((live[None] & (ref["terminal"] == 1)).any())
    seen["over"] |= bool((~live).any())
    seen["differs"] |= bool((live & (got["obs"].view(np.uint32) != got["obs"].view(np.uint32)[0]).any((0, 2))).any())
    assert (stepped[:, ~live] == 0).all(), tag + ": a book that was over has been stepped"
    return plans, ref


def new_seen():
    return {"checked": 0, "stepped": False, "nonzero": False, "ends_inside": False, "dry": False, "terminal_1": False, "over": False,
            "differs": False}


def real_steps(r, plans):
    """The yardstick without a look-ahead in it: from a snapshot of this very moment, branch after branch through lob_vec_step;
    every output of every step, [N][H][...].  (Actions out of range are counted by the real step: lob_vec_status is read.)"""
    eng, B = r.eng, r.B
    N, H = plans.shape[:2]
    ref = {"obs": np.zeros((N, H, B, r.V), np.float32), "reward": np.zeros((N, H, B), np.float64), "terminal": np.zeros((N, H, B), np.uint8),
           "stepped": np.zeros((N, H, B), np.int32)}
    eng.snapshot_save(SLOT, None)
    for n in range(N):
        for h in range(H):
            r.dev.step(eng, plans[n, h])
            got = r.dev.read(eng)
            for k in KEYS:
                ref[k][n, h] = got[k]
        eng.snapshot_restore(SLOT, None)
    eng.vec_status()
    return ref


def steps_against_the_real_steps(r, db, plans, tag, fork=True):
    N, H = plans.shape[:2]
    ref = real_steps(r, plans)
    if fork:
        check_fork(r, db.fork(r.eng), tag)
    for h in range(H):
        got = db.step(r.eng, plans[:, h])
        for k in ("obs", "terminal", "stepped"):
            np.testing.assert_array_equal(got[k], ref[k][:, h], err_msg="%s: %s of step %d" % (tag, k, h))
        np.testing.assert_array_equal(bits(got["reward"]), bits(ref["reward"][:, h]), err_msg="%s: reward of step %d" % (tag, h))
    return ref


def random_step(r):
    r.dev.step(r.eng, r.rng.integers(0, NA, size=r.B).astype(np.int32))


def to_the_end(r, bufs, N, H, tag, seen, k, cap=600):
    """Random actions on the real books until none is live; the branches are checked against the roll-out before every k-th step,
    before every step once a book is over, and once behind the last, where every book is over."""
    steps = 0
    while True:
        n_live = int((r.eng.get_terminal() == 0).sum())
        if steps % k == 0 or n_live < r.B:
            steps_against_the_rollout(r, bufs, N, H, "%s before step %d" % (tag, steps + 1), seen)
        if n_live == 0:
            return steps
        random_step(r)
        steps += 1
        assert steps < cap, tag + ": the episode did not end"


# ---- 1. against the roll-out -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 2, 9])
@pytest.mark.parametrize("B,depth,trades,ending", [(1, 5, 2, "dry"), (1, 10, 3, "session"), (63, 10, 2, "session"), (65, 5, 3, "dry"),
                                                   (300, 10, 2, "session")])
def test_against_the_rollout(B, depth, trades, ending, N):
    H = 6
    r = Run(B, ending, seed=60, p=make_params(depth, trades))
    bufs = Bufs(B, r.V)
    seen = new_seen()
    tag = "B=%d D=%d T=%d %s N=%d" % (B, depth, trades, ending, N)
    # (before every third step -- every step of a single book: an episode's end then falls inside the six steps of some check)
    steps = to_the_end(r, bufs, N, H, tag, seen, 1 if B == 1 else 3)
    term = r.eng.get_terminal()
    assert steps > 10 and ((term == 2).all() if ending == "dry" else (term == 1).all()), (steps, term)
    assert seen["stepped"] and seen["nonzero"] and seen["ends_inside"] and seen["over"], (tag, seen)
    assert seen["dry" if ending == "dry" else "terminal_1"], tag + ": the episode's kind of ending inside the branch steps"
    assert N == 1 or seen["differs"], tag + ": two branches of a live book whose observations differ"
    assert r.eng.vec_status() == (abi.LOB_OK, 0), "the branch steps count no action out of range"
    bufs.free()
    r.close()


# ---- 2. against the real steps -----------------------------------------------------------------------------------------------------------

def test_against_the_real_steps():
    B, N, H = 65, 3, 6
    r = Run(B, "dry", seed=61)
    db = DevBranch(B, r.V, N)
    points = 0
    while (r.eng.get_terminal() == 0).any():
        if points % 12 == 3 or not (r.eng.get_terminal() == 0).all():
            steps_against_the_real_steps(r, db, holey_plans(r.rng, N, H, B), "before step %d" % (points + 1))
        random_step(r)
        points += 1
        assert points < 600
    assert points > 10
    db.free()
    r.close()


# ---- 3. the window ring ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lb_pnl", [1, 3, 8])
@pytest.mark.parametrize("B", [65, 300])
def test_window_ring(B, lb_pnl):
    """NORMED reads the two PnL windows; over 12 steps a branch replaces its own pushes (lb_pnl 1: at once; 3: four times round; 8:
    once the engine's entries are used up).  Started with the windows full and once more with them still filling."""
    N, H = 2, 12
    p = make_params(5, 2)
    p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, lb_pnl
    r = Run(B, "dry", seed=62, p=p)
    db = DevBranch(B, r.V, N)
    nonzero = False
    for start in (2, 14):   # real steps in front: the windows hold 2 entries, then 16
        while len(r.hist) < start:
            r.step(1, main=False)
        ref = steps_against_the_real_steps(r, db, random_plans(r.rng, N, H, B), "lb_pnl=%d after %d steps" % (lb_pnl, start))
        nonzero |= bool((ref["reward"][:, -1] != 0.0).any())
        assert ref["stepped"].sum(1).max() == H, "a branch that pushed H times"
    # (a window of ONE entry has no deviation: that measure is 0 throughout -- tests/test_gpu_vec_rollout.py)
    assert lb_pnl == 1 or nonzero, "a nonzero NORMED reward at the last step: full windows of the branch's own pushes"
    db.free()
    r.close()


# ---- 4. every reward measure --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", sorted(abi.REWARD_NAMES, key=abi.REWARD_NAMES.get))
def test_every_reward_measure(measure):
    B, N, H = 65, 2, 5
    p = make_params(5, 2)
    p.reward_measure = abi.REWARD_NAMES[measure]
    if p.reward_measure == abi.REWARD_NORMED:
        p.lb_pnl = 3
    r = Run(B, "dry", seed=63, p=p)
    db = DevBranch(B, r.V, N)
    nonzero = False
    for start in (4, 30):
        while len(r.hist) < start:
            r.step(1, main=False)
        ref = steps_against_the_real_steps(r, db, random_plans(r.rng, N, H, B), "measure %s after %d steps" % (measure, start))
        nonzero |= bool((ref["reward"] != 0.0).any())
    assert nonzero or p.reward_measure == abi.REWARD_NONE, measure
    db.free()
    r.close()


# ---- 5. select -------------------------------------------------------------------------------------------------------------------------------

def parents_of(case, rng, N, B):
    ident = np.broadcast_to(np.arange(N, dtype=np.int32)[:, None], (N, B)).copy()
    if case == "identity":
        return [ident]
    if case == "permutation":
        return [np.broadcast_to(rng.permutation(N).astype(np.int32)[:, None], (N, B)).copy()]
    if case == "one parent":
        return [np.full((N, B), N - 2, np.int32)]
    if case == "out of range":
        p = rng.integers(0, N, size=(N, B)).astype(np.int32)
        odd = rng.random((N, B)) < 0.5
        p[odd] = rng.choice(np.array([-1, N, N + 7, np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int32), size=int(odd.sum()))
        return [p]
    if case == "per book":
        return [rng.integers(0, N, size=(N, B)).astype(np.int32)]
    assert case == "two in a row"
    return [rng.integers(0, N, size=(N, B)).astype(np.int32), rng.integers(0, N, size=(N, B)).astype(np.int32)]


@pytest.mark.parametrize("case", ["identity", "permutation", "one parent", "out of range", "per book", "two in a row"])
@pytest.mark.parametrize("reward", ["pnl", "normed-3"])
def test_select(case, reward):
    """Three steps, the select(s), three more steps: every branch equals the roll-out of its ancestor's first three actions followed
    by its own last three -- the rewards of the last three steps, obs / terminal behind them, and the stepped words of both halves.
    `out` of every select is numpy's gather of the obs / terminal in front of it.  B = 130: two full blocks and a partial one per
    branch; normed-3: the rings are part of what is copied."""
    B, N, H = 130, 5, 3
    p = make_params(5, 2)
    if reward != "pnl":
        p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, 3
    r = Run(B, "dry", seed=64, p=p)
    while (r.eng.get_terminal() == 0).all():   # to the step at which the first books are over: others run dry inside the six
        random_step(r)
    assert (r.eng.get_terminal() == 0).any()
    db, dr = DevBranch(B, r.V, N), DevRoll(B, r.V, N, 2 * H)
    a0, a1 = holey_plans(r.rng, N, H, B), holey_plans(r.rng, N, H, B)
    cols = np.arange(B)[None, :]
    check_fork(r, db.fork(r.eng), case)
    first = np.zeros((N, B), np.int32)
    for h in range(H):
        got = db.step(r.eng, a0[:, h])
        first += got["stepped"]
    anc = np.broadcast_to(np.arange(N)[:, None], (N, B)).copy()   # whose first three actions branch (n, b) now carries
    for parent in parents_of(case, r.rng, N, B):
        eff = np.where((parent >= 0) & (parent < N), parent, np.arange(N, dtype=np.int32)[:, None])
        db.fill()
        sel = db.select(r.eng, parent)
        np.testing.assert_array_equal(sel["obs"], got["obs"][eff, cols], err_msg=case + ": out.obs of select is the gather")
        np.testing.assert_array_equal(sel["terminal"], got["terminal"][eff, cols], err_msg=case + ": out.terminal of select is the gather")
        assert (sel["reward"].view(np.uint8) == 0xAB).all() and (sel["stepped"].view(np.uint8) == 0xAB).all(), "select writes no reward / stepped"
        got = {"obs": sel["obs"], "terminal": sel["terminal"]}
        anc = anc[eff, cols]
    plans = np.concatenate([a0[anc, :, cols].transpose(0, 2, 1), a1], axis=1)   # [N][2H][B]
    ref = dr.rollout(r.eng, plans, 1.0)
    last = np.zeros((N, B), np.int32)
    for h in range(H):
        got = db.step(r.eng, a1[:, h])
        np.testing.assert_array_equal(bits(got["reward"]), bits(ref["reward"][:, H + h]), err_msg="%s: reward of step %d behind the select" % (case, h))
        last += got["stepped"]
    np.testing.assert_array_equal(got["obs"], ref["obs"], err_msg=case + ": obs")
    np.testing.assert_array_equal(got["terminal"], ref["terminal"], err_msg=case + ": terminal")
    np.testing.assert_array_equal(first[anc, cols] + last, ref["stepped"], err_msg=case + ": stepped of the ancestor's half + the own half")
    assert last.any() and (ref["terminal"] == 2).any()
    if case not in ("identity",):
        assert (anc != np.arange(N)[:, None]).any()
    db.free()
    dr.free()
    r.close()


# ---- 6. nothing left behind ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [65, 300])
def test_nothing_left_behind(B):
    """fork + two steps + select + a step in front of EVERY real step, the step log recording: the dumps, getters, counters and the
    step log right before and right after are the same, and the engine stays equal to the oracle under the same actions at every
    step to the end -- books, rewards (NORMED over windows of three: the engine's own PnL windows) and step counters.  The branch
    set of one step is stepped once more behind the NEXT real step: what it returns is what the roll-out said at fork time."""
    N = 3
    p = make_params(5, 2)
    p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, 3
    r = Run(B, "dry", seed=65, p=p, reset=False)
    r.eng.step_log_enable(None, 400)
    r.reset()
    db, dr = DevBranch(B, r.V, N), DevRoll(B, r.V, N, 4)
    steps = 0
    ones = np.ones(B, bool)

    def everything():
        n_rows, n_lost = r.eng.step_log_counts()
        rows = r.eng.step_log_read(0, B, 0, max(1, int(n_rows.max())))
        return {"books": bytes(r.eng.get_books()), "state": r.eng.get_state().tobytes(), "reward": r.eng.get_reward().tobytes(),
                "terminal": r.eng.get_terminal().tobytes(), "counters": tuple(r.eng.counters()), "log_counts": n_rows.tobytes() + n_lost.tobytes(),
                "log_rows": rows.tobytes()}

    nonzero = False
    while True:
        before = everything()
        plans = holey_plans(r.rng, N, 4, B)
        ref = dr.rollout(r.eng, plans, 1.0)
        db.fork(r.eng)
        db.step(r.eng, plans[:, 0])
        db.step(r.eng, plans[:, 1])
        db.select(r.eng, np.broadcast_to(np.arange(N, dtype=np.int32)[:, None], (N, B)))
        mid = db.step(r.eng, plans[:, 2])
        after = everything()
        for k in before:
            assert after[k] == before[k], "step %d: the branch calls changed %s" % (steps, k)
        np.testing.assert_array_equal(bits(mid["reward"]), bits(ref["reward"][:, 2]))
        got = r.step(1)
        steps += 1
        check_step(r.eng, r.orc, got, r.V, 0, "B=%d step %d behind branch calls" % (B, steps), books=ones)
        c, oc = r.eng.counters(), r.orc.counters()
        assert c[0] == oc[0] and c[1] == oc[1], (steps, c, oc)
        nonzero |= bool((got["reward"] != 0.0).any())
        # the real books have stepped on: the branches have not moved
        late = db.step(r.eng, plans[:, 3])
        np.testing.assert_array_equal(bits(late["reward"]), bits(ref["reward"][:, 3]), err_msg="step %d: a branch step behind a real step" % steps)
        for k in ("obs", "terminal"):
            np.testing.assert_array_equal(late[k], ref[k], err_msg="step %d: %s of a branch step behind a real step" % (steps, k))
        if int(got["n_live"][0]) == 0:
            break
        assert steps < 600
    assert steps > 20 and nonzero
    n_rows, n_lost = r.eng.step_log_counts()
    assert int(n_rows.max()) > 20 and not n_lost.any(), "the step log recorded the real steps only"
    assert r.eng.vec_status() == (abi.LOB_OK, 0)
    db.free()
    dr.free()
    r.close()


# ---- 7. fork again ---------------------------------------------------------------------------------------------------------------------------

def test_fork_again_and_with_another_n():
    """A fork re-bases the set on the books' new present; a fork with another N -- larger (the set is allocated again), smaller (it
    is not), larger again within what is there -- works, with a select in between so that both buffers have been the live one."""
    B = 65
    r = Run(B, "dry", seed=66)
    bufs = Bufs(B, r.V)
    seen = new_seen()
    for N in (2, 9, 1, 5, 9, 12):
        for _ in range(4):
            random_step(r)
        steps_against_the_rollout(r, bufs, N, 3, "fork again, N=%d" % N, seen)
        bufs.branch(N).select(r.eng, r.rng.integers(0, N, size=(N, B)).astype(np.int32))
        steps_against_the_rollout(r, bufs, N, 2, "fork again behind a select, N=%d" % N, seen)
    assert seen["stepped"] and seen["nonzero"] and seen["differs"]
    bufs.free()
    r.close()


# ---- 8. lifetime and refusals ------------------------------------------------------------------------------------------------------------

def refused(code, name, fn, *args):
    with pytest.raises(LobError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert name.encode() in abi.load().lob_last_error()
    return str(ei.value)


def test_lifetime_and_refusals():
    B, N = 65, 3
    r = Run(B, "dry", seed=67, reset=False)
    eng, lib = r.eng, abi.load()
    db = DevBranch(B, r.V, N)
    db.words.upload(np.zeros((N, B), np.int32))

    def no_set(tag):
        assert "no live branch set" in refused(abi.LOB_ESTATE, "lob_branch_step", eng.branch_step, db.words.ptr, db.out), tag
        assert "no live branch set" in refused(abi.LOB_ESTATE, "lob_branch_select", eng.branch_select, db.words.ptr, db.out), tag

    for name, fn, args in (("lob_branch_fork", eng.branch_fork, (N, db.out)), ("lob_branch_step", eng.branch_step, (db.words.ptr, db.out)),
                           ("lob_branch_select", eng.branch_select, (db.words.ptr, db.out))):
        refused(abi.LOB_ESTATE, name, fn, *args)   # before the first lob_reset
    eng.branch_close()   # (nothing to release: LOB_OK)
    r.reset()
    r.step(3)
    no_set("before the first fork")
    books = bytes(eng.get_books())
    vp = C.c_void_p
    for n in (0, -1, abi.MAX_BRANCHES + 1):
        refused(abi.LOB_EINVAL, "lob_branch_fork", eng.branch_fork, n, db.out)
    no_set("after a refused fork")
    eng.branch_fork(N, None)   # out may be NULL
    eng.branch_step(db.words.ptr, db.out)
    eng.branch_select(db.words.ptr, None)   # out may be NULL
    db.read(eng)
    db.fill()
    checks = [(lib.lob_branch_fork, (None, N, C.byref(db.out)), b"lob_branch_fork"), (lib.lob_branch_step, (None, vp(db.words.ptr), C.byref(db.out)), b"lob_branch_step"),
              (lib.lob_branch_step, (eng.h, None, C.byref(db.out)), b"lob_branch_step"), (lib.lob_branch_step, (eng.h, vp(db.words.ptr), None), b"lob_branch_step"),
              (lib.lob_branch_select, (None, vp(db.words.ptr), C.byref(db.out)), b"lob_branch_select"),
              (lib.lob_branch_select, (eng.h, None, C.byref(db.out)), b"lob_branch_select"), (lib.lob_branch_close, (None,), b"lob_branch_close")]
    for fn, args, name in checks:
        assert fn(*args) == abi.LOB_EINVAL and name in lib.lob_last_error(), name
    if eng.td_split_supported():
        eng.td_step_begin()
        refused(abi.LOB_ESTATE, "lob_branch_fork", eng.branch_fork, N, db.out)
        refused(abi.LOB_ESTATE, "lob_branch_step", eng.branch_step, db.words.ptr, db.out)
        refused(abi.LOB_ESTATE, "lob_branch_select", eng.branch_select, db.words.ptr, db.out)
        eng.td_step_end()
        r.orc.td_step(1)
        books = bytes(eng.get_books())
        eng.branch_step(db.words.ptr, db.out)   # the set is still live behind a learner step
        assert (db.read(eng)["reward"].view(np.uint8) != 0xAB).any()
        db.fill()
    eng.sync()
    assert bytes(eng.get_books()) == books, "a refused call changed the books"
    assert all((v.view(np.uint8) == 0xAB).all() for v in db.read(eng).values()), "a refused call wrote"
    eng.branch_close()
    no_set("after close")
    eng.branch_close()   # twice is fine
    eng.branch_fork(N, db.out)
    eng.branch_step(db.words.ptr, db.out)
    r.reset()
    no_set("after lob_reset")
    r.step(2)
    seen = new_seen()
    bufs = Bufs(B, r.V)
    steps_against_the_rollout(r, bufs, N, 3, "a fork behind the reset", seen)
    assert seen["stepped"]
    bufs.free()
    db.free()
    r.close()   # (lob_destroy releases a live set)


def test_ring_mode_is_refused(monkeypatch):
    """A market track that is a ring (tests/test_gpu_snapshot.py's switches): LOB_ESTATE, and the engine steps on."""
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    B, N = 64, 2
    r = Run(B, "dry", depth=10, seed=68, n_events=1200)
    db = DevBranch(B, r.V, N)
    db.words.upload(np.zeros((N, B), np.int32))
    r.step(3)
    books = bytes(r.eng.get_books())
    assert "ring" in refused(abi.LOB_ESTATE, "lob_branch_fork", r.eng.branch_fork, N, db.out)
    assert "ring" in refused(abi.LOB_ESTATE, "lob_branch_step", r.eng.branch_step, db.words.ptr, db.out)
    assert "ring" in refused(abi.LOB_ESTATE, "lob_branch_select", r.eng.branch_select, db.words.ptr, db.out)
    assert bytes(r.eng.get_books()) == books
    assert all((v.view(np.uint8) == 0xAB).all() for v in db.read(r.eng).values()), "a refused call wrote"
    for i in range(20):
        before = r.orc.counters()[0]
        got = r.step(1)
        check_step(r.eng, r.orc, got, r.V, before, "ring mode, after the refusal, step %d" % (i + 1))
    db.free()
    r.close()


# ---- 9. other settings ---------------------------------------------------------------------------------------------------------------------

def test_after_a_masked_restore():
    B, N = 65, 3
    r = Run(B, "dry", seed=69)
    bufs = Bufs(B, r.V)
    r.step(7, main=False)
    r.save(0)
    r.step(12, main=False)
    check_fork(r, bufs.branch(N).fork(r.eng), "in front of the restore")
    m = np.random.default_rng(70).integers(0, 2, size=B).astype(bool)
    assert m.any() and not m.all()
    plans = holey_plans(r.rng, N, 4, B)
    ref = bufs.roll(N, 4).rollout(r.eng, plans, 1.0)
    r.restore(0, m)
    # the set forked in front of the restore is still the books of that moment
    for h in range(4):
        got = bufs.branch(N).step(r.eng, plans[:, h])
        np.testing.assert_array_equal(bits(got["reward"]), bits(ref["reward"][:, h]), err_msg="a set across a restore, step %d" % h)
    np.testing.assert_array_equal(got["obs"], ref["obs"])
    seen = new_seen()
    steps = to_the_end(r, bufs, N, 4, "after a masked restore", seen, 8)
    assert steps > 10 and seen["stepped"] and seen["differs"] and seen["dry"]
    bufs.free()
    r.close()


def test_day_library_with_days_of_unequal_length():
    B, N, lengths = 65, 3, (100, 150, 200)
    p = make_params(5, 2)
    days = make_days(lengths, depth=5)
    assign = ((np.arange(B) * 7) % 3).astype(np.int32)
    r = Run(B, "dry", seed=71, p=p, reset=False)
    r.eng.load_days(days)
    r.eng.days_set(assign)
    r.eng.reset()
    np.testing.assert_array_equal(r.eng.days(), assign)
    bufs = Bufs(B, r.V)
    seen = new_seen()
    steps = to_the_end(r, bufs, N, 5, "day library", seen, 10)
    assert steps > 10 and (r.eng.get_terminal() == 2).all()
    assert seen["stepped"] and seen["differs"] and seen["dry"] and seen["ends_inside"]
    bufs.free()
    r.close()


def test_above_the_16_lane_env_kernel():
    """5 000 books at depth 10 (above the 4 096 up to which lob_vec_step runs the 16-lane env kernel), 79 blocks per branch with a
    partial last one; against the real steps, which go through the 64-lane kernel there.  (A small weight vector: the private weights
    of 5 000 books are not what this test is about.)"""
    B, N, H = 5000, 2, 3
    r = Run(B, "dry", depth=10, seed=72, mem=1 << 12)
    db = DevBranch(B, r.V, N)
    for step in range(21):
        if step % 10 == 0:
            ref = steps_against_the_real_steps(r, db, holey_plans(r.rng, N, H, B), "B=5000 before step %d" % (step + 1))
        random_step(r)
    assert ref["stepped"].any() and (ref["reward"] != 0.0).any()
    db.free()
    r.close()


def test_the_most_branches():
    B, N = 65, abi.MAX_BRANCHES
    r = Run(B, "dry", seed=73)
    bufs = Bufs(B, r.V)
    r.step(6, main=False)
    seen = new_seen()
    steps_against_the_rollout(r, bufs, N, 3, "N=64", seen)
    parent = r.rng.integers(0, N, size=(N, B)).astype(np.int32)
    before = bufs.branch(N).read(r.eng)
    sel = bufs.branch(N).select(r.eng, parent)
    np.testing.assert_array_equal(sel["obs"], before["obs"][parent, np.arange(B)[None, :]])
    assert seen["stepped"] and seen["differs"]
    bufs.free()
    r.close()


# ---- 10. members and neighbours -------------------------------------------------------------------------------------------------------------

def test_null_members_and_the_neighbours_of_the_buffers():
    B, N = 65, 3
    r = Run(B, "dry", seed=74)
    r.step(9, main=False)
    actions = random_plans(r.rng, N, 2, B)
    parent = r.rng.integers(0, N, size=(N, B)).astype(np.int32)
    full = DevBranch(B, r.V, N)

    def sequence(d):
        d.fill()
        out = [d.fork(r.eng)]
        d.fill()
        out.append(d.step(r.eng, actions[:, 0]))
        d.fill()
        out.append(d.select(r.eng, parent))
        d.fill()
        out.append(d.step(r.eng, actions[:, 1]))
        return out

    ref = sequence(full)
    assert all((v.view(np.uint8) != 0xAB).any() for k, v in ref[3].items())
    for want in [(k,) for k in KEYS] + [("reward", "terminal"), ()]:
        part = DevBranch(B, r.V, N, want=want)
        got = sequence(part)   # (all members NULL: the set is forked, stepped and rearranged all the same -- the next case shows it)
        for i, call in enumerate(("fork", "step", "select", "step")):
            for k in KEYS:
                if k in want and not (call == "select" and k in ("reward", "stepped")):
                    np.testing.assert_array_equal(got[i][k].view(np.uint8), ref[i][k].view(np.uint8), err_msg="members %s: %s of %s" % (want, k, call))
                else:
                    assert (got[i][k].view(np.uint8) == 0xAB).all(), "members %s: %s of %s was written" % (want, k, call)
        part.free()
    # the sequence that wrote nothing has forked, stepped and rearranged the set: one more step behind it gives what it gives
    # behind the full sequence
    again = random_plans(r.rng, N, 1, B)[:, 0]
    ref2 = full.step(r.eng, again)
    null = DevBranch(B, r.V, N, want=())
    sequence(null)
    got = full.step(r.eng, again)
    for k in KEYS:
        np.testing.assert_array_equal(got[k].view(np.uint8), ref2[k].view(np.uint8), err_msg="a step behind NULL-member calls: " + k)
    assert got["stepped"].any()
    null.free()
    full.free()
    r.close()


# ---- 11. the torch face ----------------------------------------------------------------------------------------------------------------------

def test_vec_env_branches_through_torch():
    """tests/vec_branch_torch_child.py, in a process of its own: torch must be imported before the engine library is loaded."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vec_branch_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "vec_branch_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "branches OK" in res.stdout
