"""lob_vec_rollout: what H consecutive lob_vec_step calls would write under each of P action plans per book, in one launch, with
nothing of the engine changed.

Yardsticks, every comparison for equality of every element of every book (rewards and returns as uint64 views, no tolerance anywhere:
both sides run the same arithmetic):
  * the composed route: lob_snapshot_save, H x lob_vec_step(plans[p][h]) with a download behind each, lob_snapshot_restore, for each p;
  * lob_vec_peek for H = 1;
  * the oracle under the same actions, when a look-ahead stands in front of every step (it leaves nothing behind);
  * the oracle directly: a fresh Oracle replays the action prefix and then the plan (no engine step in the yardstick);
  * the discount loop in numpy over the call's own rewards, for `ret`.
The device buffers are plain hipMalloc memory with one guard plane in front of the P and one behind (DevRoll); the torch face runs in
a process of its own (tests/vec_rollout_torch_child.py)."""
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
from tests.test_gpu_vec_peek import DevPeek, scout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = abi.LOB_N_ACTIONS
KEYS = ("obs", "reward", "terminal", "stepped", "ret")
SLOT = 3   # the snapshot slot the composed route uses
SHAPES = [(1, 1), (3, 2), (9, 5), (5, 8)]   # (P, H) of the checks against the real steps, taken in turn


class DevRoll:
    """The plans and the five output tensors of lob_vec_rollout for one (P, H), each output with a guard plane in front and behind
    (P + 2 planes, the call is given the address of the second): read() checks that both still hold the fill."""

    def __init__(self, B, V, P, H, want=KEYS):
        self.B, self.V, self.P, self.H = B, V, P, H
        self.plans = DevArray((P, H, B), np.int32)
        self.arr = {"obs": DevArray((P + 2, B, V), np.float32), "reward": DevArray((P + 2, H, B), np.float64),
                    "terminal": DevArray((P + 2, B), np.uint8), "stepped": DevArray((P + 2, B), np.int32), "ret": DevArray((P + 2, B), np.float64)}
        self.out = abi.VecRolloutOut(*[self.arr[k].ptr + self.arr[k].host[0].nbytes if k in want else None for k in KEYS])

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

    def rollout(self, eng, plans, gamma=1.0):
        self.plans.upload(plans)
        eng.vec_rollout(self.plans.ptr, self.P, self.H, gamma, self.out)
        return self.read(eng)

    def free(self):
        self.plans.free()
        for v in self.arr.values():
            v.free()


class Rolls:
    """DevRoll buffers by (P, H), made on first use."""

    def __init__(self, B, V):
        self.B, self.V, self.d = B, V, {}

    def get(self, P, H):
        if (P, H) not in self.d:
            self.d[(P, H)] = DevRoll(self.B, self.V, P, H)
        return self.d[(P, H)]

    def free(self):
        for v in self.d.values():
            v.free()


def random_plans(rng, P, H, B):
    return rng.integers(0, N, size=(P, H, B)).astype(np.int32)


def ret_of(reward, gamma):
    """The contract's loop, every operation rounded on its own (numpy's f64 arithmetic does not fuse)."""
    P, H, B = reward.shape
    acc, d = np.zeros((P, B), np.float64), np.float64(1.0)
    for h in range(H):
        acc = acc + d * reward[:, h]
        d = d * np.float64(gamma)
    return acc


def composed(r, plans, gamma=1.0):
    """The yardstick: from a snapshot of this very moment, plan after plan through the real step.  `term` [P][H + 1][B] is
    lob_get_terminal's value in front of every step and behind the last (what the asserts on the inputs look at)."""
    eng, B = r.eng, r.B
    P, H = plans.shape[:2]
    ref = {"obs": np.zeros((P, B, r.V), np.float32), "reward": np.zeros((P, H, B), np.float64), "terminal": np.zeros((P, B), np.uint8),
           "stepped": np.zeros((P, B), np.int32), "term": np.zeros((P, H + 1, B), np.uint8)}
    term0 = eng.get_terminal()
    eng.snapshot_save(SLOT, None)
    for p in range(P):
        ref["term"][p, 0] = term0
        for h in range(H):
            r.dev.step(eng, plans[p, h])
            got = r.dev.read(eng)
            assert set(np.unique(got["stepped"])) <= {0, 1}
            ref["reward"][p, h] = got["reward"]
            ref["stepped"][p] += got["stepped"]
            ref["term"][p, h + 1] = got["terminal"]
        ref["obs"][p], ref["terminal"][p] = got["obs"], got["terminal"]
        eng.snapshot_restore(SLOT, None)
    ref["ret"] = ret_of(ref["reward"], gamma)
    return ref


def assert_equal(got, ref, tag):
    for k in ("obs", "terminal", "stepped"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s: %s" % (tag, k))
    for k in ("reward", "ret"):
        np.testing.assert_array_equal(got[k].view(np.uint64), ref[k].view(np.uint64), err_msg="%s: %s" % (tag, k))


def new_seen():
    return {"checked": 0, "ends_inside": False, "ret_differs": False, "obs_differs": False, "dry": False, "terminal_1": False, "over": False}


def rollout_against_the_steps(r, rolls, P, H, tag, seen, gamma=0.97, plans=None):
    plans = random_plans(r.rng, P, H, r.B) if plans is None else plans
    got = rolls.get(P, H).rollout(r.eng, plans, gamma)
    ref = composed(r, plans, gamma)
    assert_equal(got, ref, "%s P=%d H=%d" % (tag, P, H))
    t = ref["term"]
    live = t[0, 0] == 0
    ends = (t[:, :-1] == 0) & (t[:, 1:] != 0)   # [P][H][B]: the book's episode ends in plan step h
    seen["checked"] += 1
    seen["ends_inside"] |= bool(ends[:, 1:max(1, H - 1)].any())   # 0 < h < H - 1
    seen["ret_differs"] |= bool((live & (got["ret"].view(np.uint64) != got["ret"].view(np.uint64)[0]).any(0)).any())
    seen["obs_differs"] |= bool((live & (got["obs"].view(np.uint32) != got["obs"].view(np.uint32)[0]).any((0, 2))).any())
    seen["dry"] |= bool((ends & (t[:, 1:] == 2)).any())
    seen["terminal_1"] |= bool((ends & (t[:, 1:] == 1)).any())
    seen["over"] |= bool((~live).any())
    assert (got["stepped"][:, ~live] == 0).all(), tag + ": a book that was over has been stepped"
    return got, ref


def scouted_to_the_end(r, rolls, tag, k, seen, shapes, tail):
    """The run's oracle plays the episode first (tests/test_gpu_vec_peek.py scout); the engine then takes the same actions, and the
    look-ahead is checked against the real steps before every k-th step, before each of the last `tail` steps (books end in the
    middle of a plan) and once behind the last, where every book is over.  The (P, H) of `shapes` take turns."""
    acts, _ = scout(r.orc, r.rng, r.B)
    n = 0
    for s, a in enumerate(acts):
        if s % k == 0 or s >= len(acts) - tail:
            P, H = shapes[n % len(shapes)]
            rollout_against_the_steps(r, rolls, P, H, "%s before step %d" % (tag, s + 1), seen)
            n += 1
        r.dev.step(r.eng, a)
    np.testing.assert_array_equal(r.eng.get_terminal(), r.orc.recs()["book"]["terminal"], err_msg=tag + ": the engine's episode ends where the oracle's does")
    for P, H in shapes[-2:]:
        rollout_against_the_steps(r, rolls, P, H, tag + " at the end", seen)
    return len(acts)


# ---- 1. against the real steps ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,depth,trades,ending", [(1, 5, 2, "dry"), (1, 10, 3, "session"), (63, 10, 2, "session"), (63, 5, 3, "dry"),
                                                   (65, 5, 2, "session"), (65, 10, 3, "dry"), (300, 10, 2, "dry"), (300, 5, 3, "session")])
def test_against_the_real_steps(B, depth, trades, ending):
    r = Run(B, ending, seed=40, p=make_params(depth, trades))
    rolls = Rolls(B, r.V)
    seen = new_seen()
    tag = "B=%d D=%d T=%d %s" % (B, depth, trades, ending)
    steps = scouted_to_the_end(r, rolls, tag, 5, seen, SHAPES, max(H for _, H in SHAPES) + 2)
    term = r.eng.get_terminal()
    assert steps > 10 and ((term == 2).all() if ending == "dry" else (term == 1).all()), (steps, term)
    assert seen["ends_inside"], tag + ": a book whose episode ends at a plan step 0 < h < H - 1 (a condition on the seed)"
    assert seen["ret_differs"] and seen["obs_differs"], tag + ": a live book with two plans whose ret / obs differ (a condition on the seed)"
    assert seen["dry" if ending == "dry" else "terminal_1"], tag + ": the episode's kind of ending inside a plan (a condition on the seed)"
    assert seen["checked"] > steps // 5 and seen["over"]
    rolls.free()
    r.close()


# ---- 2. H = 1 is lob_vec_peek ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [65, 300])
def test_horizon_one_equals_peek(B):
    r = Run(B, "dry", seed=41)
    dp, dr = DevPeek(B, r.V), DevRoll(B, r.V, N, 1)
    plans = np.broadcast_to(np.arange(N, dtype=np.int32)[:, None, None], (N, 1, B))
    for point in ("early", "middle", "books over"):   # after 3 steps, 40 steps on, and once the first books have run dry
        for _ in range({"early": 3, "middle": 40}.get(point, 0)):
            r.step(1)
        while point == "books over" and (r.eng.get_terminal() == 0).all():
            r.step(1)
        live = r.eng.get_terminal() == 0
        pk = dp.peek(r.eng)
        got = dr.rollout(r.eng, plans, 1.0)
        for k in ("obs", "terminal", "stepped"):
            np.testing.assert_array_equal(got[k], pk[k], err_msg="%s: %s" % (point, k))
        np.testing.assert_array_equal(got["reward"][:, 0].view(np.uint64), pk["reward"].view(np.uint64), err_msg=point + ": reward")
        np.testing.assert_array_equal(got["ret"].view(np.uint64), (pk["reward"] + 0.0).view(np.uint64), err_msg=point + ": ret of one step")
        assert live.any() and got["stepped"].any(), point
    assert not live.all(), "the last point has books that are over"
    dp.free()
    dr.free()
    r.close()


# ---- 3. against the oracle directly ------------------------------------------------------------------------------------------------------

def test_against_the_oracle_directly():
    """B = 65, P = 3, H = 4; the scout picks at most ten steps: eight spread over the episode, the one two steps in front of the first
    step in which a book runs dry (so that it runs dry inside a plan) and the one in front of that step itself."""
    B, P, H = 65, 3, 4
    r = Run(B, "dry", seed=42)
    dr = DevRoll(B, r.V, P, H)
    sc = r.new_oracle()
    sc.reset()
    acts, ends = scout(sc, r.rng, B)
    sc.close()
    first_dry = ends.index(True)
    assert first_dry >= 2
    chosen = set(list(range(3, len(acts), max(1, len(acts) // 8)))[:8]) | {first_dry - 2, first_dry}
    assert 8 <= len(chosen) <= 10, (sorted(chosen), len(acts))
    seen_dry_inside = seen_stepped = False
    for s, act in enumerate(acts):
        if s in chosen:
            plans = random_plans(r.rng, P, H, B)
            got = dr.rollout(r.eng, plans, 1.0)
            for p in range(P):
                o = r.new_oracle()
                o.reset()
                for a in acts[:s]:
                    o.env_step(a)
                stepped = np.zeros(B, np.int32)
                for h in range(H):
                    t0 = o.recs()["book"]["terminal"]
                    n0 = o.counters()[0]
                    o.env_step(plans[p, h])
                    recs = o.recs()
                    st = (t0 == 0) & (recs["book"]["terminal"] != 2)   # (a step that runs dry is the one way a live book does not step)
                    assert int(st.sum()) == int(o.counters()[0] - n0), "the oracle's step counter"
                    tag = "before step %d, plan %d, step %d" % (s + 1, p, h)
                    np.testing.assert_array_equal(got["reward"][p, h][st], recs["reward"][st], err_msg=tag + ": reward of the books that stepped")
                    assert (got["reward"][p, h][~st].view(np.uint64) == 0).all(), tag
                    stepped += st
                    seen_dry_inside |= bool(((t0 == 0) & ~st).any() and 0 < h)
                    seen_stepped |= bool(st.any())
                tag = "before step %d, plan %d" % (s + 1, p)
                np.testing.assert_array_equal(got["stepped"][p], stepped, err_msg=tag + ": stepped")
                np.testing.assert_array_equal(got["obs"][p], recs["vars"][:, :r.V], err_msg=tag + ": obs")
                np.testing.assert_array_equal(got["terminal"][p], recs["book"]["terminal"], err_msg=tag + ": terminal")
                o.close()
        r.dev.step(r.eng, act)
        r.orc.env_step(act)
    assert seen_stepped and seen_dry_inside
    dr.free()
    r.close()


# ---- 4. leaves nothing behind; the window ring ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lb_pnl", [0, 1, 3, 8], ids=["pnl", "normed-1", "normed-3", "normed-8"])
@pytest.mark.parametrize("B", [65, 300])
def test_leaves_nothing_behind_and_the_window_ring(B, lb_pnl):
    """A look-ahead of P = 2, H = 5 in front of EVERY step: the dumps, getters and counters right before and right after it are the
    same, and the engine stays equal to the oracle under the same actions at every step to the end; at every 4th step the look-ahead
    equals the composed route.  lb_pnl 0: the PnL reward (no window is read).  NORMED reads the two PnL windows: lb_pnl 1 -- the entry
    a push replaces is the plan's previous push; 3 < H -- the plan's own pushes of three steps back, the window wrapped by the plan;
    8 >= H -- the engine's memory only."""
    P, H = 2, 5
    p = make_params(5, 2)
    if lb_pnl:
        p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, lb_pnl
    r = Run(B, "dry", seed=43, p=p)
    dr = DevRoll(B, r.V, P, H)
    steps, extra_steps, extra_events = 0, 0, 0
    full_first = full_last = nonzero_step = False
    ones = np.ones(B, bool)
    while True:
        before_dump = bytes(r.eng.get_books())
        before = {"state": r.eng.get_state().tobytes(), "reward": r.eng.get_reward().tobytes(), "counters": tuple(r.eng.counters())}
        plans = random_plans(r.rng, P, H, B)
        got = dr.rollout(r.eng, plans, 0.97)
        assert bytes(r.eng.get_books()) == before_dump, "step %d: the look-ahead changed the books" % steps
        after = {"state": r.eng.get_state().tobytes(), "reward": r.eng.get_reward().tobytes(), "counters": tuple(r.eng.counters())}
        assert after == before, "step %d: the look-ahead changed lob_get_state / lob_get_reward / the counters" % steps
        if steps % 4 == 0:
            c0 = r.eng.counters()
            assert_equal(got, composed(r, plans, 0.97), "B=%d lb_pnl=%d before step %d" % (B, lb_pnl, steps + 1))
            c1 = r.eng.counters()   # (the composed route's own steps are counted by the engine and not by the oracle)
            extra_steps, extra_events = extra_steps + int(c1[0] - c0[0]), extra_events + int(c1[1] - c0[1])
            full_first |= bool((got["reward"][:, 0] != 0.0).any())
            full_last |= bool((got["reward"][:, H - 1] != 0.0).any())
        got = r.step(1)
        steps += 1
        check_step(r.eng, r.orc, got, r.V, 0, "B=%d lb_pnl=%d step %d behind a look-ahead" % (B, lb_pnl, steps), books=ones)
        c, oc = r.eng.counters(), r.orc.counters()
        assert c[0] - extra_steps == oc[0] and c[1] - extra_events == oc[1], (steps, c, oc, extra_steps, extra_events)
        nonzero_step |= bool((got["reward"] != 0.0).any())
        if int(got["n_live"][0]) == 0:
            break
        assert steps < 600
    # (NORMED is 0 until both windows are full: a nonzero reward in a checked look-ahead's first step means they were full at its
    # entry, in its last step that they were still full four pushes on)
    # A window of ONE entry has no deviation (s / (cnt - 1) is x / 0: NaN or inf, and get_reward turns both into 0): that measure is
    # 0 throughout, so there the asserts are that the episode ran; the window is full from the second step on.
    assert steps > 20 and (lb_pnl == 1 or (nonzero_step and full_first and full_last))
    dr.free()
    r.close()


# ---- 5. every reward measure --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", sorted(abi.REWARD_NAMES, key=abi.REWARD_NAMES.get))
def test_every_reward_measure(measure):
    B = 65
    p = make_params(5, 2)
    p.reward_measure = abi.REWARD_NAMES[measure]
    if p.reward_measure == abi.REWARD_NORMED:
        p.lb_pnl = 3
    r = Run(B, "dry", seed=44, p=p)
    rolls = Rolls(B, r.V)
    seen = new_seen()
    steps = scouted_to_the_end(r, rolls, "measure " + measure, 7, seen, [(3, 4)], 6)
    assert steps > 10 and seen["obs_differs"] and seen["dry"] and seen["ends_inside"]
    if p.reward_measure != abi.REWARD_NONE:
        assert seen["ret_differs"], measure + ": the returns of two plans of some live book differ"
    rolls.free()
    r.close()


# ---- 6. skips -------------------------------------------------------------------------------------------------------------------------------

def test_actions_out_of_range_skip_the_step_and_are_not_counted():
    B, P, H = 65, 4, 6
    r = Run(B, "dry", seed=45)
    rolls = Rolls(B, r.V)
    r.step(9)
    I32MIN = np.iinfo(np.int32).min
    plans = random_plans(r.rng, P, H, B)
    holes = r.rng.random((P, H, B)) < 0.3
    plans[holes] = r.rng.choice(np.array([-1, 9, I32MIN], np.int32), size=int(holes.sum()))
    assert all((plans == v).any() for v in (-1, 9, I32MIN)) and (plans[:, 0] < 0).any() and (plans[:, -1] < 0).any()
    seen = new_seen()
    got, ref = rollout_against_the_steps(r, rolls, P, H, "plans with holes", seen, plans=plans)
    live = r.eng.get_terminal() == 0
    valid = ((plans >= 0) & (plans < N)).sum(1)   # [P][B]
    np.testing.assert_array_equal(got["stepped"][:, live], valid[:, live], err_msg="a live book far from the end steps once per valid action")
    assert live.all() and (got["stepped"] < H).any() and (got["stepped"] > 0).any()
    rc, n = r.eng.vec_status()   # (the yardstick's steps have counted theirs)
    assert rc == abi.LOB_EINVAL and n == int(holes.sum())
    rolls.get(P, H).rollout(r.eng, plans)
    assert r.eng.vec_status() == (abi.LOB_OK, 0), "a look-ahead alone counts nothing"
    # a plan of skips only: nothing steps, the engine's present observation and terminal come back
    obs0, term0 = r.observe()["obs"], r.eng.get_terminal()
    got = rolls.get(2, 3).rollout(r.eng, np.full((2, 3, B), -1, np.int32), 0.5)
    assert (got["stepped"] == 0).all() and (got["reward"].view(np.uint64) == 0).all() and (got["ret"].view(np.uint64) == 0).all()
    for p in range(2):
        np.testing.assert_array_equal(got["obs"][p], obs0)
        np.testing.assert_array_equal(got["terminal"][p], term0)
    assert r.eng.vec_status() == (abi.LOB_OK, 0)
    rolls.free()
    r.close()


# ---- 7. ret ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", [0.0, 0.97, 1.0])
def test_ret_is_the_discount_loop_over_the_rewards(gamma):
    B, P, H = 65, 5, 9
    r = Run(B, "dry", seed=46)
    dr = DevRoll(B, r.V, P, H)
    r.step(25)
    plans = random_plans(r.rng, P, H, B)
    plans[1, 2:5] = -1   # (the discount follows h whether or not the step completed)
    got = dr.rollout(r.eng, plans, gamma)
    assert (got["reward"] != 0.0).any() and (got["reward"][1, 2:5].view(np.uint64) == 0).all() and (got["reward"][1, 5:] != 0.0).any()
    np.testing.assert_array_equal(got["ret"].view(np.uint64), ret_of(got["reward"], gamma).view(np.uint64))
    if gamma == 0.0:
        np.testing.assert_array_equal(got["ret"].view(np.uint64), (got["reward"][:, 0] + 0.0).view(np.uint64))
    dr.free()
    r.close()


# ---- 8. members and neighbours -------------------------------------------------------------------------------------------------------------

def test_null_members_and_the_neighbours_of_the_buffers():
    B, P, H = 65, 3, 4
    r = Run(B, "dry", seed=47)
    r.step(9)
    plans = random_plans(r.rng, P, H, B)
    dr = DevRoll(B, r.V, P, H)
    ref = dr.rollout(r.eng, plans, 0.9)
    assert all((v.view(np.uint8) != 0xAB).any() for v in ref.values())
    for want in [(k,) for k in KEYS] + [("ret", "terminal")]:
        part = DevRoll(B, r.V, P, H, want=want)
        got = part.rollout(r.eng, plans, 0.9)
        for k in KEYS:
            if k in want:
                np.testing.assert_array_equal(got[k].view(np.uint8), ref[k].view(np.uint8), err_msg="members %s: %s" % (want, k))
            else:
                assert (got[k].view(np.uint8) == 0xAB).all(), "members %s: %s is NULL and was written" % (want, k)
        part.free()
    r.eng.vec_rollout(dr.plans.ptr, P, H, 0.9, abi.VecRolloutOut(None, None, None, None, None))   # nothing wanted: LOB_OK
    dr.free()
    r.close()


# ---- 9. other settings ---------------------------------------------------------------------------------------------------------------------

def random_to_the_end(r, rolls, tag, k, seen, shapes, cap=600):
    """Without an oracle in the engine's state: random actions until no book is live; checked before every k-th step and before every
    step from the first one at which a book is over."""
    steps = n = 0
    while True:
        n_live = int((r.eng.get_terminal() == 0).sum())
        if n_live == 0:
            break
        if steps % k == 0 or n_live < r.B:
            P, H = shapes[n % len(shapes)]
            rollout_against_the_steps(r, rolls, P, H, "%s before step %d" % (tag, steps + 1), seen)
            n += 1
        r.dev.step(r.eng, r.rng.integers(0, N, size=r.B).astype(np.int32))
        steps += 1
        assert steps < cap, tag + ": the episode did not end"
    return steps


def test_after_a_masked_restore():
    B = 65
    r = Run(B, "dry", seed=48)
    rolls = Rolls(B, r.V)
    r.step(7)
    r.save(0)
    r.step(12)
    m = np.random.default_rng(49).integers(0, 2, size=B).astype(bool)
    assert m.any() and not m.all()
    r.restore(0, m)
    seen = new_seen()
    steps = random_to_the_end(r, rolls, "after a masked restore", 6, seen, [(3, 4), (2, 6)])
    assert steps > 10 and seen["ret_differs"] and seen["obs_differs"] and seen["dry"]
    rolls.free()
    r.close()


def test_day_library_with_days_of_unequal_length():
    B, lengths = 65, (100, 150, 200)
    p = make_params(5, 2)
    days = make_days(lengths, depth=5)
    assign = ((np.arange(B) * 7) % 3).astype(np.int32)
    r = Run(B, "dry", seed=50, p=p, reset=False)
    r.eng.load_days(days)
    r.eng.days_set(assign)
    r.eng.reset()
    np.testing.assert_array_equal(r.eng.days(), assign)
    rolls = Rolls(B, r.V)
    seen = new_seen()
    steps = random_to_the_end(r, rolls, "day library", 8, seen, [(3, 4), (2, 6)])
    assert steps > 10 and (r.eng.get_terminal() == 2).all()
    assert seen["ret_differs"] and seen["obs_differs"] and seen["dry"] and seen["ends_inside"]
    rolls.free()
    r.close()


def test_above_the_16_lane_env_kernel():
    """5 000 books at depth 10 (above the 4 096 up to which lob_vec_step runs the 16-lane env kernel: the yardstick's steps go through
    the 64-lane one), 79 blocks per plan with a partial last one.  (A small weight vector: the private weights of 5 000 books are not
    what this test is about.)"""
    B = 5000
    r = Run(B, "dry", depth=10, seed=51, mem=1 << 12)
    rolls = Rolls(B, r.V)
    seen = new_seen()
    for step in range(31):
        if step % 10 == 0:
            rollout_against_the_steps(r, rolls, 2, 3, "B=5000 before step %d" % (step + 1), seen)
        r.dev.step(r.eng, r.rng.integers(0, N, size=B).astype(np.int32))
    assert seen["checked"] == 4 and seen["ret_differs"] and seen["obs_differs"]
    rolls.free()
    r.close()


@pytest.mark.parametrize("P,H", [(abi.MAX_ROLLOUT_PLANS, 1), (1, abi.MAX_ROLLOUT_STEPS)])
def test_at_the_limits(P, H):
    """The most plans, and the longest plan -- that one under the NORMED reward over windows of three steps, which the plan wraps
    twenty times, to the end of the episode and beyond."""
    B = 65
    p = make_params(5, 2)
    if H > 1:
        p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, 3
    r = Run(B, "dry", seed=52, p=p)
    rolls = Rolls(B, r.V)
    r.step(6 if H == 1 else 30)   # (an episode here is some 70 steps: the longest plan starts in its middle)
    seen = new_seen()
    got, _ = rollout_against_the_steps(r, rolls, P, H, "at the limits", seen)
    assert H == 1 or seen["dry"], "the longest plan reaches the end of the episode"
    assert (got["reward"] != 0.0).any() and got["stepped"].max() > min(H, 20) - 1
    rolls.free()
    r.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------------

def refused(code, fn, *args):
    with pytest.raises(LobError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert b"lob_vec_rollout" in abi.load().lob_last_error()
    return str(ei.value)


def steps_on_equal_to_the_oracle(r, n, tag):
    for i in range(n):
        before = r.orc.counters()[0]
        got = r.step(1)
        check_step(r.eng, r.orc, got, r.V, before, "%s, step %d" % (tag, i + 1))


def test_refusals():
    B, P, H = 65, 2, 3
    r = Run(B, "dry", seed=53, reset=False)
    eng, lib = r.eng, abi.load()
    dr = DevRoll(B, r.V, P, H)
    dr.plans.upload(random_plans(r.rng, P, H, B))
    refused(abi.LOB_ESTATE, eng.vec_rollout, dr.plans.ptr, P, H, 1.0, dr.out)   # before the first lob_reset
    r.reset()
    r.step(3)
    books = bytes(eng.get_books())
    vp = C.c_void_p
    assert lib.lob_vec_rollout(eng.h, vp(dr.plans.ptr), P, H, 1.0, None) == abi.LOB_EINVAL and b"lob_vec_rollout" in lib.lob_last_error()
    assert lib.lob_vec_rollout(None, vp(dr.plans.ptr), P, H, 1.0, C.byref(dr.out)) == abi.LOB_EINVAL and b"lob_vec_rollout" in lib.lob_last_error()
    assert lib.lob_vec_rollout(eng.h, None, P, H, 1.0, C.byref(dr.out)) == abi.LOB_EINVAL and b"lob_vec_rollout" in lib.lob_last_error()
    for n_plans, horizon in ((0, H), (-1, H), (abi.MAX_ROLLOUT_PLANS + 1, H), (P, 0), (P, -1), (P, abi.MAX_ROLLOUT_STEPS + 1)):
        refused(abi.LOB_EINVAL, eng.vec_rollout, dr.plans.ptr, n_plans, horizon, 1.0, dr.out)
    for gamma in (float("nan"), -0.01, 1.0000001, float("inf"), float("-inf")):
        refused(abi.LOB_EINVAL, eng.vec_rollout, dr.plans.ptr, P, H, gamma, dr.out)
    if eng.td_split_supported():
        eng.td_step_begin()
        refused(abi.LOB_ESTATE, eng.vec_rollout, dr.plans.ptr, P, H, 1.0, dr.out)
        eng.td_step_end()
        r.orc.td_step(1)
        books = bytes(eng.get_books())
    eng.sync()
    assert bytes(eng.get_books()) == books, "a refused call changed the books"
    assert all((v.view(np.uint8) == 0xAB).all() for v in dr.read(eng).values()), "a refused call wrote"
    steps_on_equal_to_the_oracle(r, 5, "after the refusals")
    dr.free()
    r.close()


def test_ring_mode_is_refused(monkeypatch):
    """A market track that is a ring (tests/test_gpu_snapshot.py's switches): LOB_ESTATE, and the engine steps on."""
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    B, P, H = 64, 2, 3
    r = Run(B, "dry", depth=10, seed=54, n_events=1200)
    dr = DevRoll(B, r.V, P, H)
    dr.plans.upload(random_plans(r.rng, P, H, B))
    r.step(3)
    books = bytes(r.eng.get_books())
    assert "ring" in refused(abi.LOB_ESTATE, r.eng.vec_rollout, dr.plans.ptr, P, H, 1.0, dr.out)
    assert bytes(r.eng.get_books()) == books
    assert all((v.view(np.uint8) == 0xAB).all() for v in dr.read(r.eng).values()), "a refused call wrote"
    steps_on_equal_to_the_oracle(r, 20, "ring mode, after the refusal")
    dr.free()
    r.close()


# ---- 11. the torch face ----------------------------------------------------------------------------------------------------------------------

def test_vec_env_rollout_through_torch():
    """tests/vec_rollout_torch_child.py, in a process of its own: torch must be imported before the engine library is loaded."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vec_rollout_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "vec_rollout_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "rollout OK" in res.stdout
