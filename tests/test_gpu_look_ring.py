"""Look-aheads on a ring-mode stream (include/lob_engine.h lob_look_ring / lob_track_window): lob_vec_peek,
lob_vec_rollout, lob_branch_* and lob_branch_book / lob_branch_history over a market track that is a ring of 256 entries refilled
every 16 steps.

The yardstick is the path the existing suites pin: a second engine on the same records and parameters whose track is resident
(LOB_TRACK_RING=4096) and whose switch is off.  Every comparison is for equality of every byte.  What the inputs must provide -- no cell
beyond the window in test 2, the wall within the step budget in test 5 -- is checked on the CPU by tests/test_look_ring_cases.py."""
import ctypes as C

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from rl_markets_amd.engine import LobError
from tests import look_ring_cases as lc
from tests.test_gpu_branch_obs import DevObs
from tests.test_gpu_snapshot import Run
from tests.test_gpu_vec_branch import DevBranch
from tests.test_gpu_vec_env import DevVec, check_step
from tests.test_gpu_vec_peek import DevPeek
from tests.test_gpu_vec_rollout import DevRoll, ret_of

pytestmark = pytest.mark.gpu
N = lc.N
AHEAD, BEHIND = abi.TERMINAL_AHEAD, abi.TERMINAL_BEHIND


def ring_env(mp, ring=lc.RING, refill=lc.REFILL):
    """The switches an engine reads when it is created."""
    mp.setenv("LOB_TRACK_RING", str(ring))
    mp.setenv("LOB_TRACK_REFILL", str(refill))


class Twin:
    """A second engine on a Run's records and parameters, created under the switches in force."""

    def __init__(self, r, days=None):
        """days: a day library in place of the Run's records; the caller selects the days and resets."""
        self.B, self.V, self.D, self.p = r.B, r.V, r.D, r.p
        self.eng = engine.Engine(r.p, r.B)
        if days is None:
            self.eng.load_events(r.rec)
            self.eng.reset()
        else:
            self.eng.load_days(days)
        self.dev = DevVec(r.B, r.V)

    def close(self):
        self.dev.free()
        self.eng.close()


def pair(mp, B, depth, trades, normed=False, refill=lc.REFILL, twin_ring=4096, mixed=True, move_div=1, seed=lc.SEED):
    """-> (the ring engine as a Run with its oracle, the resident twin)."""
    p = lc.make_params(depth, trades, normed)
    rec = lc.records(p, B, mixed, move_div)
    ring_env(mp, refill=refill)
    r = Run(B, p=p, rec=rec, seed=seed)
    r.rng = lc.step_rng(B, seed)
    ring_env(mp, ring=twin_ring, refill=refill)
    tw = Twin(r)
    return r, tw


class Look:
    """The buffers of one engine's look-aheads, and all of them in one call."""

    def __init__(self, r, n_br=N):
        B, V = r.B, r.V
        self.peek = DevPeek(B, V)
        self.short, self.long = DevRoll(B, V, *lc.SHORT), DevRoll(B, V, *lc.LONG)
        self.br = DevBranch(B, V, n_br)
        self.obs = DevObs(B, r.D, r.p.max_trades, n_br, lc.K_HIST)

    def all(self, eng, plans, long_plans, br_actions):
        got = {"peek." + k: v for k, v in self.peek.peek(eng).items()}
        got.update({"short." + k: v for k, v in self.short.rollout(eng, plans, 0.97).items()})
        if long_plans is not None:
            got.update({"long." + k: v for k, v in self.long.rollout(eng, long_plans, 0.97).items()})
        got.update({"fork." + k: v for k, v in self.br.fork(eng).items()})
        got.update({"branch." + k: v for k, v in self.br.step(eng, br_actions).items()})
        got.update({"obs." + k: v for k, v in self.obs.call(eng).items()})
        return got

    def free(self):
        for b in (self.peek, self.short, self.long, self.br, self.obs):
            b.free()


def same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s: %s differs between the ring and the resident track" % (tag, k)


def terminals(got):
    return np.concatenate([v.ravel() for k, v in got.items() if k.endswith(".terminal")])


def ring_against_resident(r, tw, tag, cap=1500):
    """Both engines to the end of the day under the same actions, every look-ahead compared before every step."""
    la, lb = Look(r), Look(tw)
    lrng = lc.look_rng(r.B)
    seen = {"steps": 0, "tail": False, "terminal": set(), "refills_scheduled": 0}
    while True:
        s = seen["steps"]
        plans = lrng.integers(0, N, size=lc.SHORT + (r.B,)).astype(np.int32)
        long_plans = lc.long_plans(lrng, r.B) if s % 8 == 0 else None
        br_actions = lrng.integers(-1, N, size=(N, r.B)).astype(np.int32)
        ga, gb = la.all(r.eng, plans, long_plans, br_actions), lb.all(tw.eng, plans, long_plans, br_actions)
        same(ga, gb, "%s before step %d" % (tag, s + 1))
        t = terminals(ga)
        assert not ((t == AHEAD) | (t == BEHIND)).any(), "%s before step %d: a cell outside the window" % (tag, s + 1)
        seen["terminal"] |= set(int(x) for x in np.unique(t))
        term = r.eng.get_terminal()
        if s % 4 == 0:
            lo, hi, comp = r.eng.track_window()
            assert (lo <= r.eng.track_cursor()).all(), "the real cursor is inside the window"
            seen["tail"] |= bool(((comp == 1) & (term == 0) & (hi > lc.RING)).any())
        if not (term == 0).any():
            break
        assert s < cap, tag + ": the episode did not end"
        a = r.rng.integers(0, N, size=r.B).astype(np.int32)
        r.dev.step(r.eng, a)
        tw.dev.step(tw.eng, a)
        seen["steps"] += 1
        if seen["steps"] % 32 == 0:
            assert bytes(r.eng.get_books()) == bytes(tw.eng.get_books()), tag + ": the real books of the two engines"
    assert bytes(r.eng.get_books()) == bytes(tw.eng.get_books()), tag + ": the real books of the two engines at the end"
    rc, bad = r.eng.vec_status()
    assert rc == abi.LOB_OK and r.eng.look_counts() == (0, 0), (rc, bad, r.eng.look_counts())
    la.free()
    lb.free()
    return seen


def refusal(fn, *args):
    with pytest.raises(LobError) as ei:
        fn(*args)
    assert ei.value.code == abi.LOB_ESTATE, (ei.value.code, str(ei.value))
    return str(ei.value)


# ---- 1. off by default, and off again ------------------------------------------------------------------------------------------------------

def test_off_by_default_and_off_again(monkeypatch):
    B = 64
    r, tw = pair(monkeypatch, B, 10, 2, mixed=False)
    lk, lt = Look(r, 2), Look(tw, 2)
    r.step(3)
    plans = lc.look_rng(B).integers(0, N, size=lc.SHORT + (B,)).astype(np.int32)
    lk.short.plans.upload(plans)
    eng = r.eng
    ring_text = ": the market track of this stream is a ring (longer than LOB_TRACK_RING events)"

    def look_aheads_refused():
        assert refusal(eng.vec_peek, abi.PEEK_ALL, lk.peek.out).endswith("lob_vec_peek" + ring_text)
        assert refusal(eng.vec_rollout, lk.short.plans.ptr, lc.SHORT[0], lc.SHORT[1], 1.0, lk.short.out).endswith("lob_vec_rollout" + ring_text)
        assert refusal(eng.branch_fork, 2, lk.br.out).endswith("lob_branch_fork" + ring_text)
        assert refusal(eng.branch_book, lk.obs.book_out).endswith("lob_branch_book" + ring_text)

    def snapshots_refused():
        assert "entries before the cursor are gone" in refusal(eng.snapshot_save, 0, None)
        assert "entries before the cursor are gone" in refusal(eng.snapshot_restore, 0, None)

    look_aheads_refused()
    snapshots_refused()
    eng.look_ring(True)
    snapshots_refused()
    lk.peek.peek(eng)
    lk.short.rollout(eng, plans)
    lk.br.fork(eng)
    lk.obs.call(eng)
    r.reset()   # the switch survives lob_reset
    r.step(3)
    lk.peek.peek(eng)
    eng.look_ring(False)
    look_aheads_refused()
    snapshots_refused()
    # a resident track: the switch changes no output bit
    for _ in range(3):
        tw.dev.step(tw.eng, r.hist[_])
    before = lt.peek.peek(tw.eng)
    tw.eng.look_ring(True)
    lo, hi, comp = tw.eng.track_window()
    assert (lo == 0).all() and (comp == 1).all() and (hi > 0).all()
    same(before, lt.peek.peek(tw.eng), "resident, the switch on")
    lib = abi.load()
    assert lib.lob_look_ring(None, 1) == abi.LOB_EINVAL and lib.lob_track_window(eng.h, None, None, None) == abi.LOB_EINVAL
    lk.free()
    lt.free()
    tw.close()
    r.close()


# ---- 2. ring against resident, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,depth,trades,normed", lc.CONFIGS)
def test_ring_against_resident(monkeypatch, B, depth, trades, normed):
    r, tw = pair(monkeypatch, B, depth, trades, normed)
    r.eng.look_ring(True)
    seen = ring_against_resident(r, tw, "B=%d D=%d T=%d" % (B, depth, trades))
    assert seen["steps"] >= 300, seen
    assert seen["tail"], "books whose pre-pass is complete were still stepping at a compared step"
    assert {0, 1, 2} <= seen["terminal"], seen
    tw.close()
    r.close()


# ---- 3. nothing of the engine moves ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,depth,trades,normed", lc.CONFIGS[:2])
def test_nothing_of_the_engine_moves(monkeypatch, B, depth, trades, normed):
    """Look-aheads in front of every step shift the refill schedule; the books equal, byte for byte, those of a ring engine that made
    no such call, and the oracle's to the end of the day."""
    r, quiet = pair(monkeypatch, B, depth, trades, normed, twin_ring=lc.RING)
    r.eng.look_ring(True)
    lk = Look(r)
    lrng = lc.look_rng(B)
    steps = 0
    while (r.eng.get_terminal() == 0).any():
        lk.all(r.eng, lrng.integers(0, N, size=lc.SHORT + (B,)).astype(np.int32), lc.long_plans(lrng, B) if steps % 8 == 0 else None,
               lrng.integers(-1, N, size=(N, B)).astype(np.int32))
        before = r.orc.counters()[0]
        got = r.step(1)
        quiet.dev.step(quiet.eng, r.hist[-1])
        steps += 1
        if steps % 4 == 0 or steps < 40:
            assert bytes(r.eng.get_books()) == bytes(quiet.eng.get_books()), "step %d: against the engine without look-aheads" % steps
            check_step(r.eng, r.orc, got, r.V, before, "step %d" % steps)
        if steps % 16 == 0:
            assert r.eng.vec_status() == (abi.LOB_OK, 0)
        assert steps < 1500
    assert bytes(r.eng.get_books()) == bytes(quiet.eng.get_books())
    assert r.eng.vec_status() == (abi.LOB_OK, 0) and steps >= 300
    lk.free()
    quiet.close()
    r.close()


# ---- 4. a branch that follows the real books stays in the window ----------------------------------------------------------------------------

def test_a_branch_in_lock_step_and_one_left_behind(monkeypatch):
    B = 70
    r, tw = pair(monkeypatch, B, 10, 2, twin_ring=lc.RING)
    tw.close()
    eng = r.eng
    eng.look_ring(True)
    db = DevBranch(B, r.V, 2)
    r.step(5)
    fork = db.fork(eng)
    k_fork, term_fork = eng.track_cursor(), fork["terminal"][1].copy()
    seen_behind = 0
    for s in range(300):
        a = r.rng.integers(0, N, size=B).astype(np.int32)
        got = db.step(eng, np.stack([a, np.full(B, -1, np.int32)]))
        lo, hi, comp = eng.track_window()   # (the window the launch saw: the call's refill is in front of it)
        r.dev.step(eng, a)
        real = r.dev.read(eng)
        tag = "step %d" % (s + 1)
        for k in ("obs", "reward", "terminal", "stepped"):
            assert got[k][0].tobytes() == real[k].tobytes(), "%s: %s of the branch in lock step" % (tag, k)
        behind = (term_fork == 0) & (k_fork < lo)
        np.testing.assert_array_equal(got["terminal"][1], np.where(behind, BEHIND, term_fork), err_msg=tag + ": the branch left at the fork")
        assert got["obs"][1].tobytes() == fork["obs"][1].tobytes() and not got["stepped"][1].any() and not got["reward"][1].view(np.uint64).any()
        seen_behind += int(behind.sum())
    assert seen_behind > 0 and behind.any()
    rc, _ = eng.vec_status()
    assert rc == abi.LOB_OK and eng.look_counts() == (0, seen_behind)
    # select(parent = 0): the branch left behind becomes the one in lock step
    sel = db.select(eng, np.zeros((2, B), np.int32))
    assert sel["obs"][1].tobytes() == sel["obs"][0].tobytes() and sel["terminal"][1].tobytes() == sel["terminal"][0].tobytes()
    a = r.rng.integers(0, N, size=B).astype(np.int32)
    got = db.step(eng, np.stack([a, a]))
    for k in got:
        assert got[k][0].tobytes() == got[k][1].tobytes(), k
    assert not (got["terminal"] >= AHEAD).any()
    got = db.fork(eng)
    got = db.step(eng, np.stack([a, a]))
    assert not (got["terminal"] >= AHEAD).any()
    db.free()
    r.close()


# ---- 5. running into the wall ----------------------------------------------------------------------------------------------------------------

def test_running_into_the_wall(monkeypatch):
    B = 70
    r, tw = pair(monkeypatch, B, 4, 3, mixed=False)
    eng = r.eng
    eng.look_ring(True)
    db = DevBranch(B, r.V, 2)
    for _ in range(20):
        r.step(1)
        tw.dev.step(tw.eng, r.hist[-1])
    db.fork(eng)
    obs_prev = None
    counted, wall, tw_out, a_wall = 0, None, None, None
    lrng = lc.look_rng(B)
    for s in range(lc.WALL_BUDGET):
        a = lrng.integers(0, N, size=B).astype(np.int32)
        live = tw.eng.get_terminal() == 0
        tw.dev.step(tw.eng, a)
        out = tw.dev.read(tw.eng)
        k_after = tw.eng.track_cursor()
        got = db.step(eng, np.stack([a, a]))
        lo, hi, comp = eng.track_window()
        ahead = live & (k_after > hi) & (comp == 0)   # the header's rule: the step needs the entries below k_after
        tag = "branch step %d" % (s + 1)
        for n in range(2):
            np.testing.assert_array_equal(got["terminal"][n] == AHEAD, ahead, err_msg=tag + ": terminal 3 exactly where the rule says")
            for k in ("obs", "reward", "terminal", "stepped"):
                assert got[k][n][~ahead].tobytes() == out[k][~ahead].tobytes(), "%s: %s against the twin's real step" % (tag, k)
            if ahead.any():
                assert got["obs"][n][ahead].tobytes() == obs_prev[n][ahead].tobytes() and not got["stepped"][n][ahead].any()
                assert not got["reward"][n][ahead].view(np.uint64).any()
        counted += 2 * int(ahead.sum())
        obs_prev = got["obs"].copy()
        if ahead.any():
            wall, tw_out, a_wall = ahead, out, a
            break
    assert wall is not None, "no branch reached the window's end within the budget"
    # a further call: 3 again, nothing moves (the other books stay where they are under -1)
    again = np.where(wall, a_wall, -1).astype(np.int32)
    got = db.step(eng, np.stack([again, again]))
    assert (got["terminal"][:, wall] == AHEAD).all() and got["obs"].tobytes() == obs_prev.tobytes() and not got["stepped"].any()
    counted += 2 * int(wall.sum())
    # the real books step on by 32: the window moves, the same call completes and equals the twin's step
    for _ in range(32):
        before = r.orc.counters()[0]
        real = r.step(1)
    check_step(eng, r.orc, real, r.V, before, "the real books behind the look-aheads")
    got = db.step(eng, np.stack([again, again]))
    for n in range(2):
        for k in ("obs", "reward", "terminal", "stepped"):
            assert got[k][n][wall].tobytes() == tw_out[k][wall].tobytes(), "%s of a branch behind the wall, once the window has moved" % k
    rc, bad = eng.vec_status()
    assert rc == abi.LOB_OK and bad == 0 and eng.look_counts() == (counted, 0)
    assert eng.vec_status() == (abi.LOB_OK, 0) and eng.look_counts() == (0, 0)
    steps = 0
    while (eng.get_terminal() == 0).any():
        before = r.orc.counters()[0]
        real = r.step(1)
        steps += 1
        if steps % 8 == 0:
            check_step(eng, r.orc, real, r.V, before, "to the end of the day, step %d" % steps)
    check_step(eng, r.orc, real, r.V, before, "the end of the day")
    db.free()
    tw.close()
    r.close()


def test_a_roll_out_into_the_wall(monkeypatch):
    """(1 plan, 64 steps) at steps_since_fill 15 under LOB_TRACK_REFILL=128, so that the host's rule does not refill, on a stream whose
    midprice moves four times less often: the plans run past the window's end.  Short `stepped`, `ret` and terminal 3 against the
    twin's prefix."""
    B, P, H, gamma = 70, 1, 64, 0.97
    r, tw = pair(monkeypatch, B, 10, 2, refill=128, mixed=False, move_div=4)
    r.eng.look_ring(True)
    for _ in range(15):
        r.step(1)
        tw.dev.step(tw.eng, r.hist[-1])
    hi0 = r.eng.track_window()[1]
    ra, rb = DevRoll(B, r.V, P, H), DevRoll(B, r.V, P, H)
    plans = lc.look_rng(B).integers(0, N, size=(P, H, B)).astype(np.int32)
    got, ref = ra.rollout(r.eng, plans, gamma), rb.rollout(tw.eng, plans, gamma)
    np.testing.assert_array_equal(r.eng.track_window()[1], hi0, err_msg="the host's rule did not refill")
    ahead = got["terminal"][0] == AHEAD
    assert ahead.any(), "no plan reached the window's end (a condition on the stream)"
    for k in got:
        keep = (~ahead,) if k == "obs" else (Ellipsis, ~ahead)
        assert got[k][0][keep].tobytes() == ref[k][0][keep].tobytes(), k + " of the plans inside the window"
    n = got["stepped"][0]
    assert (n[ahead] < ref["stepped"][0][ahead]).all()
    for b in np.flatnonzero(ahead):
        prefix = ref["reward"][0][:, b].copy()
        # the twin's steps complete one after the other from the first on (no -1 in the plan): the first n[b] rewards are the prefix
        prefix[n[b]:] = 0.0
        assert got["reward"][0][:, b].tobytes() == prefix.tobytes(), "book %d: the rewards of the completed steps, then +0.0" % b
        assert got["ret"][0][b].tobytes() == ret_of(prefix[None, :, None], gamma)[0, 0].tobytes(), "book %d: ret" % b
    rc, _ = r.eng.vec_status()
    assert rc == abi.LOB_OK and r.eng.look_counts() == (int(ahead.sum()), 0)
    ra.free()
    rb.free()
    tw.close()
    r.close()


# ---- 6. a day library of unequal days --------------------------------------------------------------------------------------------------------

def test_day_library_of_unequal_days(monkeypatch):
    """Days of 150 / 400 / 900 events at ring 256: the books of the short day are complete from the start with n_track < the ring.
    Two episodes, each with another assignment of the days -- set with lob_days_set on both engines, not drawn by lob_days_select: the
    two engines must play the same days, and every book must meet every kind of day, which a fixed rotation guarantees.  That no cell
    leaves the window is a property of the days (tests/test_look_ring_cases.py test_the_day_library_cannot_leave_the_window)."""
    B, depth, trades = 70, 10, 2
    p = lc.make_params(depth, trades)
    days = lc.make_days(depth, trades)
    ring_env(monkeypatch)
    r = Run(B, p=p, seed=lc.SEED, reset=False)
    ring_env(monkeypatch, ring=1024)
    tw = Twin(r, days=days)
    r.eng.load_days(days)
    r.eng.look_ring(True)
    for episode in range(2):
        assign = ((np.arange(B) * 7 + episode) % 3).astype(np.int32)
        for e in (r.eng, tw.eng):
            e.days_set(assign)
            e.reset()
        lo, hi, comp = r.eng.track_window()
        assert (comp[assign == 0] == 1).all() and (hi[assign == 0] < lc.RING).all() and (comp[assign == 2] == 0).all()
        seen = ring_against_resident(r, tw, "day library, episode %d" % episode)
        assert seen["steps"] > 100 and 2 in seen["terminal"], seen
    tw.close()
    r.close()


# ---- 7. the torch face -----------------------------------------------------------------------------------------------------------------------

def test_vec_env_ring_lookahead_through_torch():
    """tests/look_ring_torch_child.py, in a process of its own: torch must be imported before the engine library is loaded."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tests", "look_ring_torch_child.py")], cwd=root, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "look_ring_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "look ring OK" in res.stdout
