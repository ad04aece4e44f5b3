"""lob_vec_peek: what lob_vec_step would write under each of the nine actions, in one launch, with nothing of the engine changed.

Three yardsticks, every comparison for equality of every element of every book:
  * the real step: lob_snapshot_save, lob_vec_step(full(a)), download, lob_snapshot_restore, for each a (cases 1, 4, 6);
  * the oracle under the same actions, when a look-ahead stands in front of every step (case 2: it leaves nothing behind);
  * the oracle directly: a fresh Oracle replays the action prefix and then full(a) (case 3: no engine step in the yardstick).
The device buffers are plain hipMalloc memory with one guard plane in front of the nine and one behind (DevPeek); the torch face runs
in a process of its own (tests/vec_peek_torch_child.py)."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = abi.LOB_N_ACTIONS
ALL = abi.PEEK_ALL
KEYS = ("obs", "reward", "terminal", "stepped")
SLOT = 3   # the snapshot slot the real-step yardstick uses (the cases that restore on their own use slot 0)


class DevPeek:
    """The four output tensors of lob_vec_peek, each with a guard plane in front and behind (eleven planes, the call is given the
    address of the second): read() checks that both still hold the fill."""

    def __init__(self, B, V, want=KEYS):
        self.B, self.V = B, V
        self.arr = {"obs": DevArray((N + 2, B, V), np.float32), "reward": DevArray((N + 2, B), np.float64),
                    "terminal": DevArray((N + 2, B), np.uint8), "stepped": DevArray((N + 2, B), np.int32)}
        self.out = abi.VecPeekOut(*[self.arr[k].ptr + self.arr[k].host[0].nbytes if k in want else None for k in KEYS])

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

    def peek(self, eng, mask=ALL):
        eng.vec_peek(mask, self.out)
        return self.read(eng)

    def free(self):
        for v in self.arr.values():
            v.free()


def full(B, a):
    return np.full(B, a, np.int32)


def assert_plane(pk, a, got, tag):
    for k in ("obs", "terminal", "stepped"):
        np.testing.assert_array_equal(pk[k][a], got[k], err_msg="%s: %s of action %d against the step" % (tag, k, a))
    np.testing.assert_array_equal(pk["reward"][a].view(np.uint64), got["reward"].view(np.uint64), err_msg="%s: reward of action %d against the step" % (tag, a))


def new_seen():
    return {"checked": 0, "reward_differs": False, "obs_differs": False, "dry": False, "terminal_1": False, "over": False}


def peek_against_the_step(r, dp, tag, seen):
    """peek(ALL), then the nine real steps from a snapshot of this very moment; every book of every plane is compared.  Books and
    getters are where they were afterwards (what lob_snapshot_restore's own tests pin)."""
    eng, B = r.eng, r.B
    term0 = eng.get_terminal()
    pk = dp.peek(eng)
    eng.snapshot_save(SLOT, None)
    for a in range(N):
        r.dev.step(eng, full(B, a))
        got = r.dev.read(eng)
        eng.snapshot_restore(SLOT, None)
        assert_plane(pk, a, got, tag)
    live = term0 == 0
    st = pk["stepped"].astype(bool)
    assert (st == st[0]).all(), tag + ": whether a step completes does not depend on the action"
    assert not st[:, ~live].any(), tag + ": a book that was over has been stepped"
    assert (pk["reward"][~st].view(np.uint64) == 0).all(), tag + ": reward of a book that does not step is +0.0"
    np.testing.assert_array_equal(pk["terminal"][:, ~live], np.broadcast_to(term0[~live], (N, int((~live).sum()))), err_msg=tag + ": terminal of a book that was over")
    rw, ob = pk["reward"].view(np.uint64), pk["obs"].view(np.uint32)
    seen["checked"] += 1
    seen["reward_differs"] |= bool((st[0] & (rw != rw[0]).any(0)).any())
    seen["obs_differs"] |= bool((st[0] & (ob != ob[0]).any((0, 2))).any())
    seen["dry"] |= bool((live & ~st[0] & (pk["terminal"] == 2).all(0)).any())
    seen["terminal_1"] |= bool((st & (pk["terminal"] == 1)).any())
    seen["over"] |= bool((~live).any())
    return pk


def scout(orc, rng, B, cap=600):
    """The episode played by the oracle alone under random actions: -> the action arrays, and for every step whether a live book's
    episode ends in it (it runs dry, or lands in the session's last half hour)."""
    acts, ends = [], []
    t0 = orc.recs()["book"]["terminal"]
    while (t0 == 0).any():
        assert len(acts) < cap, "the episode did not end"
        a = rng.integers(0, N, size=B).astype(np.int32)
        orc.env_step(a)
        t1 = orc.recs()["book"]["terminal"]
        acts.append(a)
        ends.append(bool(((t0 == 0) & (t1 != 0)).any()))
        t0 = t1
    return acts, ends


def scouted_actions_to_the_end(r, dp, tag, k, seen):
    """The run's oracle plays the episode first (scout); the engine then takes the same actions, and the look-ahead is checked against
    the real step before every k-th step, before every step in which a book's episode ends, before each of the last three steps and
    once behind the last."""
    acts, ends = scout(r.orc, r.rng, r.B)
    for s, a in enumerate(acts):
        if s % k == 0 or ends[s] or s >= len(acts) - 3:
            peek_against_the_step(r, dp, "%s before step %d" % (tag, s + 1), seen)
        r.dev.step(r.eng, a)
    np.testing.assert_array_equal(r.eng.get_terminal(), r.orc.recs()["book"]["terminal"], err_msg=tag + ": the engine's episode ends where the oracle's does")
    peek_against_the_step(r, dp, tag + " at the end", seen)   # every book is over: nine times the books as they stand
    return len(acts)


def random_actions_to_the_end(r, dp, tag, k, seen, cap=600):
    """Without an oracle in the engine's state: random actions until no book is live; the look-ahead is checked against the real step
    before every k-th step and before every step from the first one at which a book is over (the last steps: the books end one after
    the other)."""
    steps = 0
    while True:
        n_live = int((r.eng.get_terminal() == 0).sum())
        if n_live == 0:
            break
        if steps % k == 0 or n_live < r.B:
            peek_against_the_step(r, dp, "%s before step %d" % (tag, steps + 1), seen)
        a = r.rng.integers(0, N, size=r.B).astype(np.int32)
        r.dev.step(r.eng, a)
        steps += 1
        assert steps < cap, tag + ": the episode did not end"
    peek_against_the_step(r, dp, tag + " at the end", seen)   # every book is over: nine times the books as they stand
    return steps


def assert_inputs_are_not_degenerate(seen, ending, tag):
    assert seen["reward_differs"], tag + ": a live book-step whose nine rewards are not all equal (a condition on the seed)"
    assert seen["obs_differs"], tag + ": a live book-step whose nine obs rows are not all equal (a condition on the seed)"
    if ending == "dry":
        assert seen["dry"], tag + ": a step that runs dry (a condition on the seed)"
    else:
        assert seen["terminal_1"], tag + ": a step that ends in the session's last half hour (a condition on the seed)"


# ---- 1. against the real step -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,depth,trades,ending", [(1, 5, 2, "dry"), (1, 10, 3, "session"), (63, 10, 2, "session"), (63, 5, 3, "dry"),
                                                   (65, 5, 2, "session"), (65, 10, 3, "dry"), (300, 10, 2, "dry"), (300, 5, 3, "session"),
                                                   (300, 5, 2, "session"), (65, 10, 2, "dry")])
def test_against_the_real_step(B, depth, trades, ending):
    r = Run(B, ending, seed=20, p=make_params(depth, trades))
    dp = DevPeek(B, r.V)
    seen = new_seen()
    tag = "B=%d D=%d T=%d %s" % (B, depth, trades, ending)
    steps = scouted_actions_to_the_end(r, dp, tag, 5, seen)
    term = r.eng.get_terminal()
    assert steps > 10 and ((term == 2).all() if ending == "dry" else (term == 1).all()), (steps, term)
    assert_inputs_are_not_degenerate(seen, ending, tag)
    assert seen["checked"] > steps // 5 and seen["over"]
    dp.free()
    r.close()


def test_above_the_16_lane_env_kernel():
    """5 000 books at depth 10 (above the 4 096 up to which lob_vec_step runs the 16-lane env kernel: the yardstick's steps go through
    the 64-lane one), 79 blocks per plane with a partial last one.  (A small weight vector: the private weights of 5 000 books are not
    what this test is about.)"""
    B = 5000
    r = Run(B, "dry", depth=10, seed=21, mem=1 << 12)
    dp = DevPeek(B, r.V)
    seen = new_seen()
    for step in range(31):
        if step % 10 == 0:
            peek_against_the_step(r, dp, "B=5000 before step %d" % (step + 1), seen)
        r.dev.step(r.eng, r.rng.integers(0, N, size=B).astype(np.int32))
    assert seen["checked"] == 4 and seen["reward_differs"] and seen["obs_differs"]
    dp.free()
    r.close()


# ---- 2. leaves nothing behind ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normed", [False, True], ids=["pnl", "normed"])
@pytest.mark.parametrize("B", [65, 300])
def test_leaves_nothing_behind(B, normed):
    """A look-ahead in front of EVERY step: the engine stays equal to the oracle under the same actions at every step to the end,
    counters included, and the dumps right before and right after each look-ahead are the same bytes.  normed: the reward reads the
    two PnL windows, three steps long -- full and wrapped within a few steps, so a window store of the look-ahead shows at once."""
    p = make_params(5, 2)
    if normed:
        p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, 3
    r = Run(B, "dry", seed=22, p=p)
    dp = DevPeek(B, r.V)
    steps = 0
    nonzero_reward = False
    while True:
        before_dump = bytes(r.eng.get_books())
        before = {"state": r.eng.get_state().tobytes(), "reward": r.eng.get_reward().tobytes(), "counters": tuple(r.eng.counters())}
        pk = dp.peek(r.eng)
        assert bytes(r.eng.get_books()) == before_dump, "step %d: the look-ahead changed the books" % steps
        after = {"state": r.eng.get_state().tobytes(), "reward": r.eng.get_reward().tobytes(), "counters": tuple(r.eng.counters())}
        assert after == before, "step %d: the look-ahead changed lob_get_state / lob_get_reward / the counters" % steps
        steps_before = r.orc.counters()[0]
        got = r.step(1)
        steps += 1
        check_step(r.eng, r.orc, got, r.V, steps_before, "B=%d step %d behind a look-ahead" % (B, steps))
        a = r.hist[-1]
        for k in ("obs", "terminal", "stepped"):   # (and the plane of the action each book was then given is what the step gave it)
            np.testing.assert_array_equal(pk[k][a, np.arange(B)], got[k], err_msg="step %d: %s" % (steps, k))
        np.testing.assert_array_equal(pk["reward"][a, np.arange(B)].view(np.uint64), got["reward"].view(np.uint64), err_msg="step %d: reward" % steps)
        nonzero_reward |= bool((got["reward"] != 0.0).any())
        if int(got["n_live"][0]) == 0:
            break
        assert steps < 600
    assert steps > 20 and nonzero_reward, "the windows filled and the reward moved"
    dp.free()
    r.close()


# ---- 3. against the oracle directly ---------------------------------------------------------------------------------------------------

def test_against_the_oracle_directly():
    """B = 65; the scout picks at most twelve steps: eight spread over the episode, and the first four in which a book runs dry."""
    B = 65
    r = Run(B, "dry", seed=23)
    dp = DevPeek(B, r.V)
    sc = r.new_oracle()
    sc.reset()
    acts, ends = scout(sc, r.rng, B)
    sc.close()
    chosen = set(list(range(3, len(acts), max(1, len(acts) // 8)))[:8]) | set([s for s, e in enumerate(ends) if e][:4])
    assert 8 <= len(chosen) <= 12 and any(ends[s] for s in chosen), (sorted(chosen), len(acts))
    seen_stepped = seen_dry = False
    for s, act in enumerate(acts):
        if s in chosen:
            term0 = r.orc.recs()["book"]["terminal"]
            pk = dp.peek(r.eng)
            for a in range(N):
                o = r.new_oracle()
                o.reset()
                for h in acts[:s]:
                    o.env_step(h)
                n0 = o.counters()[0]
                o.env_step(full(B, a))
                recs = o.recs()
                st = (term0 == 0) & (recs["book"]["terminal"] != 2)   # (a step that runs dry is the one way a live book does not step)
                assert int(st.sum()) == int(o.counters()[0] - n0), "the oracle's step counter"
                tag = "before step %d, action %d" % (s + 1, a)
                np.testing.assert_array_equal(pk["stepped"][a], st.astype(np.int32), err_msg=tag + ": stepped")
                np.testing.assert_array_equal(pk["obs"][a], recs["vars"][:, :r.V], err_msg=tag + ": obs")
                np.testing.assert_array_equal(pk["terminal"][a], recs["book"]["terminal"], err_msg=tag + ": terminal")
                np.testing.assert_array_equal(pk["reward"][a][st], recs["reward"][st], err_msg=tag + ": reward of the books that stepped")
                assert (pk["reward"][a][~st].view(np.uint64) == 0).all(), tag
                seen_stepped |= bool(st.any())
                seen_dry |= bool(((term0 == 0) & ~st).any())
                o.close()
        r.dev.step(r.eng, act)
        r.orc.env_step(act)
    assert seen_stepped and seen_dry
    dp.free()
    r.close()


# ---- 4. every reward measure ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("measure", sorted(abi.REWARD_NAMES, key=abi.REWARD_NAMES.get))
def test_every_reward_measure(measure):
    B = 65
    p = make_params(5, 2)
    p.reward_measure = abi.REWARD_NAMES[measure]
    if p.reward_measure == abi.REWARD_NORMED:
        p.lb_pnl = 3
    r = Run(B, "dry", seed=24, p=p)
    dp = DevPeek(B, r.V)
    seen = new_seen()
    steps = scouted_actions_to_the_end(r, dp, "measure " + measure, 7, seen)
    assert steps > 10 and seen["obs_differs"] and seen["dry"]
    if p.reward_measure != abi.REWARD_NONE:
        assert seen["reward_differs"], measure + ": the nine rewards of some live book differ"
    dp.free()
    r.close()


# ---- 5. the mask, NULL members, the neighbours of the buffers ------------------------------------------------------------------------------

def test_mask_and_null_members():
    B = 65
    r = Run(B, "dry", seed=25)
    r.step(9)
    dp = DevPeek(B, r.V)
    ref = dp.peek(r.eng)
    assert all((v.view(np.uint8) != 0xAB).any() for v in ref.values())
    for mask in [1 << a for a in range(N)] + [0x101, 0x0AA]:
        dp.fill()
        got = dp.peek(r.eng, mask)
        for a in range(N):
            for k in KEYS:
                if mask >> a & 1:
                    np.testing.assert_array_equal(got[k][a].view(np.uint8), ref[k][a].view(np.uint8), err_msg="mask %#x plane %d %s" % (mask, a, k))
                else:
                    assert (got[k][a].view(np.uint8) == 0xAB).all(), "mask %#x: plane %d of %s was written" % (mask, a, k)
    for want in (("obs",), ("reward", "stepped"), ("terminal",), ("obs", "reward", "terminal")):
        part = DevPeek(B, r.V, want=want)
        got = part.peek(r.eng)
        for k in KEYS:
            if k in want:
                np.testing.assert_array_equal(got[k].view(np.uint8), ref[k].view(np.uint8), err_msg="members %s: %s" % (want, k))
            else:
                assert (got[k].view(np.uint8) == 0xAB).all(), "members %s: %s is NULL and was written" % (want, k)
        part.free()
    none = abi.VecPeekOut(None, None, None, None)
    r.eng.vec_peek(ALL, none)   # nothing wanted: LOB_OK
    dp.free()
    r.close()


# ---- 6. after a masked restore; on a day library ------------------------------------------------------------------------------------------

def test_after_a_masked_restore():
    B = 65
    r = Run(B, "dry", seed=26)
    dp = DevPeek(B, r.V)
    r.step(7)
    r.save(0)
    r.step(12)
    m = np.random.default_rng(27).integers(0, 2, size=B).astype(bool)
    assert m.any() and not m.all()
    r.restore(0, m)
    seen = new_seen()
    steps = random_actions_to_the_end(r, dp, "after a masked restore", 4, seen)
    assert steps > 10
    assert_inputs_are_not_degenerate(seen, "dry", "after a masked restore")
    dp.free()
    r.close()


def test_day_library_with_days_of_unequal_length():
    B, lengths = 65, (100, 150, 200)
    p = make_params(5, 2)
    days = make_days(lengths, depth=5)
    assign = ((np.arange(B) * 7) % 3).astype(np.int32)
    r = Run(B, "dry", seed=28, p=p, reset=False)
    r.eng.load_days(days)
    r.eng.days_set(assign)
    r.eng.reset()
    np.testing.assert_array_equal(r.eng.days(), assign)
    dp = DevPeek(B, r.V)
    seen = new_seen()
    steps = random_actions_to_the_end(r, dp, "day library", 6, seen)
    assert steps > 10 and (r.eng.get_terminal() == 2).all()
    assert_inputs_are_not_degenerate(seen, "dry", "day library")
    dp.free()
    r.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def refused(code, fn, *args):
    with pytest.raises(LobError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert b"lob_vec_peek" in abi.load().lob_last_error()
    return str(ei.value)


def steps_on_equal_to_the_oracle(r, n, tag):
    for i in range(n):
        before = r.orc.counters()[0]
        got = r.step(1)
        check_step(r.eng, r.orc, got, r.V, before, "%s, step %d" % (tag, i + 1))


def test_refusals():
    B = 65
    r = Run(B, "dry", seed=29, reset=False)
    eng, lib = r.eng, abi.load()
    dp = DevPeek(B, r.V)
    refused(abi.LOB_ESTATE, eng.vec_peek, ALL, dp.out)   # before the first lob_reset
    r.reset()
    r.step(3)
    books = bytes(eng.get_books())
    assert lib.lob_vec_peek(eng.h, ALL, None) == abi.LOB_EINVAL and b"lob_vec_peek" in lib.lob_last_error()
    assert lib.lob_vec_peek(None, ALL, C.byref(dp.out)) == abi.LOB_EINVAL and b"lob_vec_peek" in lib.lob_last_error()
    for mask in (0, 0x200, 0x3FF, 1 << 31):
        refused(abi.LOB_EINVAL, eng.vec_peek, mask, dp.out)
    if eng.td_split_supported():
        eng.td_step_begin()
        refused(abi.LOB_ESTATE, eng.vec_peek, ALL, dp.out)
        eng.td_step_end()
        r.orc.td_step(1)
        books = bytes(eng.get_books())
    eng.sync()
    assert bytes(eng.get_books()) == books, "a refused call changed the books"
    assert all((v.view(np.uint8) == 0xAB).all() for v in dp.read(eng).values()), "a refused call wrote"
    steps_on_equal_to_the_oracle(r, 5, "after the refusals")
    dp.free()
    r.close()


def test_ring_mode_is_refused(monkeypatch):
    """A market track that is a ring (tests/test_gpu_snapshot.py's switches): LOB_ESTATE, and the engine steps on."""
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    r = Run(64, "dry", depth=10, seed=30, n_events=1200)
    dp = DevPeek(64, r.V)
    r.step(3)
    books = bytes(r.eng.get_books())
    assert "ring" in refused(abi.LOB_ESTATE, r.eng.vec_peek, ALL, dp.out)
    assert bytes(r.eng.get_books()) == books
    steps_on_equal_to_the_oracle(r, 20, "ring mode, after the refusal")
    dp.free()
    r.close()


# ---- 8. the torch face ---------------------------------------------------------------------------------------------------------------------

def test_vec_env_peek_through_torch():
    """tests/vec_peek_torch_child.py, in a process of its own: torch must be imported before the engine library is loaded."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vec_peek_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "vec_peek_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "peek OK" in res.stdout
