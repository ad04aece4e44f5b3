"""lob_snapshot_save / lob_snapshot_restore / lob_snapshot_free: the books' environment state kept and put back on the device, by mask.

The yardstick is the oracle (tests/oracle_lib.py), never a second engine.  Under private theta Oracle.env_step(actions) is
deterministic per book and independent across books, so the expected continuation of a book restored to step s is a SHADOW oracle: a
fresh Oracle on the same records, reset() and replayed with the first s action arrays the engine saw.  After a restore the engine,
the main oracle and the shadow step with the same new action arrays; the books of the mask are compared with the shadow, the others
with the main oracle (tests/test_gpu_vec_env.py check_step, `books=`), every element of every book for equality.  Actions are random
in [0, 9) from a seeded generator.  (The device counters of lob_get_counters are cumulative and are not wound back: check_step is
always given a mask here, which leaves them out.)

Shapes: B in {1, 3, 65, 300} -- lanes past B, a partial last block, rows whose tail is shorter than 16 bytes -- and one case of 5 000
books at depth 10, above the 4 096 books up to which the continuation runs through the 16-lane env kernel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from rl_markets_amd.engine import LobError
from tests import oracle_lib as ol
from tests.parity import dumps_to_np
from tests.test_gpu_days import make_days
from tests.test_gpu_vec_book import DevBook
from tests.test_gpu_vec_env import DevArray, DevVec, check_observation, check_step, gen, make_params
from tests.test_gpu_vec_history import DevHist

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 65, 300)
N_EVENTS = 160


class Run:
    """One engine, its main oracle, the device buffers and the action arrays the engine has seen (what a shadow replays)."""

    def __init__(self, B, ending="dry", depth=5, seed=0, p=None, n_events=N_EVENTS, mem=1 << 16, reset=True, rec=None):
        self.p = p if p is not None else make_params(depth, 2, mem)
        self.B, self.V, self.D = B, self.p.n_vars, self.p.depth
        # (`rec`: the caller's records [B][n][W] in place of the generator's stream)
        self.rec = rec if rec is not None else engine.gen_stream_host(gen(n_events, ending, self.p), self.p.depth, self.p.max_trades, 0, B)
        self.eng = engine.Engine(self.p, B)
        self.eng.load_events(self.rec)
        self.orc = self.new_oracle()
        self.dev = DevVec(B, self.V)
        self.mask_dev = DevArray(B, np.uint8)
        self.rng = np.random.default_rng(1000 * B + seed)
        self.hist, self.extra = [], []
        if reset:
            self.reset()

    def new_oracle(self):
        return ol.Oracle(self.p, self.rec)

    def reset(self):
        self.eng.reset()
        self.orc.reset()
        self.hist = []

    def shadow(self, s):
        """A fresh oracle replayed to step s of this episode."""
        o = self.new_oracle()
        o.reset()
        for a in self.hist[:s]:
            o.env_step(a)
        self.extra.append(o)
        return o

    def step(self, n=1, also=(), main=True):
        """n steps of random actions on the engine, the main oracle (`main`) and the oracles of `also`; -> the outputs of the last one."""
        for _ in range(n):
            a = self.rng.integers(0, abi.LOB_N_ACTIONS, size=self.B).astype(np.int32)
            self.dev.step(self.eng, a)
            if main:
                self.orc.env_step(a)
            for o in also:
                o.env_step(a)
            self.hist.append(a)
        return self.dev.read(self.eng)

    def mask(self, m):
        """The device address of the mask bytes `m` (None: NULL, every book)."""
        if m is None:
            return None
        self.mask_dev.upload(np.asarray(m).astype(np.uint8))
        return self.mask_dev.ptr

    def save(self, slot=0, m=None):
        self.eng.snapshot_save(slot, self.mask(m))

    def restore(self, slot=0, m=None):
        self.eng.snapshot_restore(slot, self.mask(m))

    def observe(self):
        self.eng.vec_observe(self.dev.out)
        return self.dev.read(self.eng)

    def check(self, got, parts, tag):
        """parts: (oracle, mask of the books that follow it) pairs that cover every book once."""
        cover = np.zeros(self.B, int)
        for o, m in parts:
            cover += m
            check_step(self.eng, o, got, self.V, 0, tag, books=m)
        assert (cover == 1).all(), "the masks part the books"

    def run_on(self, parts, n, tag, every=1, to_the_end=False):
        """n more steps (to_the_end: until n_live == 0), every `every`-th and the last one checked against `parts`."""
        oracles = [o for o, _ in parts if o is not self.orc]
        main = len(oracles) < len(parts)   # (a main oracle that no book follows any more is left where it is)
        steps = 0
        while True:
            got = self.step(1, also=oracles, main=main)
            steps += 1
            last = int(got["n_live"][0]) == 0 if to_the_end else steps == n
            if steps % every == 0 or last:
                self.check(got, parts, "%s step +%d" % (tag, steps))
            if last:
                return steps
            assert steps < 4 * N_EVENTS + 400, tag + ": the episode did not end"

    def getters(self):
        """lob_get_books, lob_get_state, lob_get_reward, lob_get_terminal as bytes."""
        return {"books": bytes(self.eng.get_books()), "state": self.eng.get_state().tobytes(), "reward": self.eng.get_reward().tobytes(),
                "terminal": self.eng.get_terminal().tobytes()}

    def close(self):
        self.dev.free()
        self.mask_dev.free()
        self.eng.close()
        self.orc.close()
        for o in self.extra:
            o.close()


def all_books(B):
    return np.ones(B, bool)


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], "%s: %s differs" % (tag, k)


class Captures:
    """The seven views of case 1: the four getters, a lob_vec_observe, a lob_vec_book and a lob_vec_history(K = 8), as bytes."""

    def __init__(self, run, K=8):
        self.run, self.K = run, K
        self.book = DevBook(run.B, run.D)
        self.hist = DevHist(run.B, K, run.D, run.p.max_trades)

    def take(self):
        r = self.run
        got = r.getters()
        for k, v in r.observe().items():
            got["observe." + k] = v.tobytes()
        r.eng.vec_book(self.book.out)
        for k, v in self.book.read(r.eng).items():
            got["book." + k] = v.tobytes()
        r.eng.vec_history(self.K, self.hist.out)
        for k, v in self.hist.read(r.eng).items():
            got["history." + k] = v.tobytes()
        return got

    def free(self):
        self.book.free()
        self.hist.free()


# ---- 1. rewind all ----------------------------------------------------------------------------------------------------------------

def rewind_all(B, ending, depth=5, every=1, mem=1 << 16):
    r = Run(B, ending, depth, mem=mem)
    cap = Captures(r)
    r.step(7)
    r.save(0)
    before = cap.take()
    r.step(18)
    assert cap.take() != before, "the books moved"
    r.restore(0)
    assert_same(cap.take(), before, "after restore(0, NULL)")
    sh = r.shadow(7)
    r.check(r.observe() | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, [(sh, all_books(B))], "restored")
    steps = r.run_on([(sh, all_books(B))], 0, "B=%d %s rewound" % (B, ending), every=every, to_the_end=True)
    term = sh.recs()["book"]["terminal"]
    assert steps > 10 and ((term == 2).all() if ending == "dry" else (term == 1).all()), (steps, term)
    cap.free()
    r.close()


@pytest.mark.parametrize("ending", ["dry", "session"])
@pytest.mark.parametrize("B", SIZES)
def test_rewind_all(B, ending):
    rewind_all(B, ending)


def test_rewind_all_above_the_16_lane_env_kernel():
    """5 000 books at depth 10 (above env16_max = 4 096: the continuation runs through the 64-lane env kernel), every 4th step and
    the last one checked.  (A small weight vector: the private weights of 5 000 books are not what this test is about.)"""
    rewind_all(5000, "dry", depth=10, every=4, mem=1 << 12)


# ---- 2. masked restore ------------------------------------------------------------------------------------------------------------

def masks_of(B, rng):
    half = rng.integers(0, 2, size=B).astype(np.uint8)
    first64 = (np.arange(B) < 64).astype(np.uint8)
    odd_values = np.where(rng.integers(0, 2, size=B) == 1, rng.integers(2, 256, size=B), 0).astype(np.uint8)
    only = lambda b: (np.arange(B) == b).astype(np.uint8)   # noqa: E731
    return {"half": half, "none": np.zeros(B, np.uint8), "book0": only(0), "last": only(B - 1), "first64": first64, "odd_values": odd_values}


@pytest.mark.parametrize("which", ["half", "none", "book0", "last", "first64", "odd_values"])
@pytest.mark.parametrize("B", SIZES)
def test_masked_restore(B, which):
    r = Run(B, "dry", seed=1)
    m8 = masks_of(B, np.random.default_rng(B))[which]
    m = m8 != 0
    r.step(7)
    r.save(0)
    r.step(18)
    sz = C.sizeof(abi.BookDump)
    before = r.getters()
    r.restore(0, m8)
    after = r.getters()
    for b in np.flatnonzero(~m):
        assert before["books"][b * sz:(b + 1) * sz] == after["books"][b * sz:(b + 1) * sz], "book %d is outside the mask and changed" % b
    if which == "none":
        assert_same(after, before, "an all-zero mask changes nothing")
    sh = r.shadow(7)
    parts = [(sh, m), (r.orc, ~m)]
    r.check(r.observe() | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, parts, "restored")
    r.run_on(parts, 0, "B=%d mask %s" % (B, which), to_the_end=True)
    r.close()


# ---- 3. / 4. restarts from the snapshot taken right after lob_reset ------------------------------------------------------------------

@pytest.mark.parametrize("ending", ["dry", "session"])
@pytest.mark.parametrize("B", SIZES)
def test_restart_recipe(B, ending):
    r = Run(B, ending, seed=2)
    r.save(0)
    r.run_on([(r.orc, all_books(B))], 0, "first run", every=8, to_the_end=True)
    term = r.eng.get_terminal()
    assert (term != 0).all()
    if ending == "dry":
        assert (term == 2).any(), "a condition on the seed: a book ran out of data"
    else:
        assert (term == 1).any(), "a condition on the seed: a book reached the end of the session"
    r.restore(0, term != 0)
    got = r.observe()
    assert int(got["n_live"][0]) == B and (got["terminal"] == 0).all(), "every book is live again"
    fresh = r.shadow(0)
    r.check(got | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, [(fresh, all_books(B))], "restarted")
    steps = r.run_on([(fresh, all_books(B))], 0, "B=%d %s second run" % (B, ending), to_the_end=True)
    assert steps > 10
    r.close()


@pytest.mark.parametrize("B", [65, 300])
def test_partial_restart(B):
    r = Run(B, "dry", seed=3)
    r.save(0)
    while True:
        got = r.step(1)
        over = got["terminal"] != 0
        if 2 * int(over.sum()) >= B:
            break
    assert 0 < int(over.sum()) < B, "about half the books are over: %d of %d" % (int(over.sum()), B)
    r.check(got, [(r.orc, all_books(B))], "before the restart")
    r.restore(0, over)
    fresh = r.shadow(0)
    parts = [(fresh, over), (r.orc, ~over)]
    got = r.observe()
    assert int(got["n_live"][0]) == B
    r.check(got | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, parts, "restarted")
    r.run_on(parts, 0, "B=%d partial restart" % B, to_the_end=True)
    r.close()


# ---- 5. the rolling means of the agent's own PnL ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", SIZES)
def test_pnl_windows(B):
    p = make_params(5, 2)
    p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, 3
    r = Run(B, "dry", seed=4, p=p, n_events=300)
    r.step(9)
    r.save(0)
    got = r.step(11)
    assert (got["stepped"] != 0).any(), "the books step: the windows of three steps are full and have wrapped"
    m = np.random.default_rng(B + 5).integers(0, 2, size=B).astype(bool)
    r.restore(0, m)
    sh = r.shadow(9)
    parts = [(sh, m), (r.orc, ~m)]
    r.check(r.observe() | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, parts, "restored")
    r.run_on(parts, 20, "B=%d normed reward" % B)
    r.close()


# ---- 6. two slots and a masked save -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", SIZES)
def test_two_slots_and_a_masked_save(B):
    r = Run(B, "dry", seed=5)
    m = np.random.default_rng(B + 6).integers(0, 2, size=B).astype(bool)
    r.step(2)
    r.save(0)
    r.step(3)
    r.save(1)
    r.step(6)
    r.save(1, m)
    r.step(5)
    r.restore(1)
    s11, s5 = r.shadow(11), r.shadow(5)
    parts = [(s11, m), (s5, ~m)]
    r.check(r.observe() | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, parts, "slot 1")
    r.run_on(parts, 6, "B=%d slot 1" % B)
    r.restore(0)
    s2 = r.shadow(2)
    r.check(r.observe() | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, [(s2, all_books(B))], "slot 0")
    r.run_on([(s2, all_books(B))], 6, "B=%d slot 0" % B)
    r.close()


# ---- 7. day library, resident track -----------------------------------------------------------------------------------------------

def test_day_library():
    B, lengths = 65, (100, 150, 200)
    p = make_params(5, 2)
    days = make_days(lengths, depth=5)
    lib = ol.DayLibrary(days)
    assign = ((np.arange(B) * 7) % 3).astype(np.int32)
    r = Run(B, "dry", seed=7, p=p, reset=False)
    r.eng.load_days(days)
    r.eng.days_set(assign)

    def oracle_on_days():
        o = ol.Oracle(p, np.stack([days[0]] * B))   # (never played: the days come by set_days)
        o.set_days(*lib.of(assign))
        return o
    r.new_oracle = oracle_on_days
    r.orc.close()
    r.orc = oracle_on_days()
    r.reset()
    np.testing.assert_array_equal(r.eng.days(), assign)
    r.step(6)
    r.save(0)
    r.step(9)
    m = np.random.default_rng(8).integers(0, 2, size=B).astype(bool)
    r.restore(0, m)
    np.testing.assert_array_equal(r.eng.days(), assign, err_msg="the days stay")
    sh = r.shadow(6)
    parts = [(sh, m), (r.orc, ~m)]
    r.check(r.observe() | {"stepped": np.zeros(B, np.int32), "reward": np.zeros(B)}, parts, "restored")
    steps = r.run_on(parts, 0, "day library", to_the_end=True)
    assert steps > 10
    r.close()


# ---- 8. stream order --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [65, 300])
def test_stream_order(B):
    """save, 3 x lob_vec_step, restore, lob_vec_step enqueued back to back: no lob_sync and no getter in between (the four action
    arrays are in device buffers of their own before the first call; the slot's buffer exists already, so no call allocates)."""
    r = Run(B, "dry", seed=8)
    r.save(0)   # (the slot's one allocation, which synchronises, happens here)
    r.step(4)
    acts = [r.rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32) for _ in range(4)]
    bufs = [DevArray(B, np.int32) for _ in acts]
    for buf, a in zip(bufs, acts):
        buf.upload(a)
    m = np.random.default_rng(B + 9).integers(0, 2, size=B).astype(bool)
    mp = r.mask(m)
    r.eng.sync()
    r.eng.snapshot_save(0, None)
    for buf in bufs[:3]:
        r.eng.vec_step(buf.ptr, r.dev.out)
    r.eng.snapshot_restore(0, mp)
    r.eng.vec_step(bufs[3].ptr, r.dev.out)
    got = r.dev.read(r.eng)
    sh = r.shadow(4)
    sh.env_step(acts[3])
    for a in acts:
        r.orc.env_step(a)
    r.check(got, [(sh, m), (r.orc, ~m)], "back to back")
    for buf in bufs:
        buf.free()
    r.close()


# ---- 9. idempotence ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", SIZES)
def test_idempotence(B):
    r = Run(B, "dry", seed=9)
    cap = Captures(r)
    r.step(6)
    now = cap.take()
    r.save(0)
    r.restore(0)
    assert_same(cap.take(), now, "save then restore at once")
    m = np.random.default_rng(B + 10).integers(0, 2, size=B).astype(bool)
    r.step(5)
    r.restore(0, m)
    once = cap.take()
    r.restore(0, m)
    assert_same(cap.take(), once, "restore twice")
    r.restore(0)
    assert_same(cap.take(), now, "restore(NULL) after a masked one")
    cap.free()
    r.close()


# ---- 10. errors -------------------------------------------------------------------------------------------------------------------

def refused(code, fn, *args):
    with pytest.raises(LobError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


def test_errors():
    B = 65
    r = Run(B, "dry", seed=10, reset=False)
    eng = r.eng
    refused(abi.LOB_ESTATE, eng.snapshot_save, 0)   # before the first lob_reset
    refused(abi.LOB_ESTATE, eng.snapshot_restore, 0)
    eng.snapshot_free(0)                            # free of an empty slot is LOB_OK
    r.reset()
    r.step(3)
    books = bytes(eng.get_books())

    def unchanged(tag):
        assert bytes(eng.get_books()) == books, tag + ": a refused call changed the books"
    for slot in (-1, abi.MAX_SNAPSHOTS):
        refused(abi.LOB_EINVAL, eng.snapshot_save, slot)
        refused(abi.LOB_EINVAL, eng.snapshot_restore, slot)
        refused(abi.LOB_EINVAL, eng.snapshot_free, slot)
    refused(abi.LOB_ESTATE, eng.snapshot_restore, 2)                                  # never saved
    refused(abi.LOB_ESTATE, eng.snapshot_save, 2, r.mask(np.ones(B, np.uint8)))       # masked save into an empty slot
    unchanged("slots")
    r.save(0)
    r.save(3)
    # the learner works until a restore, not after it, and again after lob_reset
    eng.td_step(1)
    eng.eval_step(1)
    books = bytes(eng.get_books())
    r.restore(0, np.zeros(B, np.uint8))
    assert "restore" in refused(abi.LOB_ESTATE, eng.td_step, 1)
    assert "restore" in refused(abi.LOB_ESTATE, eng.eval_step, 1)
    assert "restore" in refused(abi.LOB_ESTATE, eng.td_step_begin)
    unchanged("learner calls after a restore")
    # a later lob_reset voids every slot; a fresh save and restore work
    eng.reset()
    eng.td_step(1)
    eng.eval_step(1)
    books = bytes(eng.get_books())
    refused(abi.LOB_ESTATE, eng.snapshot_restore, 0)
    refused(abi.LOB_ESTATE, eng.snapshot_restore, 3)
    refused(abi.LOB_ESTATE, eng.snapshot_save, 0, r.mask(np.ones(B, np.uint8)))
    unchanged("after a later lob_reset")
    # between the halves of a split step
    if eng.td_split_supported():
        eng.td_step_begin()
        refused(abi.LOB_ESTATE, eng.snapshot_save, 0)
        refused(abi.LOB_ESTATE, eng.snapshot_restore, 0)
        eng.td_step_end()
        books = bytes(eng.get_books())
    r.save(0)
    eng.snapshot_restore(0)
    unchanged("a fresh save and restore")
    # lob_snapshot_free, then restore
    eng.snapshot_free(0)
    refused(abi.LOB_ESTATE, eng.snapshot_restore, 0)
    eng.snapshot_free(0)
    unchanged("free")
    # restore with the step log enabled (save still works)
    eng.step_log_enable(np.array([0, 5], np.int32), 16)
    r.save(1)
    refused(abi.LOB_ESTATE, eng.snapshot_restore, 1)
    unchanged("step log")
    eng.step_log_enable(np.zeros(0, np.int32), 0)
    eng.snapshot_restore(1)
    unchanged("step log off again")
    r.close()


def test_ring_mode_is_refused(monkeypatch):
    """A market track that is a ring (the stream is longer than the ring: tests/test_gpu_vec_env.py's switches) serves no earlier
    event count: save and restore are LOB_ESTATE alike."""
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    r = Run(64, "dry", depth=10, seed=11, n_events=1200)
    r.step(3)
    books = bytes(r.eng.get_books())
    assert "ring" in refused(abi.LOB_ESTATE, r.eng.snapshot_save, 0)
    assert "ring" in refused(abi.LOB_ESTATE, r.eng.snapshot_restore, 0)
    assert bytes(r.eng.get_books()) == books
    r.close()


# ---- the torch face -----------------------------------------------------------------------------------------------------------------

def test_vec_env_save_and_restore_through_torch():
    """tests/snapshot_torch_child.py, in a process of its own: torch must be imported before the engine library is loaded."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "snapshot_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "snapshot_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "snapshot OK" in res.stdout
