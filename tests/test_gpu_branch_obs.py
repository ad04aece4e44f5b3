"""lob_branch_book / lob_branch_history: the order book, the agent's own words and the window of the last K event records of every
branch of the live set, written to device memory branch-major.

ONE rule is checked: element [n][b] is, bit for bit, what lob_vec_book / lob_vec_history(K) would write at [b] had the engine's books
been in branch n's state.  Yardsticks, every comparison for equality of every element (f32 as uint32 views: NaNs occur, and both sides
do the same arithmetic; no tolerance anywhere):
  * behind a fork: lob_vec_book / lob_vec_history of the real books at that moment, in every plane;
  * the real steps from a snapshot, with no branch code in it: lob_snapshot_save, per branch h x (lob_vec_step with the plan's actions,
    lob_vec_book, lob_vec_history, download), lob_snapshot_restore;
  * for lob_branch_select: numpy's gather of the tensors read just before it, and the real steps along each branch's ancestry.
Every output tensor has one guard plane in front and one behind (0xAB, checked after every call) and 64 guard bytes around the whole.
The torch face runs in a process of its own (tests/branch_obs_torch_child.py); the CPU check that the scripted seeds reach what case 2
asserts is tests/test_branch_obs_seeds.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi
from rl_markets_amd.engine import LobError
from tests.branch_obs_cases import H, PRE, SEED, SHAPES, holey, random_actions, reached, script
from tests.test_gpu_days import make_days
from tests.test_gpu_snapshot import DevBook, DevHist, Run
from tests.test_gpu_vec_branch import DevBranch
from tests.test_gpu_vec_env import hip, make_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOK = ("levels", "own", "time_ms")
HIST = ("levels", "trades", "time_ms", "n_valid", "rec")
ALL = tuple("book." + k for k in BOOK) + tuple("hist." + k for k in HIST)
SLOT = 3     # the snapshot slot the real-step yardstick uses
FENCE = 64   # guard bytes in front of and behind every buffer
H2D, D2H = 1, 2


class Planes:
    """N + 2 planes of hipMalloc memory behind a fence: the calls are given the address of the second plane, which lies `offset` bytes
    behind a 16-byte boundary whatever a plane's size (a plane's first byte is 16-byte aligned only if the caller's pointer is);
    read() checks the fences and both guard planes."""

    def __init__(self, N, shape, dtype, offset=0):
        self.shape, self.dtype = (N + 2,) + tuple(shape), np.dtype(dtype)
        self.plane = int(np.prod(shape)) * self.dtype.itemsize
        self.offset = FENCE + (-self.plane) % 16 + offset
        self.nbytes = (N + 2) * self.plane
        self.total = self.offset + self.nbytes + FENCE
        p = C.c_void_p()
        assert hip().hipMalloc(C.byref(p), self.total) == 0
        self.base = p.value
        self.ptr = self.base + self.offset + self.plane
        assert self.base % 16 == 0 and self.ptr % 16 == offset
        self.fill()

    def fill(self):
        assert hip().hipMemset(self.base, 0xAB, self.total) == 0

    def read(self, name):
        raw = np.zeros(self.total, np.uint8)
        assert hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), self.base, self.total, D2H) == 0
        body = raw[self.offset:self.offset + self.nbytes]
        assert (raw[:self.offset] == 0xAB).all() and (raw[self.offset + self.nbytes:] == 0xAB).all(), name + ": bytes outside the buffer were written"
        assert (body[:self.plane] == 0xAB).all() and (body[-self.plane:] == 0xAB).all(), name + ": a guard plane was written"
        return body.view(self.dtype).reshape(self.shape)[1:-1].copy()

    def free(self):
        if self.base:
            hip().hipFree(self.base)
            self.base = None


class DevObs:
    """The eight output tensors of the two calls for one (N, K); `want`: the members that are not NULL; `offset`: bytes by which every
    pointer is moved off its 16-byte boundary (book.time_ms is int64: it stays aligned to its element)."""

    def __init__(self, B, D, T, N, K, want=ALL, offset=0):
        self.N, self.K, self.want = N, K, tuple(want)
        f32, i32 = np.float32, np.int32
        spec = {"book.levels": ((B, 4, D), f32), "book.own": ((B, abi.VEC_OWN_WORDS), f32), "book.time_ms": ((B,), np.int64),
                "hist.levels": ((B, K, 4, D), f32), "hist.trades": ((B, K, 2, T), f32), "hist.time_ms": ((B, K), i32),
                "hist.n_valid": ((B,), i32), "hist.rec": ((B,), i32)}
        self.buf = {k: Planes(N, s, dt, 0 if k == "book.time_ms" else offset) for k, (s, dt) in spec.items()}
        ptr = lambda k: self.buf[k].ptr if k in self.want else None
        self.book_out = abi.VecBookOut(*[ptr("book." + k) for k in BOOK])
        self.hist_out = abi.VecHistOut(*[ptr("hist." + k) for k in HIST])

    def fill(self):
        for v in self.buf.values():
            v.fill()

    def read(self, eng):
        eng.sync()
        return {k: v.read(k) for k, v in self.buf.items()}

    def call(self, eng):
        eng.branch_book(self.book_out)
        eng.branch_history(self.K, self.hist_out)
        return self.read(eng)

    def free(self):
        for v in self.buf.values():
            v.free()


class Real:
    """lob_vec_book and lob_vec_history(K) of the real books, under the names of DevObs."""

    def __init__(self, r, K):
        self.K = K
        self.book, self.hist = DevBook(r.B, r.D), DevHist(r.B, K, r.D, r.p.max_trades)

    def take(self, eng):
        eng.vec_book(self.book.out)
        eng.vec_history(self.K, self.hist.out)
        got = {"book." + k: v for k, v in self.book.read(eng).items()}
        got.update({"hist." + k: v for k, v in self.hist.read(eng).items()})
        return got

    def free(self):
        self.book.free()
        self.hist.free()


def bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, ref, tag, keys=ALL):
    """got [N][...] against ref [N][...] (or [...]: the same in every plane), every element."""
    for k in keys:
        want = np.broadcast_to(ref[k], got[k].shape) if ref[k].ndim < got[k].ndim else ref[k]
        np.testing.assert_array_equal(bits(got[k]), bits(want), err_msg="%s: %s" % (tag, k))


def real_steps(r, real, plans, every=1, to_the_end=False, cap=400):
    """The yardstick without a branch in it: from a snapshot of this very moment, branch after branch through lob_vec_step, the book
    and the window read behind every `every`-th step and the last.  -> ref[n][h]: the eight tensors and `terminal` (missing where
    not read); to_the_end: every branch runs until all its books are over (behind that nothing moves: its last entry holds)."""
    eng = r.eng
    N, n_steps = plans.shape[:2]
    ref = [dict() for _ in range(N)]
    eng.snapshot_save(SLOT, None)
    for n in range(N):
        for h in range(min(n_steps, cap)):
            r.dev.step(eng, plans[n, h])
            term = r.dev.read(eng)["terminal"]
            last = h == n_steps - 1 or (to_the_end and (term != 0).all())
            if h % every == every - 1 or last:
                ref[n][h] = real.take(eng)
                ref[n][h]["terminal"] = term
            if last:
                break
        assert last, "the yardstick did not reach its last step"
        eng.snapshot_restore(SLOT, None)
    eng.vec_status()   # (the real step counts the plans' holes as actions out of range: cleared)
    return ref


def stack(ref, h):
    """ref[n][h] of every branch as [N][...] (a branch that was over before step h: its last entry)."""
    rows = [rn[h] if h in rn else rn[max(rn)] for rn in ref]
    assert all(h in rn or h > max(rn) for rn in ref)
    return {k: np.stack([row[k] for row in rows]) for k in rows[0]}


def set_up(B, depth, trades, N, K, ending="dry", seed=SEED, **kw):
    r = Run(B, ending, seed=seed, p=make_params(depth, trades, **kw))
    return r, DevObs(B, depth, trades, N, K), Real(r, K), DevBranch(B, r.V, N)


def tear_down(r, *bufs):
    for b in bufs:
        b.free()
    r.close()


# ---- 1. behind a fork -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,depth,trades,N,K", SHAPES)
def test_behind_a_fork(B, depth, trades, N, K):
    r, obs, real, db = set_up(B, depth, trades, N, K)
    tag = "B=%d D=%d T=%d N=%d K=%d" % (B, depth, trades, N, K)

    def check(stage):
        ref = real.take(r.eng)
        r.eng.branch_fork(N, None)
        obs.fill()
        same(obs.call(r.eng), ref, "%s, fork %s" % (tag, stage))
        return ref

    ref = check("at reset")
    for _ in range(PRE):
        r.dev.step(r.eng, random_actions(r.rng, B))
    ref2 = check("after %d real steps" % PRE)
    assert (ref2["hist.rec"] > ref["hist.rec"]).any() and (ref2["book.own"][:, abi.OWN_TOTAL_TICKS] > 0).any()
    r.eng.clear_inventory()
    ref3 = check("after lob_clear_inventory")
    assert (ref3["book.own"][:, abi.OWN_POSITION] == 0).all()
    tear_down(r, obs, real, db)


# ---- 2. against the real steps from a snapshot ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,depth,trades,N,K", SHAPES)
def test_against_the_real_steps(B, depth, trades, N, K):
    r, obs, real, db = set_up(B, depth, trades, N, K)
    tag = "B=%d D=%d T=%d N=%d K=%d" % (B, depth, trades, N, K)
    pre, plans = script(B, N)
    for a in pre:
        r.dev.step(r.eng, a)
    ref = real_steps(r, real, plans)
    db.fork(r.eng)
    same(obs.call(r.eng), real.take(r.eng), tag + ", behind the fork")
    for h in range(H):
        step = db.step(r.eng, plans[:, h])
        want = stack(ref, h)
        np.testing.assert_array_equal(step["terminal"], want["terminal"], err_msg="%s: terminal of step %d" % (tag, h))
        same(obs.call(r.eng), want, "%s, step %d" % (tag, h))
    # the comparison was not vacuous: from the yardstick's own output (tests/test_branch_obs_seeds.py: the oracle reaches the same)
    every = [stack(ref, h) for h in range(H)]
    rec = np.stack([e["hist.rec"] for e in every], 1)
    assert reached(rec, np.stack([e["hist.n_valid"] for e in every], 1), np.stack([e["book.own"] for e in every], 1), N, K) == [], tag
    if K == 128:
        lv = every[0]["hist.levels"]
        assert (lv[:, :, 0] == 0).all((2, 3)).any() and (lv[:, :, K - 1] != 0).any(), "a slot before the stream's start is zero, the newest is not"
    tear_down(r, obs, real, db)


# ---- 3. to the end / 5. the day library -------------------------------------------------------------------------------------------------------

def to_the_end(r, obs, real, db, tag, seen, every=8, cap=400):
    """fork here, then holey plans on every branch until all are over: the yardstick's branches run to their own ends, the set is
    stepped to the longest of them; every `every`-th step and the last are compared."""
    N, B = db.N, r.B
    plans = holey(r.rng, N, cap, B, p_skip=0.1)
    ref = real_steps(r, real, plans, every=every, to_the_end=True, cap=cap)
    n_steps = max(max(rn) for rn in ref) + 1
    db.fork(r.eng)
    for h in range(n_steps):
        step = db.step(r.eng, plans[:, h])
        if h % every == every - 1 or h == n_steps - 1:
            want = stack(ref, h)
            np.testing.assert_array_equal(step["terminal"], want["terminal"], err_msg="%s: terminal of step %d" % (tag, h))
            same(obs.call(r.eng), want, "%s, step %d" % (tag, h))
            seen["terminal"] |= set(np.unique(want["terminal"]).tolist())
            seen["mixed"] |= bool(((want["terminal"] == 2).any(1) & (want["terminal"] == 0).any(1)).any())
    assert (step["terminal"] != 0).all() and n_steps > 10, (tag, n_steps)
    return n_steps


def test_to_the_end():
    B, depth, trades, N, K = 65, 5, 2, 3, 5
    seen = {"terminal": set(), "mixed": False}
    for ending in ("dry", "session"):
        r, obs, real, db = set_up(B, depth, trades, N, K, ending=ending, seed=SEED + 1)
        for _ in range(2):
            r.dev.step(r.eng, random_actions(r.rng, B))
        to_the_end(r, obs, real, db, "to the end, " + ending, seen)
        final = obs.call(r.eng)
        assert (final["hist.rec"] <= r.rec.shape[1] - 1).all(), "the window ends within the stream"
        tear_down(r, obs, real, db)
    assert {1, 2} <= seen["terminal"], "terminal 1 and the dry step among the compared branches: %r" % (seen,)


def test_day_library_with_days_of_unequal_length():
    B, depth, trades, N, K, lengths = 65, 5, 2, 3, 128, (100, 150, 200)
    r = Run(B, "dry", seed=SEED + 2, p=make_params(depth, trades), reset=False)
    days = make_days(lengths, depth=depth)
    assign = ((np.arange(B) * 7) % 3).astype(np.int32)
    r.eng.load_days(days)
    r.eng.days_set(assign)
    r.eng.reset()
    np.testing.assert_array_equal(r.eng.days(), assign)
    obs, real, db = DevObs(B, depth, trades, N, K), Real(r, K), DevBranch(B, r.V, N)
    seen = {"terminal": set(), "mixed": False}
    to_the_end(r, obs, real, db, "day library", seen, every=4)
    final = obs.call(r.eng)
    # every book ends within ITS day, neighbours on different days: the long day's books beyond the length of the short one
    assert (final["hist.rec"] <= np.asarray(lengths, np.int32)[assign] - 1).all()
    assert (final["hist.rec"][:, assign == 2] >= lengths[0]).all() and (final["hist.n_valid"][:, assign == 0] < K).all()
    assert seen["mixed"], "books of the short day dry while others of the branch are live, at a compared step"
    tear_down(r, obs, real, db)


# ---- 4. select --------------------------------------------------------------------------------------------------------------------------------

def test_select():
    B, depth, trades, N, K = 130, 5, 2, 5, 5
    r, obs, real, db = set_up(B, depth, trades, N, K, seed=SEED + 3)
    rng = r.rng
    for _ in range(PRE):
        r.dev.step(r.eng, random_actions(rng, B))
    cols = np.arange(B)[None, :]
    ident = np.arange(N, dtype=np.int32)[:, None]
    played = np.zeros((N, 0, B), np.int32)   # the actions branch (n, b) has behind it, along its ancestry
    db.fork(r.eng)

    def step():
        nonlocal played
        a = holey(rng, N, 1, B)[:, 0]
        db.step(r.eng, a)
        played = np.concatenate([played, a[:, None]], 1)
        return obs.call(r.eng)

    def select(parent, tag):
        nonlocal played
        before = obs.call(r.eng)
        eff = np.where((parent >= 0) & (parent < N), parent, ident)
        db.select(r.eng, parent)
        obs.fill()
        got = obs.call(r.eng)
        same(got, {k: v[eff, cols] for k, v in before.items()}, "select, " + tag)
        played = played[eff[:, None, :], np.arange(played.shape[1])[None, :, None], cols[:, None, :]]
        return eff

    def check_against_the_ancestry(got, tag):
        ref = real_steps(r, real, played)
        same(got, stack(ref, played.shape[1] - 1), "select, " + tag)

    for _ in range(3):
        got = step()
    assert (got["hist.rec"] != got["hist.rec"][:1]).any(), "branches that have drifted apart in front of the select"
    eff = select(rng.integers(0, N, size=(N, B)).astype(np.int32), "random per-book parents")
    assert (eff != ident).any()
    check_against_the_ancestry(step(), "a step behind random per-book parents")
    select(np.full((N, B), N - 2, np.int32), "fan-out from one parent")
    odd = rng.integers(0, N, size=(N, B)).astype(np.int32)
    out = rng.random((N, B)) < 0.5
    odd[out] = rng.choice(np.array([-1, N, N + 7, np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int32), size=int(out.sum()))
    select(odd, "out-of-range parents, a second select in a row")
    check_against_the_ancestry(step(), "a step behind two selects in a row")
    tear_down(r, obs, real, db)


# ---- 6. pointers --------------------------------------------------------------------------------------------------------------------------------

def test_null_members_alignment_and_the_launch_count():
    B, depth, trades, N, K = 65, 7, 3, 3, 5
    r, full, real, db = set_up(B, depth, trades, N, K, seed=SEED + 4)
    pre, plans = script(B, N, seed=SEED + 4)
    for a in pre:
        r.dev.step(r.eng, a)
    db.fork(r.eng)
    for h in range(3):
        db.step(r.eng, plans[:, h])
    ref = full.call(r.eng)
    assert all((v.view(np.uint8) != 0xAB).any() for v in ref.values())
    for skip in ALL:   # each member NULL in turn: skipped, its neighbours written as ever
        part = DevObs(B, depth, trades, N, K, want=[k for k in ALL if k != skip])
        got = part.call(r.eng)
        assert (got[skip].view(np.uint8) == 0xAB).all(), skip + " is NULL and was written"
        same(got, ref, "without " + skip, keys=[k for k in ALL if k != skip])
        part.free()
    none = DevObs(B, depth, trades, N, K, want=())
    r.eng.kernel_timing(True)
    full.call(r.eng)
    count = lambda: (r.eng.kernel_time_ms("branch_book_kernel")[1], r.eng.kernel_time_ms("branch_hist_kernel")[1])
    launched = count()
    assert min(launched) >= 1, launched
    assert all((v.view(np.uint8) == 0xAB).all() for v in none.call(r.eng).values())   # (call() raises unless both return LOB_OK)
    assert count() == launched, "a struct of NULL members launched a kernel"
    r.eng.kernel_timing(False)
    none.free()
    off = DevObs(B, depth, trades, N, K, offset=4)   # no pointer 16-byte aligned: a word per lane
    assert all(off.buf[k].ptr % 16 == 4 for k in ALL if k != "book.time_ms") and all(v.ptr % 16 == 0 for v in full.buf.values())
    same(off.call(r.eng), ref, "every pointer moved by 4 bytes")
    off.free()
    tear_down(r, full, real, db)


# ---- 7. nothing left behind ---------------------------------------------------------------------------------------------------------------------

def test_nothing_left_behind():
    B, depth, trades, N, K = 65, 5, 2, 3, 5
    r, obs, real, db = set_up(B, depth, trades, N, K, seed=SEED + 5)
    twin = DevBranch(B, r.V, N)
    pre, plans = script(B, N, seed=SEED + 5)
    for a in pre:
        r.dev.step(r.eng, a)

    def everything():
        got = {"books": bytes(r.eng.get_books()), "counters": r.eng.counters().tobytes(), "rng": r.eng.rng_counters().tobytes()}
        got.update({"observe." + k: v.tobytes() for k, v in r.observe().items()})
        return got

    # what the branch steps give WITHOUT the two calls among them
    db.fork(r.eng)
    plain = [db.step(r.eng, plans[:, h]) for h in range(H)]
    before = everything()
    twin.fork(r.eng)
    for h in range(H):
        for _ in range(3):
            obs.call(r.eng)
        got = twin.step(r.eng, plans[:, h])
        for k in got:
            np.testing.assert_array_equal(got[k].view(np.uint8), plain[h][k].view(np.uint8), err_msg="step %d behind a burst: %s" % (h, k))
    assert plain[-1]["stepped"].any()
    after = everything()
    for k in before:
        assert after[k] == before[k], "the calls changed " + k
    assert r.eng.vec_status() == (abi.LOB_OK, 0)
    twin.free()
    tear_down(r, obs, real, db)


# ---- 8. lifetime and refusals --------------------------------------------------------------------------------------------------------------------

def refused(code, name, fn, *args):
    with pytest.raises(LobError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert name.encode() in abi.load().lob_last_error()
    return str(ei.value)


def both_refused(eng, obs, code, tag, text=""):
    assert text in refused(code, "lob_branch_book", eng.branch_book, obs.book_out), tag
    assert text in refused(code, "lob_branch_history", eng.branch_history, obs.K, obs.hist_out), tag


def test_lifetime_and_refusals():
    B, depth, trades, N, K = 65, 5, 2, 3, 5
    r = Run(B, "dry", seed=SEED + 6, p=make_params(depth, trades), reset=False)
    eng, lib = r.eng, abi.load()
    obs, db = DevObs(B, depth, trades, N, K), DevBranch(B, r.V, N)
    db.words.upload(np.zeros((N, B), np.int32))
    both_refused(eng, obs, abi.LOB_ESTATE, "before the first lob_reset")
    r.reset()
    r.step(3)
    both_refused(eng, obs, abi.LOB_ESTATE, "before any fork", "no live branch set")
    eng.branch_fork(N, None)
    eng.branch_step(db.words.ptr, db.out)
    obs.call(eng)
    obs.fill()

    def untouched(tag):
        assert all((v.view(np.uint8) == 0xAB).all() for v in obs.read(eng).values()), tag + ": a refused call wrote"

    books = bytes(eng.get_books())
    for k in (0, -1, abi.MAX_HISTORY + 1):
        assert "K = %d" % k in refused(abi.LOB_EINVAL, "lob_branch_history", eng.branch_history, k, obs.hist_out)
    for fn, args, name in ((lib.lob_branch_book, (eng.h, None), b"lob_branch_book"), (lib.lob_branch_history, (eng.h, K, None), b"lob_branch_history"),
                           (lib.lob_branch_book, (None, C.byref(obs.book_out)), b"lob_branch_book"),
                           (lib.lob_branch_history, (None, K, C.byref(obs.hist_out)), b"lob_branch_history")):
        assert fn(*args) == abi.LOB_EINVAL and name in lib.lob_last_error(), name
    if eng.td_split_supported():
        eng.td_step_begin()
        both_refused(eng, obs, abi.LOB_ESTATE, "inside a split learner step")
        eng.td_step_end()
        r.orc.td_step(1)
        untouched("arguments, a split learner step")
        books = bytes(eng.get_books())
        assert (obs.call(eng)["hist.rec"] >= 0).all(), "the set is still live behind a learner step"
        obs.fill()
    eng.branch_close()
    both_refused(eng, obs, abi.LOB_ESTATE, "after lob_branch_close", "no live branch set")
    untouched("after lob_branch_close")
    assert bytes(eng.get_books()) == books, "a refused call changed the books"
    eng.branch_fork(N, None)
    obs.call(eng)
    obs.fill()
    r.reset()
    both_refused(eng, obs, abi.LOB_ESTATE, "after lob_reset", "no live branch set")
    untouched("after lob_reset")
    r.step(2)
    real = Real(r, K)
    eng.branch_fork(N, None)
    same(obs.call(eng), real.take(eng), "a fork behind the reset")
    tear_down(r, obs, real, db)


def test_ring_mode_is_refused(monkeypatch):
    """A market track that is a ring (tests/test_gpu_vec_branch.py's switches): no set can be forked, LOB_ESTATE."""
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    B, N, K = 64, 2, 5
    r = Run(B, "dry", depth=10, seed=SEED + 7, n_events=1200)
    obs = DevObs(B, 10, r.p.max_trades, N, K)
    r.step(3)
    books = bytes(r.eng.get_books())
    refused(abi.LOB_ESTATE, "lob_branch_fork", r.eng.branch_fork, N, None)
    both_refused(r.eng, obs, abi.LOB_ESTATE, "ring mode")
    assert bytes(r.eng.get_books()) == books
    assert all((v.view(np.uint8) == 0xAB).all() for v in obs.read(r.eng).values()), "a refused call wrote"
    tear_down(r, obs)


# ---- 9. the most branches / 10. above the 16-lane env kernel ------------------------------------------------------------------------------------

def short_run(B, depth, trades, N, K, n_steps, seed, **kw):
    r, obs, real, db = set_up(B, depth, trades, N, K, seed=seed, **kw)
    pre, plans = script(B, N, n_steps=n_steps, seed=seed)
    for a in pre:
        r.dev.step(r.eng, a)
    ref = real_steps(r, real, plans)
    db.fork(r.eng)
    for h in range(n_steps):
        db.step(r.eng, plans[:, h])
        got = obs.call(r.eng)
        same(got, stack(ref, h), "B=%d N=%d, step %d" % (B, N, h))
    assert N == 1 or (got["hist.rec"] != got["hist.rec"][:1]).any()
    tear_down(r, obs, real, db)


def test_the_most_branches():
    short_run(65, 5, 2, abi.MAX_BRANCHES, 2, 2, SEED + 8)


def test_above_the_16_lane_env_kernel():
    """5 000 books at depth 10, above the 4 096 up to which lob_vec_step runs the 16-lane env kernel (tests/test_gpu_vec_branch.py):
    79 blocks per plane with a partial last one.  (A small weight vector: the private weights are not what this test is about.)"""
    short_run(5000, 10, 2, 2, 5, 3, SEED + 9, mem=1 << 12)


# ---- 11. the torch face ----------------------------------------------------------------------------------------------------------------------------

def test_vec_env_branch_tensors_through_torch():
    """tests/branch_obs_torch_child.py, in a process of its own: torch must be imported before the engine library is loaded."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "branch_obs_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "branch_obs_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "branch obs OK" in res.stdout
