"""lob_vec_step / lob_vec_observe / lob_vec_status: the environment face with actions and observations in device memory.

The yardstick is the oracle (tests/oracle_lib.py: oracle_env_step, the runner's `while (!env.isTerminal())`) and the getters the
rest of the suite pins to it (lob_get_books, lob_get_state, lob_get_terminal) -- never a second engine.  Everything is compared
for equality.  The device buffers of these tests are plain hipMalloc memory (no torch in this process: one HIP runtime per
process, rl_markets_amd/abi.py); the torch-facing wrapper runs in a process of its own (tests/vec_env_torch_child.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from rl_markets_amd.engine import LobError
from tests import oracle_lib as ol
from tests.parity import assert_books_equal, compare_env, compare_learner_step, dumps_to_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H2D, D2H = 1, 2
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return _hip


class DevArray:
    """A device buffer with a numpy face: upload() / download() are whole-buffer hipMemcpy calls."""

    def __init__(self, shape, dtype, fill=0xAB):
        self.host = np.zeros(shape, dtype)
        p = C.c_void_p()
        assert hip().hipMalloc(C.byref(p), max(self.host.nbytes, 16)) == 0
        self.ptr = p.value
        assert hip().hipMemset(self.ptr, fill, max(self.host.nbytes, 16)) == 0   # (a value no output takes: an unwritten slot shows)

    def upload(self, a):
        a = np.ascontiguousarray(a, self.host.dtype).reshape(self.host.shape)
        assert hip().hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0

    def download(self):
        assert hip().hipMemcpy(self.host.ctypes.data_as(C.c_void_p), self.ptr, self.host.nbytes, D2H) == 0
        return self.host.copy()

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = None


class DevVec:
    """The five output buffers of one engine, and its action buffer."""

    def __init__(self, B, V, want=("obs", "reward", "terminal", "stepped", "n_live")):
        self.B, self.V = B, V
        self.actions = DevArray(B, np.int32)
        self.arr = {"obs": DevArray((B, V), np.float32), "reward": DevArray(B, np.float64), "terminal": DevArray(B, np.uint8),
                    "stepped": DevArray(B, np.int32), "n_live": DevArray(1, np.int32)}
        self.out = abi.VecOut(*[self.arr[k].ptr if k in want else None for k in ("obs", "reward", "terminal", "stepped", "n_live")])

    def step(self, eng, a):
        self.actions.upload(a)
        eng.vec_step(self.actions.ptr, self.out)

    def read(self, eng):
        eng.sync()
        return {k: v.download() for k, v in self.arr.items()}

    def free(self):
        self.actions.free()
        for v in self.arr.values():
            v.free()


def make_params(depth=5, trades=2, mem=1 << 16, algo=abi.ALGO_QLAMBDA):
    p = engine.default_params()
    p.depth, p.max_trades = depth, trades
    p.algo, p.theta_mode, p.memory_size = algo, abi.THETA_PRIVATE, mem
    return p


def gen(n_events, ending="dry", p=None):
    """Generator settings of the two ways an episode ends.  "dry": the default clock (half a second per event from the start of
    the session), the data ends hours before the session does.  "session": the same cadence started 150 events before the
    session's last half hour (Market::IsOpen, market.cpp:67-70), so isTerminal() comes true in the middle of the data."""
    g = engine.default_gen_params()
    g.n_events = n_events
    if ending == "session":
        g.t0_ms = int(p.market.close_ms - 30 * 60000 - 150 * g.dt_ms)
    return g


def check_observation(eng, orc, got, V, tag, books=None):
    """The contract of the outputs that holds after lob_vec_step and lob_vec_observe alike (`books`: a mask of the books compared)."""
    m = np.ones(eng.B, bool) if books is None else books
    recs = orc.recs()
    np.testing.assert_array_equal(got["obs"][m], recs["vars"][m][:, :V], err_msg=tag + ": obs against the oracle's vars")
    term = eng.get_terminal()
    np.testing.assert_array_equal(got["terminal"], term, err_msg=tag + ": terminal against lob_get_terminal")
    np.testing.assert_array_equal(got["terminal"][m], recs["book"]["terminal"][m], err_msg=tag + ": terminal against the oracle")
    assert int(got["n_live"][0]) == int((term == 0).sum()), tag + ": n_live"
    not2 = term != 2
    np.testing.assert_array_equal(got["obs"][not2], eng.get_state()[not2], err_msg=tag + ": obs against lob_get_state")
    return recs, term


def check_step(eng, orc, got, V, steps_before, tag, books=None):
    m = np.ones(eng.B, bool) if books is None else books
    eb = dumps_to_np(eng.get_books())
    recs, term = check_observation(eng, orc, got, V, tag, books)
    assert_books_equal(eb[m], recs["book"][m], tag)
    st = got["stepped"]
    assert set(np.unique(st)) <= {0, 1}, tag
    st = st.astype(bool)
    np.testing.assert_array_equal(got["reward"][st & m], recs["reward"][st & m], err_msg=tag + ": reward of the stepped books")
    assert (got["reward"][~st].view(np.uint64) == 0).all(), tag + ": reward of a book that did not step is +0.0"
    np.testing.assert_array_equal(got["reward"][st], eng.get_reward()[st], err_msg=tag + ": reward against lob_get_reward")
    if books is None:
        oc, c = orc.counters(), eng.counters()
        assert int(st.sum()) == int(oc[0] - steps_before), tag + ": stepped books against the oracle's step counter"
        assert c[0] == oc[0] and c[1] == oc[1], (tag, c, oc)
    return st, term


def run_to_the_end(eng, orc, dev, V, cap, rng, tag, every=1):
    """Random actions until n_live == 0 (at most `cap` steps), every `every`-th step and the last one checked.  -> what was seen."""
    B = eng.B
    seen = {"steps": 0, "dry_step": False, "over_while_others_step": False, "terminal": None}
    prev_term = eng.get_terminal()
    while True:
        assert seen["steps"] < cap, tag + ": the episode did not end"
        before = orc.counters()[0]
        a = rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)
        dev.step(eng, a)
        orc.env_step(a)
        seen["steps"] += 1
        got = dev.read(eng)
        last = int(got["n_live"][0]) == 0
        if seen["steps"] % every == 0 or last:
            st, term = check_step(eng, orc, got, V, before, "%s step %d" % (tag, seen["steps"]))
            live_before = prev_term == 0
            assert not st[~live_before].any(), tag + ": a book that was over has been stepped"
            seen["dry_step"] |= bool((live_before & ~st & (term == 2)).any())
            seen["over_while_others_step"] |= bool((prev_term == 1).any() and st.any())
            prev_term = term
        else:
            prev_term = got["terminal"]
        if last:
            break
    seen["terminal"] = prev_term
    return seen


# ---- 1. random actions to the end of the episode --------------------------------------------------------------------------------

@pytest.mark.parametrize("ending", ["dry", "session"])
@pytest.mark.parametrize("depth,trades", [(5, 2), (10, 2), (10, 4)])
@pytest.mark.parametrize("B", [1, 64, 200])
def test_random_actions_to_the_end(B, depth, trades, ending):
    n_events = 300
    p = make_params(depth, trades)
    V = p.n_vars
    rec = engine.gen_stream_host(gen(n_events, ending, p), depth, trades, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    dev = DevVec(B, V)
    eng.reset()
    orc.reset()
    eng.vec_observe(dev.out)
    got = dev.read(eng)
    compare_env(eng, orc, "reset")
    check_observation(eng, orc, got, V, "after reset")
    np.testing.assert_array_equal(got["obs"], eng.get_state(), err_msg="after reset: obs against lob_get_state")
    np.testing.assert_array_equal(got["reward"], eng.get_reward(), err_msg="lob_vec_observe: reward is lob_get_reward's")
    assert (got["stepped"] == 0).all()
    assert (got["terminal"] == 0).all(), "every book starts live: a condition on the inputs"
    seen = run_to_the_end(eng, orc, dev, V, n_events, np.random.default_rng(100 * B + depth + trades), "B=%d D=%d T=%d %s" % (B, depth, trades, ending))
    oterm = orc.recs()["book"]["terminal"]
    if ending == "dry":
        assert (oterm == 2).all() and seen["dry_step"], "the books run dry, and a dry step (stepped == 0) was seen"
    else:
        assert (oterm == 1).all(), "the session's last half hour arrives before the data ends"
        assert B == 1 or seen["over_while_others_step"], "books that were over were left alone while others stepped"
    assert seen["steps"] > 20
    dev.free()
    eng.close()
    orc.close()


@pytest.mark.parametrize("B,n_vars", [(300, 13), (200, 5), (64, 4)])
def test_rows_that_are_no_multiple_of_16_bytes(B, n_vars):
    """The default state has eight variables and leaves vec_observe_kernel in two 16-byte stores per lane; 13 and 5 variables take
    its other path (the block's rows through LDS), 4 the one-store form.  300 books: two blocks, the second one partial."""
    p = make_params(5, 2)
    order = np.random.default_rng(n_vars).permutation(abi.LOB_MAX_VARS)
    p.n_vars = n_vars
    for i in range(abi.LOB_MAX_VARS):
        p.vars[i] = int(order[i]) if i < n_vars else 0
    rec = engine.gen_stream_host(gen(200), 5, 2, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    dev = DevVec(B, n_vars)
    eng.reset()
    orc.reset()
    eng.vec_observe(dev.out)
    check_observation(eng, orc, dev.read(eng), n_vars, "after reset")
    seen = run_to_the_end(eng, orc, dev, n_vars, 200, np.random.default_rng(B), "B=%d V=%d" % (B, n_vars), every=5)
    assert seen["steps"] > 20 and (seen["terminal"] == 2).all()
    dev.free()
    eng.close()
    orc.close()


# ---- 2. closed loop with no host in it -----------------------------------------------------------------------------------------

def test_closed_loop_through_torch_with_no_host_in_it():
    """B = 256, 120 steps through VecEnv, the action an exact function of the previous observation computed by torch on the
    device, the oracle driven by the same function in numpy: tests/vec_env_torch_child.py, in a process of its own because torch
    must be imported before the engine library is loaded (one HIP runtime per process) and this process has loaded it."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vec_env_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "vec_env_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "closed loop OK" in res.stdout


# ---- 3. a day library, with the step log on --------------------------------------------------------------------------------------

def test_day_library_two_episodes_with_the_step_log():
    from tests.test_gpu_days import make_days
    from tests.test_gpu_step_log import Expect, assert_log_equals, oracle_books
    B, lengths = 48, (150, 220, 300)
    p = make_params(5, 2)
    V = p.n_vars
    days = make_days(lengths, depth=5)
    lib = ol.DayLibrary(days)
    eng = engine.Engine(p, B)
    eng.load_days(days)
    orc = ol.Oracle(p, np.stack([days[0]] * B))   # (never played: every episode's days come by set_days)
    sel = np.array([0, 5, 11, 17, 23, 31, 40, 47], np.int32)
    eng.step_log_enable(sel, 512)
    dev = DevVec(B, V)
    rng = np.random.default_rng(3)
    assign = [np.arange(B) % 3, (np.arange(B) // 3 + 1) % 3]
    for episode in range(2):
        assert len(np.unique(assign[episode][sel])) == 3 and (assign[0] != assign[1]).any()
        eng.days_set(assign[episode])
        eng.reset()
        np.testing.assert_array_equal(eng.days(), assign[episode])
        orc.set_days(*lib.of(assign[episode]))
        orc.reset()
        eng.vec_observe(dev.out)
        check_observation(eng, orc, dev.read(eng), V, "episode %d reset" % episode)
        ex = Expect(oracle_books(orc, sel))
        steps = 0
        while True:
            assert steps < max(lengths)
            before = orc.counters()[0]
            a = rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)
            dev.step(eng, a)
            orc.env_step(a)
            ex.after_step(oracle_books(orc, sel))
            steps += 1
            got = dev.read(eng)
            check_step(eng, orc, got, V, before, "episode %d step %d" % (episode, steps))
            if int(got["n_live"][0]) == 0:
                break
        n_rows = assert_log_equals(eng, sel, ex.rows, "episode %d" % episode)
        assert n_rows.min() > 20
        lens = np.array(lengths)[assign[episode]]
        assert (dumps_to_np(eng.get_books())["terminal"] == 2).all() and steps > 60 and len(set(lens)) == 3
        eng.clear_inventory()
        orc.clear_inventory()
    dev.free()
    eng.close()
    orc.close()


# ---- 4. a ring-mode stream -------------------------------------------------------------------------------------------------------

def test_ring_mode_stream_across_refills(monkeypatch):
    """A 256-entry market-track ring refilled every 16 steps (tests/test_gpu_replay.py's switches) under a 1 200-event stream:
    lob_vec_step refills it on schedule as lob_step does."""
    monkeypatch.setenv("LOB_TRACK_RING", "256")
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    B, n_events = 64, 1200
    p = make_params(10, 2)
    V = p.n_vars
    rec = engine.gen_stream_host(gen(n_events), 10, 2, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    dev = DevVec(B, V)
    eng.kernel_timing(True)
    eng.reset()
    orc.reset()
    seen = run_to_the_end(eng, orc, dev, V, n_events, np.random.default_rng(4), "ring", every=8)
    eng.sync()
    _, refills = eng.kernel_time_ms("prepass_extend_kernel")
    assert refills >= 3 and seen["steps"] > 16 * 3 + 8, (refills, seen["steps"])
    _, n_obs = eng.kernel_time_ms("vec_observe_kernel")
    _, n_act = eng.kernel_time_ms("vec_actions_kernel")
    assert n_obs == n_act == seen["steps"]
    dev.free()
    eng.close()
    orc.close()


# ---- 5. bad actions --------------------------------------------------------------------------------------------------------------

def test_bad_actions_are_counted_and_not_stepped():
    B, bad_step, bad = 64, 6, {7: -1, 41: 9}
    p = make_params(5, 2)
    V = p.n_vars
    rec = engine.gen_stream_host(gen(300), 5, 2, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    dev = DevVec(B, V)
    eng.reset()
    orc.reset()
    rng = np.random.default_rng(5)
    good = np.ones(B, bool)
    assert eng.vec_status() == (abi.LOB_OK, 0)
    for step in range(30):
        before = orc.counters()[0]
        a = rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)
        if step == bad_step:
            dumps_before = bytes(eng.get_books())
            sz = C.sizeof(abi.BookDump)
            ea = a.copy()
            for b, v in bad.items():
                ea[b] = v
            dev.step(eng, ea)
            orc.env_step(a)          # (the oracle's copies of the two books step with an action of their own and are left out from here on)
            good[list(bad)] = False
            got = dev.read(eng)
            dumps_after = bytes(eng.get_books())
            for b in bad:
                assert got["stepped"][b] == 0 and got["terminal"][b] == 0
                assert dumps_after[b * sz:(b + 1) * sz] == dumps_before[b * sz:(b + 1) * sz], "book %d was touched" % b
            check_step(eng, orc, got, V, before, "bad-action step", books=good)
            assert got["stepped"][good].all()
            rc, n = eng.vec_status()
            assert rc == abi.LOB_EINVAL and n == 2 and b"out of range" in abi.load().lob_last_error()
            assert eng.vec_status() == (abi.LOB_OK, 0)
            ticks_then = dumps_to_np(eng.get_books())["total_ticks"].copy()
            continue
        dev.step(eng, a)
        orc.env_step(a)
        got = dev.read(eng)
        check_step(eng, orc, got, V, before, "step %d" % step, books=None if good.all() else good)
        if step == bad_step + 1:
            ticks = dumps_to_np(eng.get_books())["total_ticks"]
            for b in bad:
                assert got["stepped"][b] == 1 and ticks[b] == ticks_then[b] + 1, "book %d steps normally afterwards" % b
    assert eng.vec_status() == (abi.LOB_OK, 0)
    # the count is sticky until read, and lob_reset clears it
    a = np.full(B, 9, np.int32)
    dev.step(eng, a)
    dev.step(eng, a)
    got = dev.read(eng)
    assert (got["stepped"] == 0).all()
    eng.reset()
    assert eng.vec_status() == (abi.LOB_OK, 0)
    dev.step(eng, np.full(B, -1, np.int32))
    assert eng.vec_status() == (abi.LOB_EINVAL, B)
    dev.free()
    eng.close()
    orc.close()


# ---- 6. state rules --------------------------------------------------------------------------------------------------------------

def test_state_rules_and_null_members():
    B = 200
    p = make_params(5, 2)
    V = p.n_vars
    rec = engine.gen_stream_host(gen(300), 5, 2, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    dev = DevVec(B, V)
    dev.actions.upload(np.zeros(B, np.int32))
    for call in (lambda: eng.vec_step(dev.actions.ptr, dev.out), lambda: eng.vec_observe(dev.out)):
        with pytest.raises(LobError) as ei:
            call()
        assert ei.value.code == abi.LOB_ESTATE, "before lob_reset"
    eng.reset()
    orc.reset()
    lib = abi.load()
    assert lib.lob_vec_step(eng.h, None, C.byref(dev.out)) == abi.LOB_EINVAL
    assert lib.lob_vec_step(eng.h, C.c_void_p(dev.actions.ptr), None) == abi.LOB_EINVAL
    assert lib.lob_vec_observe(eng.h, None) == abi.LOB_EINVAL
    compare_env(eng, orc, "refused calls change nothing")
    # a NULL member is skipped, the others are still right: two complementary halves, stepped side by side with the full set
    halves = [DevVec(B, V, want=("obs", "n_live")), DevVec(B, V, want=("reward", "terminal", "stepped"))]
    rng = np.random.default_rng(6)
    for step in range(6):
        before = orc.counters()[0]
        a = rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)
        h = halves[step % 2]
        h.step(eng, a)
        orc.env_step(a)
        eng.vec_observe(dev.out)       # (the full set, without a step: stepped comes back 0, reward from getReward())
        part, full = h.read(eng), dev.read(eng)
        for k, v in h.arr.items():
            unwritten = (v.host.view(np.uint8) == 0xAB).all()
            assert unwritten == (getattr(h.out, k) is None), (k, "a NULL member is skipped and the others are written")
        merged = dict(full)
        for k in h.arr:
            if getattr(h.out, k) is not None:
                merged[k] = part[k]
        if step % 2 == 0:
            merged["stepped"] = (dumps_to_np(eng.get_books())["total_ticks"] == step + 1).astype(np.int32)
            merged["reward"] = np.where(merged["stepped"] == 1, full["reward"], 0.0)
        else:
            merged["obs"], merged["n_live"] = full["obs"], full["n_live"]
        assert (full["stepped"] == 0).all()
        check_step(eng, orc, merged, V, before, "NULL members, step %d" % step)
    for h in halves:
        h.free()
    eng.td_step_begin()
    for call in (lambda: eng.vec_step(dev.actions.ptr, dev.out), lambda: eng.vec_observe(dev.out)):
        with pytest.raises(LobError) as ei:
            call()
        assert ei.value.code == abi.LOB_ESTATE, "between lob_td_step_begin and lob_td_step_end"
    eng.td_step_end()
    dev.free()
    eng.close()
    orc.close()


@pytest.mark.parametrize("algo", [abi.ALGO_SARSA, abi.ALGO_QLAMBDA], ids=["sarsa", "qlambda"])
def test_learner_steps_after_vec_steps(algo):
    """10 vec steps, then 20 learner steps, private theta: the vec path leaves the learner's bookkeeping as lob_step does."""
    B = 48
    p = make_params(5, 2, algo=algo)
    V = p.n_vars
    rec = engine.gen_stream_host(gen(400), 5, 2, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    dev = DevVec(B, V)
    eng.reset()
    orc.reset()
    rng = np.random.default_rng(8)
    for step in range(10):
        before = orc.counters()[0]
        a = rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)
        dev.step(eng, a)
        orc.env_step(a)
    check_step(eng, orc, dev.read(eng), V, before, "vec step 10")
    for step in range(20):
        eng.td_step(1)
        orc.td_step(1)
        compare_learner_step(eng, orc, "learner step %d after the vec steps" % step)
    for b in range(0, B, 9):
        np.testing.assert_array_equal(eng.theta(b), orc.theta(b))
    assert eng.vec_status() == (abi.LOB_OK, 0)
    dev.free()
    eng.close()
    orc.close()


@pytest.mark.parametrize("algo", [abi.ALGO_SARSA, abi.ALGO_QLAMBDA], ids=["sarsa", "qlambda"])
def test_learner_steps_behind_greedy_steps_skipped_books_and_dry_books(algo):
    """Named regression cases of tests/test_gpu_call_sequences.py (NOTES.md, the call sequences): learner steps, private theta, exact,
      a. behind lob_eval_step in the same episode -- reset, eval_step, td_step_begin + _end was the reduced list: the greedy step
         leaves the state behind it in the learner's `state` object, as lob_step and lob_vec_step do (include/lob_engine.h
         lob_eval_step), and the learner step acts on it;
      b. behind a lob_vec_step that skipped books (actions out of range) and behind a mid-episode lob_clear_inventory;
      c. behind vec steps in which books ran out of data -- reset, vec steps to the first dry book, td_step_begin + _end: those
         books keep their traces, and the record says so."""
    B = 48
    p = make_params(5, 2, algo=algo)
    V = p.n_vars
    rec = engine.gen_stream_host(gen(160), 5, 2, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    dev = DevVec(B, V)
    eng.reset()
    orc.reset()
    rng = np.random.default_rng(9)

    def vec(n, p_skip):
        for _ in range(n):
            a = rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)
            a[rng.random(B) < p_skip] = -1
            dev.step(eng, a)
            orc.env_step(a)
        return dev.read(eng)

    def learner(n, tag, split=False):
        for step in range(n):
            if split and eng.td_split_supported():
                eng.td_step_begin()
                eng.td_step_end()
                orc.td_step_begin()
                orc.td_step_end()
            else:
                eng.td_step(1)
                orc.td_step(1)
            compare_learner_step(eng, orc, "%s, learner step %d" % (tag, step))

    learner(3, "at the start")
    eng.eval_step(2)
    orc.eval_step(2)
    learner(3, "behind two greedy steps", split=True)
    vec(4, 0.2)
    learner(3, "behind vec steps that skipped books")
    eng.clear_inventory()
    orc.clear_inventory()
    # d. a greedy step behind a mid-episode lob_clear_inventory chooses its action in the state with the new position (reduced list:
    #    reset, eval_step, clear_inventory, eval_step): clear_inventory_kernel refreshes the latest getState()
    eng.eval_step(1)
    orc.eval_step(1)
    compare_env(eng, orc, "a greedy step behind lob_clear_inventory")
    np.testing.assert_array_equal(eng.last_actions(), orc.recs()["action"])
    np.testing.assert_array_equal(eng.rng_counters(), orc.recs()["rng_ctr"])
    learner(2, "behind lob_clear_inventory and a greedy step", split=True)
    eng.eval_step(1)
    orc.eval_step(1)
    for _ in range(60):
        got = vec(1, 0.1)
        if (got["terminal"] == 2).any():
            break
    assert (got["terminal"] == 2).any() and (got["terminal"] == 0).any(), "some books have run dry in a vec step, others are live"
    learner(3, "behind vec steps in which books ran dry", split=True)
    assert eng.vec_status()[0] == abi.LOB_EINVAL, "the skipped books were counted"
    for b in range(0, B, 9):
        np.testing.assert_array_equal(eng.theta(b), orc.theta(b))
    dev.free()
    eng.close()
    orc.close()
