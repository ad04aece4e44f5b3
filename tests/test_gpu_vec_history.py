"""lob_vec_history: the last K event records of every book, written to device memory.

The yardstick is THE HOST RECORDS THE TEST ITSELF LOADED, indexed by the engine's `rec` through tests/vec_history_expected.py (pure
numpy, tested on hand-made records by tests/test_vec_history_abi.py) and compared for equality.  `rec` itself is pinned against
lob_get_books ON THE SAME ENGINE AT THE SAME MOMENT: for every book with rec >= 0 record `rec` has exactly the dump's levels; for
every book with terminal != 2, rec == cursor - 1 (the oracle-side fact: tests/test_vec_history_abi.py); slot K - 1 of `levels` is
lob_vec_book's output.  The device buffers are the DevBuf of tests/test_gpu_vec_book.py (plain hipMalloc memory pre-filled with
0xAB, guard bytes behind them; no torch in this process); the torch face runs in tests/vec_history_torch_child.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from rl_markets_amd.engine import LobError
from tests.parity import dumps_to_np
from tests.test_gpu_days import make_days
from tests.test_gpu_vec_book import DevBook, DevBuf
from tests.test_gpu_vec_env import gen, make_params
from tests.vec_history_expected import NAMES, assert_record_has_dump_levels, expected_history

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 7, 64, 128)


class DevHist:
    """The five output buffers of lob_vec_history for one engine and one K (`want`: the members that are not NULL)."""

    def __init__(self, B, K, D, T, want=NAMES, offset=0):
        self.K = K
        self.buf = {"levels": DevBuf((B, K, 4, D), np.float32, offset), "trades": DevBuf((B, K, 2, T), np.float32, offset),
                    "time_ms": DevBuf((B, K), np.int32, offset), "n_valid": DevBuf(B, np.int32, offset), "rec": DevBuf(B, np.int32, offset)}
        self.want = tuple(want)
        self.out = abi.VecHistOut(*[self.buf[k].ptr if k in self.want else None for k in NAMES])

    def refill(self):
        for v in self.buf.values():
            v.refill()

    def read(self, eng):
        eng.sync()
        got = {}
        for k, v in self.buf.items():
            got[k], fenced = v.download()
            assert fenced, "%s: bytes outside the buffer were written" % k
        return got

    def free(self):
        for v in self.buf.values():
            v.free()


class Source:
    """The host records an engine plays: flat [n][W], the first record and the length of every book's stream in it."""

    def __init__(self, flat, start, length):
        self.flat = np.ascontiguousarray(flat, dtype=np.uint32)
        self.start = np.asarray(start, dtype=np.int64)
        self.length = np.broadcast_to(np.asarray(length, dtype=np.int64), self.start.shape)

    @staticmethod
    def per_book(rec):
        B, n, W = rec.shape
        return Source(rec.reshape(B * n, W), np.arange(B, dtype=np.int64) * n, n)


class Seen:
    """What the comparisons of one test have covered."""

    def __init__(self):
        self.terminal, self.short, self.full, self.pairs, self.strong = set(), 0, 0, 0, 0

    def assert_covered(self, terminals):
        assert self.terminal == set(terminals), "books in these terminal states were compared: %s" % sorted(self.terminal)
        assert self.short > 0 and self.full > 0, "books with n_valid < K and with n_valid == K were compared"
        assert 2 * self.strong >= self.pairs > 0, "at least half of the (book, step) pairs pin rec by the cursor: %d of %d" % (self.strong, self.pairs)


def check(eng, devs, src, D, T, tag, seen, book=None):
    """lob_vec_history for every K of `devs` (into buffers refilled with 0xAB), lob_vec_book and lob_get_books, now.  -> the dump"""
    for dev in devs:
        dev.refill()
        eng.vec_history(dev.K, dev.out)
    if book is not None:
        eng.vec_book(book.out)
    got = [dev.read(eng) for dev in devs]
    dump = dumps_to_np(eng.get_books())
    rec = got[0]["rec"] if "rec" in devs[0].want else None
    assert rec is not None, "the first set of buffers carries rec"
    # rec, pinned
    assert ((rec >= -1) & (rec < src.length)).all(), tag + ": rec within the book's stream"
    assert_record_has_dump_levels(src.flat, src.start, rec, dump, D, tag + ": record rec against lob_get_books")
    strong = dump["terminal"] != 2
    np.testing.assert_array_equal(rec[strong], dump["cursor"][strong] - 1, err_msg=tag + ": rec against cursor - 1 where terminal != 2")
    lv_book = book.read(eng)["levels"] if book is not None else None
    for dev, g in zip(devs, got):
        exp = expected_history(src.flat, src.start, src.length, rec, dev.K, D, T)
        for k in NAMES:
            if k in dev.want:
                np.testing.assert_array_equal(g[k], exp[k], err_msg="%s K=%d: %s against the host records" % (tag, dev.K, k))
            else:
                assert (g[k].view(np.uint8) == 0xAB).all(), "%s K=%d: %s is NULL and was written" % (tag, dev.K, k)
        if lv_book is not None and "levels" in dev.want:
            have = rec >= 0
            np.testing.assert_array_equal(g["levels"][have, dev.K - 1], lv_book[have], err_msg="%s K=%d: slot K-1 against lob_vec_book" % (tag, dev.K))
        seen.short += int((exp["n_valid"] < dev.K).sum())
        seen.full += int((exp["n_valid"] == dev.K).sum())
    seen.terminal |= set(np.unique(dump["terminal"]).tolist())
    seen.pairs += len(rec)
    seen.strong += int(strong.sum())
    return dump


class Stepper:
    """lob_vec_step with random actions from a device buffer."""

    def __init__(self, eng, seed):
        self.eng, self.rng = eng, np.random.default_rng(seed)
        self.actions = DevBuf(eng.B, np.int32)
        self.vout = abi.VecOut(None, None, None, None, None)

    def step(self):
        self.actions.upload(self.rng.integers(0, abi.LOB_N_ACTIONS, size=self.eng.B).astype(np.int32))
        self.eng.vec_step(self.actions.ptr, self.vout)

    def free(self):
        self.actions.free()


def run_to_the_end(eng, st, devs, src, D, T, tag, seen, book=None, limit=1000):
    d = check(eng, devs, src, D, T, tag + " after reset", seen, book)
    steps = 0
    while (d["terminal"] == 0).any():
        assert steps < limit, tag + ": the episode did not end"
        st.step()
        steps += 1
        d = check(eng, devs, src, D, T, "%s vec step %d" % (tag, steps), seen, book)
    return d, steps


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trades", [1, 2, 8])
@pytest.mark.parametrize("depth", [1, 5, 10])
@pytest.mark.parametrize("B", [1, 3, 65, 257])
def test_every_shape_against_the_host_records(B, depth, trades):
    """K = 1, 2, 7, 64 and 128 side by side at every point, both ways an episode ends (tests/test_gpu_vec_env.py gen(): "dry" ->
    terminal 2, "session" -> terminal 1; tests/test_vec_history_abi.py shows on the oracle that these lengths leave most pairs
    at terminal != 2 and take rec from below 64 to beyond 128).  After lob_reset, after every one of 40 lob_vec_steps with random
    actions, after lob_td_step(5), lob_eval_step(3) and lob_clear_inventory, and after every further lob_vec_step until no book is live."""
    seen = Seen()
    for ending, n_events in (("dry", 150), ("session", 300)):
        tag = "B=%d D=%d T=%d %s" % (B, depth, trades, ending)
        p = make_params(depth, trades)
        rec = engine.gen_stream_host(gen(n_events, ending, p), depth, trades, 0, B)
        src = Source.per_book(rec)
        eng = engine.Engine(p, B)
        eng.load_events(rec)
        devs = [DevHist(B, K, depth, trades) for K in KS]
        book = DevBook(B, depth)
        st = Stepper(eng, 1000 * B + 10 * depth + trades)
        eng.reset()
        d = check(eng, devs, src, depth, trades, tag + " after reset", seen, book)
        assert (d["terminal"] == 0).all(), "a condition on the inputs"
        for step in range(40):
            st.step()
            check(eng, devs, src, depth, trades, "%s vec step %d" % (tag, step), seen, book)
        eng.td_step(5)
        check(eng, devs, src, depth, trades, tag + " after lob_td_step(5)", seen, book)
        eng.eval_step(3)
        check(eng, devs, src, depth, trades, tag + " after lob_eval_step(3)", seen, book)
        eng.clear_inventory()
        d = check(eng, devs, src, depth, trades, tag + " after lob_clear_inventory", seen, book)
        extra = 0
        while (d["terminal"] == 0).any():
            assert extra < n_events, tag + ": the episode did not end"
            st.step()
            extra += 1
            d = check(eng, devs, src, depth, trades, "%s further vec step %d" % (tag, extra), seen, book)
        assert (d["terminal"] == (2 if ending == "dry" else 1)).all(), tag
        assert eng.vec_status() == (abi.LOB_OK, 0)
        st.free()
        book.free()
        for dev in devs:
            dev.free()
        eng.close()
    seen.assert_covered({0, 1, 2})


def test_hardened_stream_windows():
    """A stream of tests/hard_streams.py to the end of the data: windows that contain rows sharing a timestamp (their trade slots
    zeroed), crossed rows and prices off the grid, against the host records as everywhere else."""
    from tests import hard_streams as hs
    B, depth, trades = 65, hs.DEPTH, hs.TRADES
    rec, _, rows = hs.batch("all")
    rec, same = rec[:B], rows["same_time"][:B]
    src = Source.per_book(rec)
    eng = engine.Engine(make_params(depth, trades), B)
    eng.load_events(rec)
    devs = [DevHist(B, K, depth, trades) for K in (7, 64)]
    book = DevBook(B, depth)
    st = Stepper(eng, 78)
    seen = Seen()
    eng.reset()
    d, steps = run_to_the_end(eng, st, devs, src, depth, trades, "hardened", seen, book)
    got = devs[0].read(eng)
    # the last windows of 7 rows: some hold a same-timestamp row, whose time repeats and whose trade slots are empty
    idx = got["rec"][:, None] - (6 - np.arange(7))[None, :]
    in_window = np.take_along_axis(same, np.clip(idx, 0, hs.N_EVENTS - 1), axis=1) & (idx >= 0)
    later = in_window.copy()
    later[:, 0] = False                       # (slot 0 has no predecessor in the window)
    assert later.any()
    bs, ks = np.nonzero(later)
    np.testing.assert_array_equal(got["time_ms"][bs, ks], got["time_ms"][bs, ks - 1])
    assert (got["trades"][in_window] == 0).all()
    assert eng.vec_status() == (abi.LOB_OK, 0)
    st.free()
    book.free()
    for dev in devs:
        dev.free()
    eng.close()


# ---- 2. stream modes -----------------------------------------------------------------------------------------------------------------

def test_replayed_stream_never_reads_before_the_phase():
    """lob_load_events_shared with every phase[b] >= K: the records before a book's window exist and are not zero, and must not
    show."""
    B, depth, trades, n_total, n_events, K = 65, 5, 2, 700, 200, 128
    p = make_params(depth, trades)
    day = engine.gen_stream_host(gen(n_total), depth, trades, 0, 1)[0]
    rng = np.random.default_rng(5)
    phase = rng.integers(K, n_total - n_events + 1, size=B)
    phase[0], phase[1], phase[2] = K, n_total - n_events, phase[3]
    assert (phase >= K).all() and day[:, 2].all()
    src = Source(day, phase, n_events)
    eng = engine.Engine(p, B)
    eng.load_events_shared(day, phase, n_events)
    devs = [DevHist(B, K, depth, trades), DevHist(B, 7, depth, trades)]
    book = DevBook(B, depth)
    st = Stepper(eng, 6)
    seen = Seen()
    eng.reset()
    d, steps = run_to_the_end(eng, st, devs, src, depth, trades, "replayed stream", seen, book)
    seen.assert_covered({0, 2})
    assert steps > 20
    st.free()
    book.free()
    for dev in devs:
        dev.free()
    eng.close()


@pytest.mark.parametrize("ring", [False, True], ids=["resident track", "ring-mode track"])
def test_day_library_of_unequal_days(monkeypatch, ring):
    """lob_load_days, three days of unequal length, two episodes with a fresh random draw each: a book's window is its day's
    records and ends at its day's first record, whichever day lies before it in the library.  Once with the longest day longer
    than the resident track (tests/test_gpu_days_shared.py: a 256-entry ring refilled every 16 steps)."""
    lengths = [150, 170, 300]
    if ring:
        monkeypatch.setenv("LOB_TRACK_RING", "256")
        monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    B, depth, trades = 65, 10, 2
    p = engine.default_params()
    p.depth, p.max_trades = depth, trades
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_SHARED, 1 << 20
    days = make_days(lengths, depth=depth)
    flat = np.concatenate(days)
    day_first = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    eng = engine.Engine(p, B)
    eng.load_days(days)
    eng.kernel_timing(True)
    eng.days_select(abi.DAYS_RANDOM, 0, len(days))   # (the correlated first draw, replaced below before any reset)
    devs = [DevHist(B, 128, depth, trades), DevHist(B, 7, depth, trades)]
    book = DevBook(B, depth)
    st = Stepper(eng, 7)
    seen = Seen()
    drawn = []
    for ep in range(2):
        eng.days_select(abi.DAYS_RANDOM, 0, len(days))
        eng.reset()
        d = eng.days()
        drawn.append(d.copy())
        assert len(np.unique(d)) == len(days) and (d > 0).sum() > B // 3, "books on every day, many on days > 0"
        src = Source(flat, day_first[d], np.array(lengths)[d])
        dump, steps = run_to_the_end(eng, st, devs, src, depth, trades, "days episode %d" % ep, seen, book)
        assert (dump["terminal"] == 2).all() and steps > 40
        eng.clear_inventory()
        check(eng, devs, src, depth, trades, "days episode %d after lob_clear_inventory" % ep, seen, book)
        eng.handle_terminal()
    assert (drawn[0] != drawn[1]).any(), "a new draw"
    seen.assert_covered({0, 2})
    eng.sync()
    _, refills = eng.kernel_time_ms("prepass_extend_kernel")
    assert refills >= 2 or not ring, refills
    st.free()
    book.free()
    for dev in devs:
        dev.free()
    eng.close()


def test_streams_generated_on_the_device():
    """lob_gen_events_device: no host copy was ever uploaded; lob_gen_stream_host makes the same records."""
    B, depth, trades = 257, 10, 2
    p = make_params(depth, trades)
    g = gen(150)
    eng = engine.Engine(p, B)
    eng.gen_events(g)
    src = Source.per_book(engine.gen_stream_host(g, depth, trades, int(p.book_id_offset), B))
    devs = [DevHist(B, 64, depth, trades), DevHist(B, 2, depth, trades)]
    st = Stepper(eng, 8)
    seen = Seen()
    eng.reset()
    run_to_the_end(eng, st, devs, src, depth, trades, "device-generated streams", seen, None)
    seen.assert_covered({0, 2})
    st.free()
    for dev in devs:
        dev.free()
    eng.close()


def test_staged_stream_is_followed_after_the_reset():
    """lob_stage_events, then lob_reset: history is read from the stream handed over, not from the buffer the engine started with."""
    B, depth, trades, n, K = 65, 5, 2, 200, 64
    p = make_params(depth, trades)
    rec_a = engine.gen_stream_host(gen(n), depth, trades, 0, B)
    g = gen(n)
    g.seed = 777
    rec_b = engine.gen_stream_host(g, depth, trades, 1000, B)
    assert not np.array_equal(rec_a[:, :, 2:], rec_b[:, :, 2:])
    eng = engine.Engine(p, B)
    eng.load_events(rec_a)
    devs = [DevHist(B, K, depth, trades)]
    book = DevBook(B, depth)
    st = Stepper(eng, 9)
    seen = Seen()
    eng.reset()
    eng.stage_events(rec_b)
    for step in range(10):
        st.step()
        check(eng, devs, Source.per_book(rec_a), depth, trades, "first stream, step %d" % step, seen, book)
    eng.clear_inventory()
    eng.handle_terminal()
    eng.reset()                      # (adopts the staged stream)
    src = Source.per_book(rec_b)
    check(eng, devs, src, depth, trades, "staged stream after reset", seen, book)
    for step in range(30):
        st.step()
        check(eng, devs, src, depth, trades, "staged stream, step %d" % step, seen, book)
    assert seen.short > 0 and seen.full > 0
    st.free()
    book.free()
    devs[0].free()
    eng.close()


# ---- 3. NULL members, unaligned destinations, return codes -----------------------------------------------------------------------------

def stepped_engine(B, depth, trades, steps=30, seed=4):
    p = make_params(depth, trades)
    rec = engine.gen_stream_host(gen(200), depth, trades, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    st = Stepper(eng, seed)
    eng.reset()
    for _ in range(steps):
        st.step()
    eng.sync()
    st.free()
    return eng, Source.per_book(rec)


def test_null_members_and_guard_words():
    """Each member NULL in turn: that buffer keeps its fill, the others are written in full; all NULL: LOB_OK, nothing written.
    `rec` is then taken from a full set of buffers filled by the call before."""
    B, depth, trades, K = 67, 5, 2, 7
    eng, src = stepped_engine(B, depth, trades)
    seen = Seen()
    full = DevHist(B, K, depth, trades)
    for missing in NAMES:
        dev = DevHist(B, K, depth, trades, want=[n for n in NAMES if n != missing])
        check(eng, [full, dev], src, depth, trades, "without " + missing, seen)
        dev.free()
    for only in NAMES:
        dev = DevHist(B, K, depth, trades, want=[only])
        check(eng, [full, dev], src, depth, trades, "only " + only, seen)
        dev.free()
    dev = DevHist(B, K, depth, trades, want=())
    assert abi.load().lob_vec_history(eng.h, K, C.byref(dev.out)) == abi.LOB_OK
    got = dev.read(eng)
    assert all((got[k].view(np.uint8) == 0xAB).all() for k in NAMES), "all members NULL: nothing is written"
    dev.free()
    full.free()
    eng.close()


@pytest.mark.parametrize("depth,trades", [(5, 1), (10, 2), (3, 8)])
def test_destinations_that_are_not_16_byte_aligned(depth, trades):
    B = 67
    eng, src = stepped_engine(B, depth, trades)
    seen = Seen()
    for K in (1, 7, 64):
        dev, off = DevHist(B, K, depth, trades), DevHist(B, K, depth, trades, offset=4)
        assert all(dev.buf[k].ptr % 16 == 0 and off.buf[k].ptr % 16 == 4 for k in NAMES)
        check(eng, [dev, off], src, depth, trades, "aligned, and 4 bytes into the allocation", seen)   # (the four bytes before and the guard behind: DevHist.read)
        dev.free()
        off.free()
    eng.close()


def test_return_codes():
    B, depth, trades = 65, 5, 2
    p = make_params(depth, trades)
    rec = engine.gen_stream_host(gen(200), depth, trades, 0, B)
    src = Source.per_book(rec)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    dev = DevHist(B, 8, depth, trades)
    lib = abi.load()
    seen = Seen()
    with pytest.raises(LobError) as ei:
        eng.vec_history(8, dev.out)
    assert ei.value.code == abi.LOB_ESTATE, "before the first lob_reset"
    eng.reset()
    check(eng, [dev], src, depth, trades, "after the refusal before lob_reset", seen)
    for K in (0, 129, -1):
        assert lib.lob_vec_history(eng.h, K, C.byref(dev.out)) == abi.LOB_EINVAL
        assert b"lob_vec_history" in lib.lob_last_error()
    assert lib.lob_vec_history(eng.h, 8, None) == abi.LOB_EINVAL and lib.lob_vec_history(None, 8, C.byref(dev.out)) == abi.LOB_EINVAL
    eng.td_step(2)
    check(eng, [dev], src, depth, trades, "after the refusals", seen)
    eng.td_step_begin()
    with pytest.raises(LobError) as ei:
        eng.vec_history(8, dev.out)
    assert ei.value.code == abi.LOB_ESTATE, "between lob_td_step_begin and lob_td_step_end"
    eng.td_step_end()
    d = check(eng, [dev], src, depth, trades, "after lob_td_step_end", seen)
    assert (d["total_ticks"] == 3).all()
    dev.free()
    eng.close()


# ---- 4. no engine state changed --------------------------------------------------------------------------------------------------------

def test_learner_is_unaffected():
    """Two engines run the same 30 learner steps; one enqueues lob_vec_history behind every step, one never does: lob_get_books
    and the weights are bit-identical."""
    B, depth, trades = 48, 5, 2
    p = make_params(depth, trades)
    rec = engine.gen_stream_host(gen(400), depth, trades, 0, B)
    engs = []
    for _ in range(2):
        e = engine.Engine(p, B)
        e.load_events(rec)
        e.reset()
        engs.append(e)
    dev = DevHist(B, 32, depth, trades)
    for step in range(30):
        for e in engs:
            e.td_step(1)
        engs[0].vec_history(32, dev.out)
    assert bytes(engs[0].get_books()) == bytes(engs[1].get_books())
    for b in range(0, B, 5):
        np.testing.assert_array_equal(engs[0].theta(b), engs[1].theta(b))
    np.testing.assert_array_equal(engs[0].rng_counters(), engs[1].rng_counters())
    check(engs[0], [dev], Source.per_book(rec), depth, trades, "after 30 learner steps", Seen())
    dev.free()
    for e in engs:
        e.close()


# ---- the torch face ----------------------------------------------------------------------------------------------------------------------

def test_vec_env_with_the_history_through_torch():
    """VecEnv(eng, history=16): tests/vec_history_torch_child.py, in a fresh process of its own because torch must be imported
    before the engine library is loaded (one HIP runtime per process) and this process has loaded it."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vec_history_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "vec_history_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "vec history OK" in res.stdout
