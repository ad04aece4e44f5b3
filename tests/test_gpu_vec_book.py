"""lob_vec_book: the depth levels, the agent's own words and the market time of every book, written to device memory.

The yardstick is lob_get_books ON THE SAME ENGINE AT THE SAME MOMENT, converted in numpy (astype(np.float32): IEEE round to nearest
even, like the contract) and compared for equality -- the rest of the suite pins lob_get_books to the oracle.  The device buffers
are plain hipMalloc memory pre-filled with 0xAB with 64 guard bytes behind them (no torch in this process: one HIP runtime per
process, rl_markets_amd/abi.py); the torch-facing wrapper runs in a process of its own (tests/vec_book_torch_child.py)."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from rl_markets_amd.engine import LobError
from tests import oracle_lib as ol
from tests.parity import compare_learner_step, dumps_to_np
from tests.test_gpu_days import make_days
from tests.test_gpu_vec_env import gen, hip, make_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H2D, D2H = 1, 2
GUARD = 64
NAMES = ("levels", "own", "time_ms")


class DevBuf:
    """hipMalloc memory with a numpy face (the DevArray of tests/test_gpu_vec_env.py) that starts `offset` bytes into its allocation
    and has GUARD bytes behind it; everything is filled with 0xAB, a value no output takes."""

    def __init__(self, shape, dtype, offset=0):
        self.shape, self.dtype, self.offset = shape, np.dtype(dtype), offset
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        self.total = offset + self.nbytes + GUARD
        p = C.c_void_p()
        assert hip().hipMalloc(C.byref(p), self.total) == 0
        self.base = p.value
        self.ptr = self.base + offset
        self.refill()

    def refill(self):
        assert hip().hipMemset(self.base, 0xAB, self.total) == 0

    def upload(self, a):
        a = np.ascontiguousarray(a, self.dtype).reshape(self.shape)
        assert hip().hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0

    def download(self):
        """-> (the array, True when the bytes before and behind it still hold the fill)"""
        raw = np.zeros(self.total, np.uint8)
        assert hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), self.base, self.total, D2H) == 0
        body = raw[self.offset:self.offset + self.nbytes]
        fenced = bool((raw[:self.offset] == 0xAB).all() and (raw[self.offset + self.nbytes:] == 0xAB).all())
        return body.view(self.dtype).reshape(self.shape).copy(), fenced

    def free(self):
        if self.base:
            hip().hipFree(self.base)
            self.base = None


class DevBook:
    """The three output buffers of lob_vec_book for one engine (`want`: the members that are not NULL)."""

    def __init__(self, B, D, want=NAMES, offset=0):
        self.buf = {"levels": DevBuf((B, 4, D), np.float32, offset), "own": DevBuf((B, abi.VEC_OWN_WORDS), np.float32, offset),
                    "time_ms": DevBuf(B, np.int64)}
        self.want = tuple(want)
        self.out = abi.VecBookOut(*[self.buf[k].ptr if k in self.want else None for k in NAMES])

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


def expected(dump, D):
    """What the contract names, from the dump records of lob_get_books."""
    lv = np.stack([dump["ask_px"][:, :D], dump["ask_vol"][:, :D], dump["bid_px"][:, :D], dump["bid_vol"][:, :D]], axis=1).astype(np.float32)
    own = np.stack([dump[f].astype(np.float32) for f in abi.OWN_FIELDS], axis=1)
    return {"levels": lv, "own": own, "time_ms": dump["time_ms"].astype(np.int64)}


def assert_book_equals_dump(eng, dev, D, tag, want=NAMES):
    """lob_vec_book now, and lob_get_books now.  -> the dump"""
    eng.vec_book(dev.out)
    got = dev.read(eng)
    dump = dumps_to_np(eng.get_books())
    exp = expected(dump, D)
    for k in NAMES:
        if k in want:
            np.testing.assert_array_equal(got[k], exp[k], err_msg="%s: %s against lob_get_books" % (tag, k))
        else:
            assert (got[k].view(np.uint8) == 0xAB).all(), "%s: %s is NULL and was written" % (tag, k)
    return dump


def make_engine(B, depth, trades, n_events, ending="dry", algo=abi.ALGO_QLAMBDA):
    p = make_params(depth, trades, algo=algo)
    rec = engine.gen_stream_host(gen(n_events, ending, p), depth, trades, 0, B)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    return p, rec, eng


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trades", [1, 2, 8])
@pytest.mark.parametrize("depth", [1, 5, 10])
@pytest.mark.parametrize("B", [1, 3, 65, 257, 300])
def test_every_shape_against_the_dump(B, depth, trades):
    """Both ways an episode ends (tests/test_gpu_vec_env.py gen(): "dry" -> terminal 2, "session" -> terminal 1).  After lob_reset,
    after every one of 40 lob_vec_steps with random actions, after lob_td_step(5), lob_eval_step(3) and lob_clear_inventory -- and,
    because these streams end around step 50-60 whatever the agent does, after every further lob_vec_step until no book is live, so
    that books in all three terminal states are compared."""
    seen = set()
    for ending, n_events in (("dry", 150), ("session", 300)):
        tag = "B=%d D=%d T=%d %s" % (B, depth, trades, ending)
        p, rec, eng = make_engine(B, depth, trades, n_events, ending)
        dev = DevBook(B, depth)
        actions = DevBuf(B, np.int32)
        vout = abi.VecOut(None, None, None, None, None)
        rng = np.random.default_rng(1000 * B + 10 * depth + trades)

        def vec_step():
            actions.upload(rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32))
            eng.vec_step(actions.ptr, vout)

        eng.reset()
        d = assert_book_equals_dump(eng, dev, depth, tag + " after reset")
        assert (d["ask_px"][:, :depth] > 0).all() and (d["terminal"] == 0).all(), "a condition on the inputs"
        seen |= set(np.unique(d["terminal"]).tolist())
        for step in range(40):
            vec_step()
            d = assert_book_equals_dump(eng, dev, depth, "%s vec step %d" % (tag, step))
            seen |= set(np.unique(d["terminal"]).tolist())
        if B >= 65:
            assert d["ask_has_order"].any() and d["bid_has_order"].any() and (d["position"] != 0).any(), "the own words are not all zero"
        eng.td_step(5)
        d = assert_book_equals_dump(eng, dev, depth, tag + " after lob_td_step(5)")
        eng.eval_step(3)
        d = assert_book_equals_dump(eng, dev, depth, tag + " after lob_eval_step(3)")
        eng.clear_inventory()
        d = assert_book_equals_dump(eng, dev, depth, tag + " after lob_clear_inventory")
        seen |= set(np.unique(d["terminal"]).tolist())
        extra = 0
        while (d["terminal"] == 0).any():
            assert extra < n_events, tag + ": the episode did not end"
            vec_step()
            extra += 1
            d = assert_book_equals_dump(eng, dev, depth, "%s further vec step %d" % (tag, extra))
            seen |= set(np.unique(d["terminal"]).tolist())
        assert (d["terminal"] == (2 if ending == "dry" else 1)).all(), tag
        assert eng.vec_status() == (abi.LOB_OK, 0)
        actions.free()
        dev.free()
        eng.close()
    assert seen == {0, 1, 2}, "books in all three terminal states were compared"


# ---- 2. a batch beyond the 16-lanes-per-book env kernel --------------------------------------------------------------------------------

def test_larger_batch_with_one_weight_vector():
    B, depth, trades = 4160, 10, 2
    p = make_params(depth, trades)
    p.theta_mode, p.memory_size = abi.THETA_SHARED, 1 << 20
    g = gen(200)
    eng = engine.Engine(p, B)
    eng.gen_events(g)
    dev = DevBook(B, depth)
    eng.reset()
    assert_book_equals_dump(eng, dev, depth, "B=4160 after reset")
    for step in range(10):
        eng.td_step(1)
        d = assert_book_equals_dump(eng, dev, depth, "B=4160 learner step %d" % step)
    assert (d["total_ticks"] == 10).all() and len(np.unique(d["ask_px"][:, 0])) > 1
    dev.free()
    eng.close()


def test_hardened_stream_with_crossed_books():
    """A stream of tests/hard_streams.py (rows that share a timestamp, crossed rows, prices off the grid, jumps): after the reset and
    every lob_vec_step to the end of the data.  A book whose data ends inside a run of crossed rows is left crossed: those levels too."""
    from tests import hard_streams as hs
    B, depth, trades = 65, hs.DEPTH, hs.TRADES
    rec = hs.batch("all")[0][:B]
    eng = engine.Engine(make_params(depth, trades), B)
    eng.load_events(rec)
    dev = DevBook(B, depth)
    actions = DevBuf(B, np.int32)
    vout = abi.VecOut(None, None, None, None, None)
    rng = np.random.default_rng(77)
    eng.reset()
    d = assert_book_equals_dump(eng, dev, depth, "hardened after reset")
    crossed, steps = 0, 0
    while (d["terminal"] == 0).any():
        assert steps < hs.N_EVENTS, "the episode did not end"
        actions.upload(rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32))
        eng.vec_step(actions.ptr, vout)
        steps += 1
        d = assert_book_equals_dump(eng, dev, depth, "hardened vec step %d" % steps)
        crossed += int((d["ask_px"][:, 0] < d["bid_px"][:, 0]).sum())
    assert crossed > 0, "crossed books were compared"
    assert eng.vec_status() == (abi.LOB_OK, 0)
    actions.free()
    dev.free()
    eng.close()


# ---- 3. a day library whose longest day is longer than the resident track -------------------------------------------------------------

def test_day_library_in_ring_mode(monkeypatch):
    lengths, ring = [100, 108, 116, 124, 132, 300], 256     # tests/test_gpu_days_shared.py
    monkeypatch.setenv("LOB_TRACK_RING", str(ring))
    monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    B, depth = 64, 10
    p = engine.default_params()
    p.depth, p.max_trades = depth, 2
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_SHARED, 20000000
    days = make_days(lengths, depth=depth)
    assert max(lengths) > ring
    eng = engine.Engine(p, B)
    eng.load_days(days)
    eng.days_select(abi.DAYS_IN_ORDER, 0, len(days))
    eng.kernel_timing(True)
    dev = DevBook(B, depth)
    eng.reset()
    assert len(np.unique(eng.days())) == len(days)
    d = assert_book_equals_dump(eng, dev, depth, "days after reset")
    steps, saw_mixed = 0, False
    while (d["terminal"] == 0).any():
        assert steps < max(lengths)
        eng.td_step(1)
        steps += 1
        d = assert_book_equals_dump(eng, dev, depth, "days learner step %d" % steps)
        saw_mixed |= bool((d["terminal"] == 0).any() and (d["terminal"] != 0).any())
    eng.sync()
    _, refills = eng.kernel_time_ms("prepass_extend_kernel")
    _, launches = eng.kernel_time_ms("vec_book_kernel")
    assert refills >= 3 and steps > 3 * 16 and saw_mixed and launches == steps + 1, (refills, steps, saw_mixed, launches)
    dev.free()
    eng.close()


# ---- 4. NULL members, 5. unaligned destinations -----------------------------------------------------------------------------------------

def stepped_engine(B, depth, steps=12, seed=4):
    p, rec, eng = make_engine(B, depth, 2, 200)
    actions = DevBuf(B, np.int32)
    vout = abi.VecOut(None, None, None, None, None)
    rng = np.random.default_rng(seed)
    eng.reset()
    for _ in range(steps):
        actions.upload(rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32))
        eng.vec_step(actions.ptr, vout)
    eng.sync()
    actions.free()
    return eng


def test_null_members_and_guard_words():
    B, depth = 300, 5
    eng = stepped_engine(B, depth)
    subsets = [s for n in (1, 2, 3) for s in itertools.combinations(NAMES, n)]
    assert len(subsets) == 7
    for want in subsets:
        dev = DevBook(B, depth, want=want)
        assert_book_equals_dump(eng, dev, depth, "members " + "+".join(want), want=want)   # (the guards: DevBook.read)
        dev.free()
    dev = DevBook(B, depth, want=())
    assert abi.load().lob_vec_book(eng.h, C.byref(dev.out)) == abi.LOB_OK
    got = dev.read(eng)
    assert all((got[k].view(np.uint8) == 0xAB).all() for k in NAMES), "all members NULL: nothing is written"
    dev.free()
    eng.close()


@pytest.mark.parametrize("depth", [5, 10])
def test_destinations_that_are_not_16_byte_aligned(depth):
    B = 300
    eng = stepped_engine(B, depth)
    dev, off = DevBook(B, depth), DevBook(B, depth, offset=4)
    assert dev.buf["levels"].ptr % 16 == 0 and off.buf["levels"].ptr % 16 == 4 and off.buf["own"].ptr % 16 == 4
    assert_book_equals_dump(eng, dev, depth, "aligned")
    assert_book_equals_dump(eng, off, depth, "4 bytes into the allocation")   # (the four bytes before and the guard behind: DevBook.read)
    dev.free()
    off.free()
    eng.close()


# ---- 6. no engine state changed --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_book", [False, True], ids=["plain", "with lob_vec_book"])
def test_learner_run_against_the_oracle_is_unchanged(with_book):
    """30 learner steps against the oracle through tests/parity.py, once as they are and once with lob_vec_book enqueued behind
    every step: books, weights and random-number counters equal the oracle's either way."""
    B, depth = 48, 5
    p, rec, eng = make_engine(B, depth, 2, 400)
    orc = ol.Oracle(p, rec)
    dev = DevBook(B, depth)
    eng.reset()
    orc.reset()
    for step in range(30):
        eng.td_step(1)
        if with_book:
            eng.vec_book(dev.out)
        orc.td_step(1)
        compare_learner_step(eng, orc, "learner step %d" % step)
    for b in range(0, B, 5):
        np.testing.assert_array_equal(eng.theta(b), orc.theta(b))
    np.testing.assert_array_equal(eng.rng_counters(), orc.recs()["rng_ctr"])
    if with_book:
        np.testing.assert_array_equal(dev.read(eng)["levels"], expected(dumps_to_np(eng.get_books()), depth)["levels"])
    dev.free()
    eng.close()
    orc.close()


# ---- 7. call-sequence errors -----------------------------------------------------------------------------------------------------------

def test_call_sequence_errors():
    B, depth = 65, 5
    p, rec, eng = make_engine(B, depth, 2, 200)
    dev = DevBook(B, depth)
    lib = abi.load()
    with pytest.raises(LobError) as ei:
        eng.vec_book(dev.out)
    assert ei.value.code == abi.LOB_ESTATE, "before the first lob_reset"
    eng.reset()
    assert_book_equals_dump(eng, dev, depth, "after the refusal before lob_reset")
    assert lib.lob_vec_book(eng.h, None) == abi.LOB_EINVAL and lib.lob_last_error()
    assert lib.lob_vec_book(None, C.byref(dev.out)) == abi.LOB_EINVAL
    eng.td_step(2)
    assert_book_equals_dump(eng, dev, depth, "after the refusal of a NULL out")
    eng.td_step_begin()
    with pytest.raises(LobError) as ei:
        eng.vec_book(dev.out)
    assert ei.value.code == abi.LOB_ESTATE, "between lob_td_step_begin and lob_td_step_end"
    eng.td_step_end()
    assert_book_equals_dump(eng, dev, depth, "after lob_td_step_end")
    eng.td_step(2)
    d = assert_book_equals_dump(eng, dev, depth, "two steps later")
    assert (d["total_ticks"] == 5).all()
    dev.free()
    eng.close()


# ---- 8. stream order -------------------------------------------------------------------------------------------------------------------

def test_stream_order_without_synchronisation():
    """step, book -> set 1, step, book -> set 2, one lob_sync: set 1 is the dump a twin run takes after step 1, set 2 after step 2."""
    B, depth = 257, 10
    rng = np.random.default_rng(8)
    acts = [rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32) for _ in range(2)]
    vout = abi.VecOut(None, None, None, None, None)
    p, rec, twin = make_engine(B, depth, 2, 200)
    a = [DevBuf(B, np.int32), DevBuf(B, np.int32)]
    twin.reset()
    dumps = []
    for k in range(2):
        a[k].upload(acts[k])
        twin.vec_step(a[k].ptr, vout)
        dumps.append(expected(dumps_to_np(twin.get_books()), depth))
    twin.close()
    assert not np.array_equal(dumps[0]["time_ms"], dumps[1]["time_ms"]) and not np.array_equal(dumps[0]["levels"], dumps[1]["levels"])
    p, rec, eng = make_engine(B, depth, 2, 200)
    sets = [DevBook(B, depth), DevBook(B, depth)]
    eng.reset()
    for k in range(2):           # (the actions were uploaded above; nothing waits in here)
        eng.vec_step(a[k].ptr, vout)
        eng.vec_book(sets[k].out)
    eng.sync()
    for k in range(2):
        got = sets[k].read(eng)
        for name in NAMES:
            np.testing.assert_array_equal(got[name], dumps[k][name], err_msg="set %d: %s against the twin run's dump after step %d" % (k + 1, name, k + 1))
        sets[k].free()
        a[k].free()
    eng.close()


# ---- the torch face ----------------------------------------------------------------------------------------------------------------------

def test_vec_env_with_the_book_through_torch():
    """VecEnv(eng, book=True) at B = 300, depth 5: tests/vec_book_torch_child.py, in a fresh process of its own because torch must
    be imported before the engine library is loaded (one HIP runtime per process) and this process has loaded it."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vec_book_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "vec_book_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "vec book OK" in res.stdout
