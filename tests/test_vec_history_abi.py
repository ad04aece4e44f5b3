"""lob_vec_history on the host side: the header's struct and constants against the ctypes mirror, the export, the refusal of a NULL
engine, the raw wrapper's independence of torch, the numpy statement of the contract that the GPU tests compare with
(tests/vec_history_expected.py) on hand-made records, and -- on the oracle -- the fact the GPU tests pin `rec` with: wherever
terminal != 2 the record cursor - 1 of the book's stream holds exactly the levels of the dump.  CPU only -- no compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import oracle_lib as ol
from tests.vec_history_expected import NAMES, assert_record_has_dump_levels, expected_history

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")


def probe(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %d %d\\n",sizeof(lob_vec_hist_out),offsetof(lob_vec_hist_out,levels),'
                   'offsetof(lob_vec_hist_out,trades),offsetof(lob_vec_hist_out,time_ms),offsetof(lob_vec_hist_out,n_valid),'
                   'offsetof(lob_vec_hist_out,rec),LOB_MAX_HISTORY,LOB_ABI_VERSION);return 0;}')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return list(map(int, subprocess.check_output([str(exe)]).split()))


def test_header_layout_and_its_ctypes_mirror(tmp_path):
    got = probe(tmp_path)
    assert got == [40, 0, 8, 16, 24, 32, 128, 6], "sizeof, the five offsets, LOB_MAX_HISTORY, LOB_ABI_VERSION"
    V = abi.VecHistOut
    assert C.sizeof(V) == got[0] and tuple(getattr(V, n).offset for n in NAMES) == tuple(got[1:6])
    assert [f[0] for f in V._fields_] == list(NAMES) and all(f[1] is C.c_void_p for f in V._fields_)
    assert abi.MAX_HISTORY == got[6] and abi.load().lob_abi_version() == got[7]


def test_symbol_is_exported_declared_and_in_the_header():
    lib = abi.load()
    assert hasattr(lib, "lob_vec_history") and "lob_vec_history" in lib._declared
    assert lib.lob_vec_history.argtypes[1] is C.c_int32 and lib.lob_vec_history.argtypes[2] is C.POINTER(abi.VecHistOut)
    assert lib.lob_vec_history.restype is C.c_int
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+lob_vec_history\s*\(\s*lob_engine\s*\*\s*e\s*,\s*int32_t\s+K\s*,\s*const\s+lob_vec_hist_out\s*\*\s*out\s*\)\s*;", src)


def test_null_engine_is_refused_with_a_message():
    lib = abi.load()
    lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))   # (a call that succeeds: the message below is this refusal's)
    out = abi.VecHistOut(None, None, None, None, None)
    assert lib.lob_vec_history(None, 8, C.byref(out)) == abi.LOB_EINVAL
    msg = lib.lob_last_error()
    assert msg and b"lob_vec_history" in msg


def test_engine_wrapper_exists_without_torch():
    code = ("import sys\nfrom rl_markets_amd import engine, abi\nassert callable(engine.Engine.vec_history)\n"
            "assert abi.VecHistOut is not None and abi.MAX_HISTORY == 128\nassert 'torch' not in sys.modules, 'rl_markets_amd.engine imported torch'\nprint('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


# ---- the expected-history helper, on hand-made records -----------------------------------------------------------------------------

def hand_made(n, D, T, salt):
    """n ABI records whose every word names itself: time 1000 * salt + e, ask_px[l] = salt + e + l / 16, ask_vol[l] = 100 e + l,
    bid_px[l] = -(that), bid_vol[l] = 16777217 + e (a volume that f32 cannot hold) at level 0, trade prices and volumes likewise."""
    r = np.full((n, abi.load().lob_record_words(D, T)), 0xABABABAB, np.uint32)   # (the padding words: never in the output)
    e = np.arange(n)
    r[:, 0] = 1000 * salt + e
    r[:, 1] = 0xDEAD                       # (flags: never in the output)
    lv = np.arange(D)
    apx = (salt + e[:, None] + lv[None, :] / 16.0).astype(np.float32)
    r[:, 2:2 + D] = apx.view(np.uint32)
    r[:, 2 + D:2 + 2 * D] = (100 * e[:, None] + lv[None, :]).astype(np.int32).view(np.uint32)
    r[:, 2 + 2 * D:2 + 3 * D] = (-apx).view(np.uint32)
    bv = (7 * e[:, None] + lv[None, :]).astype(np.int32)
    bv[:, 0] = 16777217 + e
    r[:, 2 + 3 * D:2 + 4 * D] = bv.view(np.uint32)
    tr = np.arange(T)
    r[:, 2 + 4 * D:2 + 4 * D + T] = (0.5 + salt + e[:, None] + tr[None, :]).astype(np.float32).view(np.uint32)
    r[:, 2 + 4 * D + T:2 + 4 * D + 2 * T] = (e[:, None] * 3 + tr[None, :]).astype(np.int32).view(np.uint32)
    return r


def test_expected_history_on_hand_made_records():
    D, T, K = 3, 2, 4
    # three streams back to back: lengths 6, 2, 5 (the second shorter than K)
    flat = np.concatenate([hand_made(6, D, T, 10), hand_made(2, D, T, 20), hand_made(5, D, T, 30)])
    start, length = np.array([0, 6, 8]), np.array([6, 2, 5])
    rec = np.array([5, 1, -1])             # a full window, r < K - 1, no snapshot
    x = expected_history(flat, start, length, rec, K, D, T)
    assert x["levels"].shape == (3, K, 4, D) and x["levels"].dtype == np.float32 and x["trades"].shape == (3, K, 2, T) and x["trades"].dtype == np.float32
    assert x["time_ms"].shape == (3, K) and x["time_ms"].dtype == np.int32 and x["n_valid"].dtype == np.int32 and x["rec"].dtype == np.int32
    np.testing.assert_array_equal(x["n_valid"], [4, 2, 0])
    np.testing.assert_array_equal(x["rec"], [5, 1, -1])
    # book 0: records 2, 3, 4, 5 of its stream, oldest first
    np.testing.assert_array_equal(x["time_ms"][0], [10002, 10003, 10004, 10005])
    np.testing.assert_array_equal(x["levels"][0, 3, 0], np.float32([15.0, 15.0625, 15.125]))
    np.testing.assert_array_equal(x["levels"][0, 0, 1], np.float32([200, 201, 202]))
    np.testing.assert_array_equal(x["levels"][0, 3, 2], -np.float32([15.0, 15.0625, 15.125]))
    assert x["levels"][0, 3, 3, 0] == np.float32(16777222) and np.float32(16777222) == 16777222, "16777217 + 5 rounds to the even neighbour"
    assert x["levels"][0, 2, 3, 0] == np.float32(16777220), "16777221 is a tie: round to nearest EVEN"
    np.testing.assert_array_equal(x["trades"][0, 3], np.float32([[15.5, 16.5], [15, 16]]))
    # book 1: r = 1 < K - 1: two leading zero slots, never book 0's last records
    np.testing.assert_array_equal(x["time_ms"][1], [0, 0, 20000, 20001])
    assert not x["levels"][1, :2].any() and not x["trades"][1, :2].any()
    np.testing.assert_array_equal(x["levels"][1, 2, 0], np.float32([20.0, 20.0625, 20.125]))
    np.testing.assert_array_equal(x["trades"][1, 3, 1], np.float32([3, 4]))
    # book 2: no snapshot: everything zero
    assert not x["levels"][2].any() and not x["trades"][2].any() and not x["time_ms"][2].any()
    # K = 1 is the current record; K beyond every stream is fine
    x1 = expected_history(flat, start, length, rec, 1, D, T)
    np.testing.assert_array_equal(x1["levels"][:, 0], x["levels"][:, K - 1])
    np.testing.assert_array_equal(x1["n_valid"], [1, 1, 0])
    x9 = expected_history(flat, start, length, rec, 9, D, T)
    np.testing.assert_array_equal(x9["n_valid"], [6, 2, 0])
    np.testing.assert_array_equal(x9["time_ms"][0], [0, 0, 0, 10000, 10001, 10002, 10003, 10004, 10005])
    np.testing.assert_array_equal(x9["levels"][:, 5:], x["levels"])
    # a replayed stream: one flat stream, three phases; the slots before a phase are zeros although records lie there
    xs = expected_history(flat, np.array([4, 8, 3]), 5, np.array([1, 0, 4]), K, D, T)
    np.testing.assert_array_equal(xs["time_ms"], [[0, 0, 10004, 10005], [0, 0, 0, 30000], [10004, 10005, 20000, 20001]])
    with pytest.raises(AssertionError):
        expected_history(flat, start, length, np.array([6, 1, -1]), K, D, T)   # rec beyond the book's stream


# ---- the fact behind the GPU tests' pin of `rec` -------------------------------------------------------------------------------------

@pytest.mark.parametrize("ending", ["dry", "session"])
@pytest.mark.parametrize("depth,trades,B", [(5, 2, 9), (10, 8, 5), (1, 1, 4)])
def test_record_before_the_cursor_holds_the_dumps_levels_on_the_oracle(depth, trades, B, ending):
    """Random actions on the oracle until no book is live (the streams of tests/test_gpu_vec_env.py gen(): "dry" ends with
    terminal 2, "session" with terminal 1): after the reset and after every step, for every book whose terminal != 2, record
    cursor - 1 of the host stream has exactly the dump's level prices and volumes.  (At terminal == 2 it need not -- the cursor
    stops short of the stream's last record while the snapshot has moved on --, so there the GPU tests pin `rec` by level equality
    alone.)  Also what the GPU test relies on for its counts: most (book, step) pairs are at terminal != 2, the window starts
    short of K = 64 and ends beyond K = 128 records."""
    p = engine.default_params()
    p.depth, p.max_trades = depth, trades
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_PRIVATE, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 150 if ending == "dry" else 300
    if ending == "session":
        g.t0_ms = int(p.market.close_ms - 30 * 60000 - 150 * g.dt_ms)
    rec = engine.gen_stream_host(g, depth, trades, 0, B)
    flat, start = rec.reshape(-1, rec.shape[-1]), np.arange(B) * g.n_events
    orc = ol.Oracle(p, rec)
    orc.reset()
    rng = np.random.default_rng(11)
    pairs = strong = step = 0
    lo, hi = 1 << 30, -1
    while True:
        d = orc.recs()["book"]
        cur, term = d["cursor"].astype(np.int64), d["terminal"]
        n = assert_record_has_dump_levels(flat, start, cur - 1, d, depth, "%s step %d" % (ending, step), books=term != 2)
        assert n == int((term != 2).sum()), "every such book has a snapshot"
        pairs, strong = pairs + B, strong + n
        if step % 10 == 0 and (term != 2).all():
            # the helper on these records: the newest slot is the dump, the slot before it the record before
            for K in (1, 7, 128):
                x = expected_history(flat, start, g.n_events, cur - 1, K, depth, trades)
                lv = np.stack([d["ask_px"][:, :depth], d["ask_vol"][:, :depth], d["bid_px"][:, :depth], d["bid_vol"][:, :depth]], axis=1)
                np.testing.assert_array_equal(x["levels"][:, K - 1], lv.astype(np.float32))
                np.testing.assert_array_equal(x["time_ms"][:, K - 1], rec[np.arange(B), cur - 1, 0].view(np.int32))
                np.testing.assert_array_equal(x["n_valid"], np.minimum(K, cur))
                if K > 1:
                    np.testing.assert_array_equal(x["trades"][:, K - 2, 0], rec[np.arange(B), cur - 2, 2 + 4 * depth:2 + 4 * depth + trades].view(np.float32))
        lo, hi = min(lo, int(cur.min()) - 1), max(hi, int(cur.max()) - 1)
        if not (term == 0).any():
            break
        orc.env_step(rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32))
        step += 1
        assert step < g.n_events
    assert (term == (2 if ending == "dry" else 1)).all()
    assert 2 * strong >= pairs and lo + 1 < 64 and hi + 1 >= 128, (strong, pairs, lo, hi)
    orc.close()
