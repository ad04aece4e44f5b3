"""lob_step_log_*: the profit-log row of every completed step, recorded on the device for a chosen set of books.

The yardsticks are the oracle (tests/oracle_lib.py), the reference's own Backtester rows (tests/golden/step_log/profit_rows_b0.npz,
written by tests/golden/make_profit_rows.py) and lob_get_books, which the rest of the suite pins to the oracle -- never the
log itself.  A row is compared as its 96 bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from rl_markets_amd.engine import STEP_ROW_DTYPE, LobError
from tests import oracle_lib as ol
from tests.parity import dumps_to_np
from tests.test_gpu_days import make_days

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rl_markets_amd", "host", "lob_run")
DEPTH, TRADES = 5, 2


def params(algo=abi.ALGO_QLAMBDA, theta_mode=abi.THETA_PRIVATE, mem=1 << 16, first_book=0):
    p = engine.default_params()
    p.depth, p.max_trades = DEPTH, TRADES
    p.algo, p.theta_mode, p.memory_size = algo, theta_mode, mem
    p.book_id_offset = first_book
    return p


def streams(p, B, n_events):
    g = engine.default_gen_params()
    g.n_events = n_events
    return engine.gen_stream_host(g, DEPTH, TRADES, p.book_id_offset, B)


def rows_of_books(books):
    """What a row holds, from book dumps (lob_get_books, or the oracle's rec(b)["book"]) taken right after the step."""
    books = np.atleast_1d(books)
    r = np.zeros(len(books), dtype=STEP_ROW_DTYPE)
    ap0, bp0 = books["ask_px"][:, 0].astype(np.float64), books["bid_px"][:, 0].astype(np.float64)
    r["time_ms"], r["position"] = books["time_ms"], books["position"]
    r["midprice"], r["spread"] = (ap0 + bp0) / 2.0, ap0 - bp0
    for dst, src in (("ask_quote", "ask_quote"), ("bid_quote", "bid_quote"), ("pnl_step", "pnl_step"), ("episode_pnl", "episode_pnl"),
                     ("episode_bandh", "episode_bandh"), ("episode_reward", "episode_reward"), ("step", "total_ticks"),
                     ("action", "last_action"), ("ask_level", "ask_level"), ("bid_level", "bid_level")):
        r[dst] = books[src]
    return r


class Expect:
    """The rows a sequence of single steps should have logged: after every step, a book whose total_ticks has moved and which
    is not out of data has completed a performAction (base.cpp:278 counts the tick, base.cpp:289-290 leaves on a dry stream)."""

    def __init__(self, books0):
        self.ticks = books0["total_ticks"].copy()
        self.rows = [[] for _ in range(len(books0))]

    def after_step(self, books):
        done = (books["total_ticks"] != self.ticks) & (books["terminal"] != 2)
        assert ((books["total_ticks"] - self.ticks)[done] == 1).all()
        self.ticks = books["total_ticks"].copy()
        if done.any():
            r = rows_of_books(books[done])
            for i, b in enumerate(np.flatnonzero(done)):
                self.rows[b].append(r[i])
        return done


def assert_log_equals(eng, sel, expect_rows, tag, cap=None):
    """The whole log of `eng` against the expected rows of the selected books (lists of rows per selected book)."""
    n_rows, n_lost = eng.step_log_counts()
    want_n = np.array([len(r) for r in expect_rows])
    stored = want_n if cap is None else np.minimum(want_n, cap)
    np.testing.assert_array_equal(n_rows, stored, err_msg=tag + ": stored rows")
    np.testing.assert_array_equal(n_lost, want_n - stored, err_msg=tag + ": lost rows")
    width = max(1, int(stored.max()) + 2) if cap is None else cap
    width = min(width, eng._slog_cap)
    got = eng.step_log_read(0, len(sel), 0, width)
    assert got.shape == (len(sel), width)
    for j in range(len(sel)):
        want = np.zeros(width, dtype=STEP_ROW_DTYPE)
        for k in range(min(int(stored[j]), width)):
            want[k] = expect_rows[j][k]
        if got[j].tobytes() != want.tobytes():
            k = next(k for k in range(width) if got[j][k].tobytes() != want[k].tobytes())
            raise AssertionError("%s: selected book %d (book %d) row %d:\n  log    %r\n  expect %r" % (tag, j, sel[j], k, got[j][k], want[k]))
    return n_rows


def oracle_books(orc, sel):
    return np.array([orc.rec(int(b))["book"] for b in sel], dtype=ol.BOOK_DTYPE)


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [abi.ALGO_SARSA, abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q], ids=["sarsa", "qlambda", "double_q"])
def test_rows_match_the_oracle_step_by_step(algo):
    """A training episode through lob_td_step(7), then a greedy one through lob_eval_step(5): 256 books, private theta, 20 books
    logged; the oracle is stepped one step at a time and every completed step of a logged book gives the expected row."""
    B, n_events = 256, 400
    p = params(algo)
    rec = streams(p, B, n_events)
    sel = np.unique(np.r_[0, 63, 64, 255, np.random.default_rng(5).choice(B, 16, replace=False)]).astype(np.int32)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    eng.step_log_enable(sel, 512)
    for episode, (step_e, step_o, n) in enumerate(((eng.td_step, orc.td_step, 7), (eng.eval_step, orc.eval_step, 5))):
        eng.reset()
        orc.reset()
        ex = Expect(oracle_books(orc, sel))
        calls = 0
        while True:
            step_e(n)
            for _ in range(n):
                step_o(1)
                ex.after_step(oracle_books(orc, sel))
            calls += 1
            assert calls < 400
            if eng.counters()[2] == 0:
                break
        tag = "episode %d (%s)" % (episode, "training" if episode == 0 else "greedy")
        n_rows = assert_log_equals(eng, sel, ex.rows, tag)
        assert n_rows.min() > 20, tag
        eng.clear_inventory()
        orc.clear_inventory()
        assert np.array_equal(eng.step_log_counts()[0], n_rows), "lob_clear_inventory logs nothing"
        eng.handle_terminal()
        orc.handle_terminal()
    eng.close()
    orc.close()


def test_rows_of_lob_step_match_the_oracle():
    """An episode driven by lob_step with random host actions (launch_env alone: the learner's kernels never run)."""
    B = 96
    p = params()
    rec = streams(p, B, 400)
    sel = np.arange(0, B, 5, dtype=np.int32)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    orc = ol.Oracle(p, rec)
    eng.step_log_enable(sel, 512)
    eng.reset()
    orc.reset()
    ex = Expect(oracle_books(orc, sel))
    rng = np.random.default_rng(17)
    for s in range(400):
        a = rng.integers(0, abi.LOB_N_ACTIONS, size=B).astype(np.int32)
        eng.step(a)
        orc.env_step(a)
        ex.after_step(oracle_books(orc, sel))
    n_rows = assert_log_equals(eng, sel, ex.rows, "lob_step")
    assert n_rows.min() > 20
    assert (dumps_to_np(eng.get_books())["terminal"] != 0).all(), "the episode has run to its end"
    eng.close()
    orc.close()


# ---- 2. against the reference itself --------------------------------------------------------------------------------------------

def test_backtest_rows_of_the_reference():
    """The rows the reference's own Backtester handed to profit_log (tests/golden/make_profit_rows.py), replayed on the engine:
    one training episode, then the greedy episode through lob_eval_step(6) with book 0 logged.  Everything but bandh_step is
    compared for equality; bandh_step, the difference of two consecutive episode_bandh here and a sum of its own in the
    reference, with the bound the CPU sweep uses for the same quantity (tests/test_oracle_ref_sweep.py): 1e-9 * max(1, |total|)."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "step_log", "profit_rows_b0.npz"))
    assert int(fx["abi_version"]) == abi.load().lob_abi_version()
    p, g = abi.Params(), engine.default_gen_params()
    assert fx["params"].nbytes == C.sizeof(p) and fx["gen"].nbytes == C.sizeof(g)
    C.memmove(C.byref(p), fx["params"].tobytes(), C.sizeof(p))
    C.memmove(C.byref(g), fx["gen"].tobytes(), C.sizeof(g))
    want = fx["rows"]
    rec = engine.gen_stream_host(g, 5, p.max_trades, p.book_id_offset, 1)
    eng = engine.Engine(p, 1)
    eng.load_events(rec)
    eng.reset()
    eng.td_step(int(fx["train_steps"]) + 2)
    eng.clear_inventory()
    eng.step_log_enable([0], len(want) + 8)
    eng.reset()
    for _ in range(len(want) // 6 + 2):
        eng.eval_step(6)
    assert eng.counters()[2] == 0
    n_rows, n_lost = eng.step_log_counts()
    assert n_rows[0] == len(want) > 50 and n_lost[0] == 0
    got = eng.step_log_read()[0]
    bandh = 0.0
    for i, (r, w) in enumerate(zip(got, want)):
        mine = (r["time_ms"], r["action"], r["position"], r["midprice"], r["spread"], r["ask_quote"], r["bid_quote"], r["ask_level"],
                r["bid_level"], r["pnl_step"])
        for k, name in enumerate(("time", "action", "position", "midprice", "spread", "quoted_ask", "quoted_bid", "ask_level",
                                  "bid_level", "pnl_step")):
            assert float(mine[k]) == w[1 + k], "row %d: %s %r != %r" % (i, name, mine[k], w[1 + k])
        step_move = r["episode_bandh"] - bandh
        bandh = r["episode_bandh"]
        assert abs(step_move - w[11]) <= 1e-9 * max(1.0, abs(bandh)), "row %d: bandh_step %r != %r" % (i, step_move, w[11])
        assert r["step"] == i + 1
    eng.close()


# ---- 3. batching and splitting ---------------------------------------------------------------------------------------------------

def test_batched_split_and_single_steps_log_the_same_rows():
    B, n = 512, 96
    p = params()
    rec = streams(p, B, 1200)
    logs = []
    for how in ("single", "batched", "halves"):
        eng = engine.Engine(p, B)
        eng.load_events(rec)
        eng.step_log_enable(None, n)
        eng.reset()
        if how == "single":
            for _ in range(n):
                eng.td_step(1)
        elif how == "batched":
            eng.td_step(n)
        else:
            assert eng.td_split_supported()
            for _ in range(n):
                eng.td_step_begin()
                eng.td_step_end()
        counts = eng.step_log_counts()
        logs.append((counts[0].tobytes(), counts[1].tobytes(), eng.step_log_read(0, B, 0, n).tobytes()))
        assert counts[0].max() == n
        eng.close()
    assert logs[0] == logs[1], "td_step(1) x n against td_step(n)"
    assert logs[0] == logs[2], "td_step(1) x n against begin / end x n"


# ---- 4. the log is an observer ---------------------------------------------------------------------------------------------------

def test_the_log_changes_nothing_and_costs_nothing_when_off():
    B, n = 512, 120
    p = params(abi.ALGO_DOUBLE_Q)
    rec = streams(p, B, 1200)
    seen = []
    for logged in (True, False):
        eng = engine.Engine(p, B)
        eng.load_events(rec)
        if logged:
            eng.step_log_enable(None, n)
        eng.kernel_timing(1)
        eng.reset()
        eng.td_step(n // 2)
        for _ in range(n // 4):
            eng.td_step_begin()
            eng.td_step_end()
        eng.eval_step(n // 4)
        eng.sync()
        _, launches = eng.kernel_time_ms("step_log_kernel")
        assert launches == (n if logged else 0)
        seen.append((bytes(eng.get_books()), eng.theta(0).tobytes(), eng.theta(B - 1).tobytes(), eng.theta(B).tobytes(),
                     np.asarray(eng.counters()).tobytes(), eng.rng_counters().tobytes()))
        if logged:
            assert eng.step_log_counts()[0].max() == n
        eng.close()
    for a, b, name in zip(seen[0], seen[1], ("lob_get_books", "theta of book 0", "theta of the last book", "theta_b of book 0",
                                             "lob_get_counters", "lob_get_rng_counters")):
        assert a == b, name


# ---- 5. tail, capacity and the dry stream ---------------------------------------------------------------------------------------

def day_into_the_close(p, n_events, before_close, book_id):
    """A synthetic day whose last `before_close` events lie before the session's close: its books end with terminal == 1."""
    g = engine.default_gen_params()
    g.n_events = n_events
    g.t0_ms = int(p.market.close_ms - 30 * 60000 - before_close * g.dt_ms)
    return engine.gen_stream_host(g, DEPTH, TRADES, book_id, 1)[0]


def test_tail_capacity_and_dry_streams():
    """Days of clearly different lengths, every book logged.  The synthetic days end mid-session: their books run out of data
    (terminal == 2) and the step that found the stream dry has counted its tick without a row; one more day runs into the close."""
    B = 384
    p = params()
    days = make_days([300, 520, 900]) + [day_into_the_close(p, 700, 450, 2000)]
    eng = engine.Engine(p, B)
    eng.load_days(days)
    cap_all = 1024
    shortest = None
    for cap in (cap_all, None):
        if cap is None:
            cap = shortest // 2     # below the shortest day's steps
            assert cap >= 8
        eng.step_log_enable(None, cap)
        eng.days_set((np.arange(B) % len(days)).astype(np.int32))
        eng.reset()
        calls = 0
        while True:
            eng.td_step(16)
            calls += 1
            assert calls < 400
            if eng.counters()[2] == 0:
                break
        eng.td_step(3)              # every book is over: nothing more is logged
        books = dumps_to_np(eng.get_books())
        n_rows, n_lost = eng.step_log_counts()
        dry = books["terminal"] == 2
        print("cap %d: rows %d..%d, lost %d..%d, terminal==2: %d, terminal==1: %d" % (cap, n_rows.min(), n_rows.max(), n_lost.min(),
                                                                                    n_lost.max(), dry.sum(), (books["terminal"] == 1).sum()))
        assert dry.any(), "some books ran out of data"
        assert (books["terminal"] != 0).all()
        np.testing.assert_array_equal(n_rows + n_lost, books["total_ticks"] - dry.astype(np.int32))
        if cap == cap_all:
            assert (n_lost == 0).all()
            assert n_rows.min() < n_rows.max(), "only some books step in the tail of the episode"
            assert n_rows.min() > 16
            shortest = int(n_rows.min())
            width = int(n_rows.max()) + 3
        else:
            assert (n_rows == cap).all() and (n_lost > 0).all()
            width = cap
        got = eng.step_log_read(0, B, 0, width)
        k = np.arange(width)[None, :]
        beyond = k >= n_rows[:, None]
        assert (got["step"][~beyond] == (np.broadcast_to(k, got.shape) + 1)[~beyond]).all(), "row k is the book's k-th step"
        flat = got.view(np.uint8).reshape(B, width, STEP_ROW_DTYPE.itemsize)
        assert not flat[beyond].any(), "slots beyond a book's count are zero bytes"
        # the last stored row of a book that lost none is its final state before lob_clear_inventory
        if cap == cap_all:
            last = got[np.arange(B), n_rows - 1]
            fin = rows_of_books(books)
            live_end = ~dry
            assert last[live_end].tobytes() == fin[live_end].tobytes()
        # a window of the log: books 7.., rows 5..
        part = eng.step_log_read(7, 9, 5, 6)
        assert part.tobytes() == np.ascontiguousarray(got[7:16, 5:11]).tobytes()
    eng.close()


# ---- 6. at scale -----------------------------------------------------------------------------------------------------------------

def test_all_books_of_the_headline_batch():
    """65 536 books, all logged, 40 steps in one call, against lob_get_books of a second engine stepped one step at a time.
    Shared weights with alpha = 0: the weights stay where they are, so two engines run the same run bit for bit."""
    B, n = 65536, 40
    p = params(theta_mode=abi.THETA_SHARED, mem=1 << 20)
    p.alpha = 0.0
    g = engine.default_gen_params()
    g.n_events = 400
    a, b = engine.Engine(p, B), engine.Engine(p, B)
    for e in (a, b):
        e.gen_events(g)
    a.step_log_enable(None, n)
    a.reset()
    a.td_step(n)
    b.reset()
    ex_ticks = dumps_to_np(b.get_books())["total_ticks"].copy()
    k_of = np.zeros(B, dtype=np.int64)
    want = np.zeros((B, n), dtype=STEP_ROW_DTYPE)
    for s in range(n):
        b.td_step(1)
        books = dumps_to_np(b.get_books())
        done = (books["total_ticks"] != ex_ticks) & (books["terminal"] != 2)
        np.testing.assert_array_equal(done, b.stepped().astype(bool) & (books["terminal"] != 2))
        ex_ticks = books["total_ticks"].copy()
        idx = np.flatnonzero(done)
        want[idx, k_of[idx]] = rows_of_books(books[idx])
        k_of[idx] += 1
    n_rows, n_lost = a.step_log_counts()
    np.testing.assert_array_equal(n_rows, k_of)
    assert (n_lost == 0).all() and (k_of == n).sum() > B // 2
    got = a.step_log_read(0, B, 0, n)
    assert got.tobytes() == want.tobytes()
    a.close()
    b.close()


# ---- 7. life cycle and errors ----------------------------------------------------------------------------------------------------

def code_of(fn, *args):
    with pytest.raises(LobError) as ei:
        fn(*args)
    return ei.value.code


def test_life_cycle_and_errors():
    B = 64
    p = params()
    eng = engine.Engine(p, B)
    eng.load_events(streams(p, B, 400))
    assert code_of(eng.step_log_counts) == abi.LOB_ESTATE, "the log is off"
    eng.reset()
    eng.td_step(5)
    eng.step_log_enable([3, 9, 40], 32)
    eng.td_step(5)                       # mid-episode: nothing is recorded before the next reset
    n_rows, n_lost = eng.step_log_counts()
    assert not n_rows.any() and not n_lost.any()
    assert not eng.step_log_read(0, 3, 0, 32).view(np.uint8).any()
    eng.reset()
    eng.td_step(6)
    assert (eng.step_log_counts()[0] == 6).all()
    first = eng.step_log_read(0, 3, 0, 6)
    assert (first["step"] == np.arange(1, 7)).all()
    eng.reset()                          # a second reset empties the log
    assert not eng.step_log_counts()[0].any() and not eng.step_log_read(0, 3, 0, 32).view(np.uint8).any()
    eng.td_step(2)
    assert (eng.step_log_counts()[0] == 2).all()
    # ranges
    assert code_of(eng.step_log_read, 0, 4, 0, 1) == abi.LOB_EINVAL
    assert code_of(eng.step_log_read, 2, 2, 0, 1) == abi.LOB_EINVAL
    assert code_of(eng.step_log_read, 0, 1, 30, 3) == abi.LOB_EINVAL
    assert code_of(eng.step_log_read, 0, 1, 0, 33) == abi.LOB_EINVAL
    assert code_of(eng.step_log_read, -1, 1, 0, 1) == abi.LOB_EINVAL
    assert eng.lib.lob_step_log_read(eng.h, 0, 1, 0, 1, None) == abi.LOB_EINVAL
    assert eng.lib.lob_step_log_counts(eng.h, None, None) == abi.LOB_EINVAL
    # bad lists leave the log as it was
    for bad in ([5, 3], [3, 3], [0, B], [-1, 2]):
        assert code_of(eng.step_log_enable, bad, 8) == abi.LOB_EINVAL, bad
    assert code_of(eng.step_log_enable, [1], 0) == abi.LOB_EINVAL
    assert eng.lib.lob_step_log_enable(eng.h, None, B - 1, 8) == abi.LOB_EINVAL, "NULL selects every book: n_sel == n_books"
    assert (eng.step_log_counts()[0] == 2).all()
    # inside a half step
    eng.td_step_begin()
    assert code_of(eng.step_log_enable, [1], 8) == abi.LOB_ESTATE
    assert code_of(eng.step_log_counts) == abi.LOB_ESTATE
    assert code_of(eng.step_log_read, 0, 1, 0, 1) == abi.LOB_ESTATE
    eng.td_step_end()
    assert (eng.step_log_counts()[0] == 3).all(), "the end half writes the row"
    # off
    eng.step_log_enable([], 1)
    assert code_of(eng.step_log_read, 0, 1, 0, 1) == abi.LOB_ESTATE
    assert code_of(eng.step_log_counts) == abi.LOB_ESTATE
    eng.td_step(3)
    # more than the device holds
    assert eng.lib.lob_step_log_enable(eng.h, None, B, 2 ** 31 - 1) == abi.LOB_ENOMEM
    eng.td_step(1)
    eng.close()


# ---- 8. lob_run --------------------------------------------------------------------------------------------------------------------

def test_lob_run_profit_log_books(tmp_path):
    one, many = str(tmp_path / "one.csv"), str(tmp_path / "many.csv")
    base = [EXE, "-c", os.path.join(ROOT, "config", "engine.yaml"), "-a", "sarsa", "-n", "4", "-e", "1", "--events", "400"]
    out = subprocess.run(base + ["--profit-log", one], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run(base + ["--profit-log", many, "--profit-log-books", "0:3"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    files = [many + ".%d" % b for b in range(3)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(many) and not os.path.exists(many + ".3")
    texts = [open(f).read() for f in files]
    assert texts[0] == open(one).read()
    header = "episode,step,action,position,midprice,spread,quoted_ask,quoted_bid,ask_level,bid_level,pnl_step,bandh_step"
    for t in texts:
        lines = t.strip().splitlines()
        assert lines[0] == header and len(lines) > 50
    assert texts[0] != texts[1] and texts[1] != texts[2], "the books play different streams"
