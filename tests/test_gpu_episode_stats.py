"""lob_episode_stats: the batch's episode statistics reduced on the device, for the whole engine and per library day.

The yardstick is lob_get_books (+ lob_get_days) reduced with numpy here: every count, integer figure, extreme and the book that
holds it must be EXACT; an f64 sum must lie within n * 2^-53 * sum|x| of math.fsum, a sum of squares within
2n * 2^-53 * sum x^2 -- the worst-case bounds of any summation order (one more rounding per square), nothing tuned."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests.parity import dumps_to_np
from tests.test_episode_stats_abi import identity
from tests.test_gpu_days import make_days

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rl_markets_amd", "host", "lob_run")
EPS = 2.0 ** -53
DEPTH, TRADES = 5, 2


def params(algo=abi.ALGO_QLAMBDA, theta_mode=abi.THETA_SHARED, mem=1 << 20, first_book=0):
    p = engine.default_params()
    p.depth, p.max_trades = DEPTH, TRADES
    p.algo, p.theta_mode, p.memory_size = algo, theta_mode, mem
    p.book_id_offset = first_book
    assert p.epsilon == 0.8      # books differ: four actions in five are random
    return p


def synthetic(p, B, n_events, first_book=None):
    g = engine.default_gen_params()
    g.n_events = n_events
    eng = engine.Engine(p, B)
    eng.load_events(engine.gen_stream_host(g, DEPTH, TRADES, p.book_id_offset if first_book is None else first_book, B))
    return eng


def run_out(eng, cap=4000):
    for _ in range(cap):
        if eng.counters()[2] == 0:
            return
        eng.td_step(8)
    raise AssertionError("books still live after %d steps" % (8 * cap))


def quantities(books, ids):
    """Per quantity the values and the global ids of the books it counts, from the dumps."""
    tt = books["total_ticks"].astype(np.int64)
    made = tt > 0
    f = [(books["episode_reward"], ids), (books["episode_reward"][made] / tt[made].astype(np.float64), ids[made]),
         (books["episode_pnl"], ids), (books["episode_bandh"], ids)]
    mo = books["market_buys"].astype(np.int64) + books["market_sells"]
    i = [(tt, ids), (books["ask_transactions"].astype(np.int64) + books["bid_transactions"] + mo, ids), (mo, ids),
         (books["ticks_with_position"].astype(np.int64), ids)]
    return f, i


def check_record(rec, books, ids, group, tag):
    """One record against the numpy reduction of the dumps of its books (`ids` ascending: numpy's first extreme = lowest id)."""
    n = len(books)
    assert rec["group"] == group, tag
    term = books["terminal"]
    got = (int(rec["n_books"]), int(rec["n_live"]), int(rec["n_terminal"]), int(rec["n_out_of_data"]), int(rec["n_rho"]))
    assert got == (n, int((term == 0).sum()), int((term == 1).sum()), int((term == 2).sum()), int((books["total_ticks"] > 0).sum())), tag
    if n == 0:
        assert rec.tobytes() == identity(group).tobytes(), tag + ": an empty group is the identity record"
        return
    fq, iq = quantities(books, ids)
    for q, (x, xid) in enumerate(fq):
        s, t = rec["f"][q], "%s f[%d]" % (tag, q)
        if len(x) == 0:
            assert s.tobytes() == identity()["f"][q].tobytes(), t
            continue
        assert np.isfinite(x).all(), t
        ref, ref2 = math.fsum(x), math.fsum(x * x)
        bound, bound2 = len(x) * EPS * math.fsum(np.abs(x)), 2 * len(x) * EPS * ref2
        if abs(s["sum"] - ref) > bound or abs(s["sumsq"] - ref2) > bound2:
            print("%s: sum %r ref %r bound %g; sumsq %r ref %r bound %g" % (t, s["sum"], ref, bound, s["sumsq"], ref2, bound2))
        assert abs(s["sum"] - ref) <= bound, t + " sum"
        assert abs(s["sumsq"] - ref2) <= bound2, t + " sumsq"
        assert s["min"] == x.min() and s["argmin"] == xid[np.argmin(x)], t + " min"
        assert s["max"] == x.max() and s["argmax"] == xid[np.argmax(x)], t + " max"
    for q, (y, yid) in enumerate(iq):
        s, t = rec["i"][q], "%s i[%d]" % (tag, q)
        assert s["sum"] == y.sum() and s["sumsq"] == (y * y).sum(), t + " sums"
        assert s["min"] == y.min() and s["argmin"] == yid[np.argmin(y)], t + " min"
        assert s["max"] == y.max() and s["argmax"] == yid[np.argmax(y)], t + " max"


def check_engine(eng, tag, by_day=False):
    """Every record of eng.episode_stats(by_day) against the dumps; returns (records, dumps)."""
    st = eng.episode_stats(by_day)
    books = dumps_to_np(eng.get_books())
    ids = int(eng.params.book_id_offset) + np.arange(eng.B, dtype=np.int64)
    check_record(st[0], books, ids, -1, tag + " whole")
    if by_day:
        day = eng.days()
        n_days = len(eng.day_first) - 1
        assert len(st) == 1 + n_days
        for d in range(n_days):
            sel = day == d
            check_record(st[1 + d], books[sel], ids[sel], d, "%s day %d" % (tag, d))
        assert int(st["n_books"][1:].sum()) == eng.B, tag + ": every book is in one day group"
        check_merged(st[1:], st[0], tag + " merge of the day groups")
    else:
        assert len(st) == 1
    return st, books


def check_merged(parts, whole, tag):
    """merge(parts) against `whole`: integers, counts, extremes exact; the f64 sums within the bound (the orders differ)."""
    m = identity(int(parts[0]["group"]))
    for r in parts:
        m = engine.merge_episode_stats(m, r)
    assert m["group"] == -1 or len(set(parts["group"])) == 1
    for name in ("n_books", "n_live", "n_terminal", "n_out_of_data", "n_rho"):
        assert m[name] == whole[name], tag + " " + name
    assert m["i"].tobytes() == whole["i"].tobytes(), tag + " integer figures"
    for name in ("min", "max", "argmin", "argmax"):
        np.testing.assert_array_equal(m["f"][name], whole["f"][name], err_msg=tag + " " + name)
    # |x| <= max(|min|, |max|) for every book: n * that bounds sum|x|, n * that^2 bounds sum x^2
    n = int(whole["n_books"])
    big = np.maximum(np.abs(whole["f"]["min"]), np.abs(whole["f"]["max"]))
    assert (np.abs(m["f"]["sum"] - whole["f"]["sum"]) <= 2 * n * EPS * n * big).all(), tag + " sums"
    assert (np.abs(m["f"]["sumsq"] - whole["f"]["sumsq"]) <= 4 * n * EPS * n * big * big).all(), tag + " sums of squares"


# ---- 1. end of episode, one group; 3. reproducible ------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [abi.ALGO_QLAMBDA, abi.ALGO_SARSA, abi.ALGO_DOUBLE_Q], ids=["qlambda", "sarsa", "double_q"])
def test_end_of_episode_whole_batch(algo):
    B = 32768
    eng = synthetic(params(algo), B, 400)
    eng.reset()
    run_out(eng)
    eng.clear_inventory()
    st, books = check_engine(eng, "end of episode")
    r = st[0]
    assert r["n_live"] == 0 and r["n_terminal"] + r["n_out_of_data"] == B
    assert r["i"][abi.STATI_MARKET_ORDERS]["sum"] > 0 and len(set(books["episode_reward"])) > B // 2   # the books differ
    assert eng.episode_stats().tobytes() == st.tobytes()     # two calls in a row: the whole byte image
    eng.close()


# ---- 2. mid-episode snapshot, read-only; 3. two engines built alike -----------------------------------------------------------

@pytest.mark.parametrize("B,theta_mode", [(32768, abi.THETA_SHARED), (512, abi.THETA_PRIVATE)], ids=["shared_32768", "private_512"])
def test_mid_episode_snapshot_changes_nothing(B, theta_mode):
    """The call every 8th step on one engine and never on its twin: after 40 steps the dumps, the RNG counters, the flow and
    path statistics of the two are bit-equal, and so are the weights with a weight vector per book.  With ONE shared vector the
    update's f64 atomic additions land in an order the hardware decides ("agrees ... to the order of the atomic
    additions"), so two engines agree on theta to the last bits only, with this call or without: there the weights are held to
    the tolerance the suite uses for two shared-theta engines (tests/test_gpu_halfstep.py), everything else to bit equality."""
    mem = 1 << 20 if theta_mode == abi.THETA_SHARED else 1 << 14
    eng, twin = synthetic(params(theta_mode=theta_mode, mem=mem), B, 400), synthetic(params(theta_mode=theta_mode, mem=mem), B, 400)
    eng.reset()
    twin.reset()
    for step in range(1, 41):
        eng.td_step(1)
        twin.td_step(1)
        if step % 8 == 0:
            eng.episode_stats()
    st, books = check_engine(eng, "step 40")
    assert st[0]["n_live"] > 0
    tb = dumps_to_np(twin.get_books())
    assert books.tobytes() == tb.tobytes()
    if theta_mode == abi.THETA_PRIVATE:
        for b in (0, 1, B // 2, B - 1):
            np.testing.assert_array_equal(eng.theta(b), twin.theta(b))
    else:
        np.testing.assert_allclose(eng.theta(), twin.theta(), rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(eng.rng_counters(), twin.rng_counters())
    assert eng.flow_stats() == twin.flow_stats()
    np.testing.assert_array_equal(eng.path_stats(), twin.path_stats())
    assert twin.episode_stats().tobytes() == st.tobytes()     # two engines that ran the same run
    eng.close()
    twin.close()


# ---- 4. per day ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_days,B", [(1, 64), (7, 5000), (300, 2500)])
def test_per_day(n_days, B):
    assert B >= 4 * n_days
    rng = np.random.default_rng(n_days)
    days = make_days(rng.integers(300, 420, size=n_days))
    eng = engine.Engine(params(mem=1 << 16), B)
    eng.load_days(days)
    # every day has books by construction
    eng.days_select(abi.DAYS_IN_ORDER, 0, n_days)
    eng.reset()
    run_out(eng)
    eng.clear_inventory()
    st, _ = check_engine(eng, "in order", by_day=True)
    assert (st["n_books"][1:] >= 4).all() and st[0]["n_live"] == 0
    assert eng.episode_stats(True).tobytes() == st.tobytes()
    np.testing.assert_array_equal(eng.episode_stats(False), st[:1])     # record 0 does not depend on by_day
    # random draws from a part of the library: the days outside it are certainly empty
    first, n = (1, n_days - 3) if n_days >= 7 else (0, n_days)
    for ep in range(2):
        eng.handle_terminal()
        eng.days_select(abi.DAYS_RANDOM, first, n)
        eng.reset()
        eng.td_step(30 + 20 * ep)
        st, _ = check_engine(eng, "random draw %d" % ep, by_day=True)
        empty = np.flatnonzero(st["n_books"][1:] == 0)
        assert st[0]["n_live"] > 0
        if n_days >= 7:
            assert {0, n_days - 2, n_days - 1} <= set(empty.tolist())
        for d in empty:
            assert st[1 + d].tobytes() == identity(int(d)).tobytes()
    eng.close()


def test_errors():
    lib = abi.load()
    out = np.zeros(8, dtype=engine.EPISODE_STATS_DTYPE)
    n = C.c_int32(-7)
    ptr = out.ctypes.data_as(C.c_void_p)
    eng = synthetic(params(mem=1 << 16), 16, 300)
    assert lib.lob_episode_stats(eng.h, 0, ptr, 8, C.byref(n)) == abi.LOB_ESTATE     # before the first reset
    eng.reset()
    assert lib.lob_episode_stats(eng.h, 0, ptr, 8, None) == abi.LOB_EINVAL
    assert lib.lob_episode_stats(eng.h, 0, None, 8, C.byref(n)) == abi.LOB_EINVAL
    assert lib.lob_episode_stats(eng.h, 1, ptr, 8, C.byref(n)) == abi.LOB_ESTATE     # by_day without a library
    assert lib.lob_episode_stats(eng.h, 0, ptr, 0, C.byref(n)) == abi.LOB_EINVAL and n.value == 1
    assert lib.lob_episode_stats(eng.h, 0, ptr, 8, C.byref(n)) == abi.LOB_OK and n.value == 1
    eng.td_step_begin()
    assert lib.lob_episode_stats(eng.h, 0, ptr, 8, C.byref(n)) == abi.LOB_ESTATE     # a half-done learner step
    eng.td_step_end()
    assert lib.lob_episode_stats(eng.h, 0, ptr, 8, C.byref(n)) == abi.LOB_OK
    eng.load_days(make_days([300, 310, 320]))
    eng.days_select(abi.DAYS_IN_ORDER, 0, 3)
    assert lib.lob_episode_stats(eng.h, 1, ptr, 8, C.byref(n)) == abi.LOB_ESTATE     # no episode on the library yet
    eng.reset()
    n.value = 0
    assert lib.lob_episode_stats(eng.h, 1, ptr, 3, C.byref(n)) == abi.LOB_EINVAL and n.value == 4
    assert lib.lob_episode_stats(eng.h, 1, ptr, 4, C.byref(n)) == abi.LOB_OK and n.value == 4
    assert list(out["group"][:4]) == [-1, 0, 1, 2]
    eng.close()


# ---- 5. global ids and merging --------------------------------------------------------------------------------------------------

def test_two_shards_merge_to_the_single_engine():
    B, half = 256, 128
    whole = synthetic(params(theta_mode=abi.THETA_PRIVATE, mem=1 << 14), B, 360)
    shards = [synthetic(params(theta_mode=abi.THETA_PRIVATE, mem=1 << 14, first_book=k * half), half, 360) for k in range(2)]
    for e in [whole] + shards:
        e.reset()
        run_out(e)
        e.clear_inventory()
    sw, bw = check_engine(whole, "single engine")
    parts = []
    for k, e in enumerate(shards):
        s, bk = check_engine(e, "shard %d" % k)
        assert bk.tobytes() == bw[k * half:(k + 1) * half].tobytes()    # private theta: the books do not depend on the sharding
        parts.append(s[0])
    for name in ("argmin", "argmax"):     # global ids
        for kind in ("f", "i"):
            assert (parts[0][kind][name] < half).all() and (parts[1][kind][name] >= half).all()
    check_merged(np.array(parts), sw[0], "shards")
    assert (sw[0]["f"]["argmax"] >= half).any() or (sw[0]["f"]["argmin"] >= half).any()
    for e in [whole] + shards:
        e.close()


# ---- 6. small and odd batches ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 63, 65, 4096, 4097])
def test_small_and_odd_batches(B):
    eng = synthetic(params(mem=1 << 16), B, 330)
    eng.reset()
    st, _ = check_engine(eng, "after reset")          # no step made: nobody counts for rho
    assert st[0]["n_rho"] == 0 and st[0]["f"][abi.STATF_RHO].tobytes() == identity()["f"][abi.STATF_RHO].tobytes()
    eng.td_step(30)
    check_engine(eng, "step 30")
    run_out(eng)
    eng.clear_inventory()
    st, _ = check_engine(eng, "end")
    assert st[0]["n_live"] == 0 and st[0]["n_rho"] > 0
    eng.close()


# ---- 7. the driver ---------------------------------------------------------------------------------------------------------------

def test_lob_run_batch_log(tmp_path):
    from tests.test_gpu_days_driver import config, day_dirs
    md_dir, tas_dir, files = day_dirs(tmp_path, [700, 520, 860, 610, 750])
    cfg = config(tmp_path, "\nevaluation:\n    n_samples: 2\n")
    B, episodes = 6, 2
    log = tmp_path / "logs" / "batch.csv"
    log.parent.mkdir()
    cmd = [EXE, "-c", cfg, "-a", "q_learn", "-n", str(B), "-e", str(episodes), "--md-dir", md_dir, "--tas-dir", tas_dir]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(log.parent))
    assert plain.returncode == 0, plain.stderr
    assert os.listdir(str(log.parent)) == []               # without the flag: no file
    out = subprocess.run(cmd + ["--batch-log", str(log)], capture_output=True, text=True, timeout=600, cwd=str(log.parent))
    assert out.returncode == 0, out.stderr
    assert out.stdout == plain.stdout                      # and with it stdout is what it was
    assert os.listdir(str(log.parent)) == ["batch.csv"]
    rows = log.read_text().strip().splitlines()
    head = rows[0].split(",")
    assert head[:7] == ["episode", "group", "day_file", "n_books", "n_terminal", "n_out_of_data", "epsilon"]
    assert head[7:] == [q + "_" + s for q in ("reward", "rho", "pnl") for s in ("mean", "std", "min", "max")] + \
        [q + "_" + s for q in ("steps", "transactions") for s in ("mean", "min", "max")] + ["ppt"]
    recs = [dict(zip(head, r.split(","))) for r in rows[1:]]
    assert all(len(r.split(",")) == len(head) for r in rows[1:])

    # the same two training episodes on an Engine (lob_run's Agent: alpha 0.001, epsilon = float(eps_init) * 1 after episode 0)
    p = engine.default_params()
    p.algo = abi.ALGO_QLAMBDA
    eng = engine.Engine(p, B)
    eng.load_days([engine.convert_csv(md, tas) for md, tas in files])
    eps = float(np.float32(0.8))
    eng.set_epsilon(eps)
    n_rows = 0
    for ep in range(episodes):
        eng.days_select(abi.DAYS_RANDOM, 0, 3)
        eng.reset()
        run_out(eng)
        eng.clear_inventory()
        books, day = dumps_to_np(eng.get_books()), eng.days()
        mine = [r for r in recs if r["episode"] == str(ep + 1)]
        played = sorted(set(day.tolist()))
        n_rows += 1 + len(played)
        assert [int(r["group"]) for r in mine] == [-1] + played          # one row for the batch, one per day that had books
        assert mine[0]["day_file"] == "" and [r["day_file"] for r in mine[1:]] == [files[d][0] for d in played]
        for r in mine:
            sel = np.ones(B, bool) if r["group"] == "-1" else day == int(r["group"])
            b = books[sel]
            ids = np.arange(B)[sel]
            assert (int(r["n_books"]), int(r["n_terminal"]), int(r["n_out_of_data"])) == (len(b), int((b["terminal"] == 1).sum()), int((b["terminal"] == 2).sum()))
            # (the training row's epsilon column: the policy's descr() AFTER HandleTerminal(ep), serial.cpp:79-88)
            assert float(r["epsilon"]) == pytest.approx(eps * (float(np.float32(0.0001)) / eps) ** (ep / 800.0), rel=1e-5)
            fq, iq = quantities(b, ids)
            for name, (x, _) in zip(("reward", "rho", "pnl"), (fq[0], fq[1], fq[2])):
                assert float(r[name + "_mean"]) == pytest.approx(x.mean(), rel=1e-9, abs=1e-12), name
                assert float(r[name + "_min"]) == pytest.approx(x.min(), rel=1e-9, abs=1e-12), name
                assert float(r[name + "_max"]) == pytest.approx(x.max(), rel=1e-9, abs=1e-12), name
                # sqrt(sumsq / n - mean^2) loses what the subtraction cancels: of the order of 2^-53 * mean^2 / std^2, relative
                assert float(r[name + "_std"]) == pytest.approx(x.std(), rel=1e-6, abs=1e-6 * abs(x.mean())), name
            for name, (y, _) in zip(("steps", "transactions"), (iq[0], iq[1])):
                assert float(r[name + "_mean"]) == pytest.approx(y.mean(), rel=1e-9), name
                assert (int(r[name + "_min"]), int(r[name + "_max"])) == (y.min(), y.max()), name
            assert float(r["ppt"]) == pytest.approx(math.fsum(fq[2][0]) / iq[1][0].sum(), rel=1e-9, abs=1e-12)
        eng.handle_terminal()
        eng.set_alpha(0.001)
        eng.set_epsilon(eps * (float(np.float32(0.0001)) / eps) ** (ep / 800.0))
    eng.close()
    # the greedy round over the two held-out days: two books, a day each
    test = [r for r in recs if r["episode"] == "test1"]
    assert [int(r["group"]) for r in test] == [-1, 3, 4] and [r["n_books"] for r in test] == ["2", "1", "1"]
    assert [r["day_file"] for r in test[1:]] == [files[3][0], files[4][0]]
    assert len(recs) == n_rows + 3
    # the day rows of the test round are the stdout rows of those days
    for r, line in zip(test[1:], [l.split(",") for l in out.stdout.splitlines() if l.startswith("test,") and not l.startswith("test,episode")]):
        assert r["reward_mean"] == line[4] and r["rho_mean"] == line[5] and r["pnl_mean"] == line[6]
        assert r["transactions_min"] == line[7] and r["ppt"] == line[8] and r["reward_std"] == "0"
