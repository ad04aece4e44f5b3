"""tests/hard_streams.py on the CPU: the mutator is deterministic and makes valid streams; the batch the GPU tests run
(tests/test_gpu_hard_streams.py) really contains every pathology in rows the books consume; and the oracle -- the yardstick of
those GPU tests -- agrees with the UNMODIFIED reference on hardened streams step for step (where oracle/_ref is built)."""
import ctypes as C
import os

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import hard_streams as hs
from tests import oracle_lib as ol


def validate(rec, D, T):
    lib = abi.load()
    rc = lib.lob_validate_stream(rec.ctypes.data_as(C.c_void_p), D, T, rec.shape[0], rec.shape[1])
    return rc, (lib.lob_last_error() if rc else b"")


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("D", [3, 5, 10])
def test_harden_is_deterministic_and_valid(D, T):
    g = engine.default_gen_params()
    g.n_events = 300
    g.trade2_prob_q16 = 40000
    plain = engine.gen_stream_host(g, D, T, 0, 12)
    a, ca = hs.harden(plain, D, T, 7, dry=True)
    b, cb = hs.harden(plain, D, T, 7, dry=True)
    assert a.shape == plain.shape and a.dtype == np.uint32
    assert np.array_equal(a, b) and ca == cb
    assert validate(a, D, T) == (0, b"")
    for k in hs.KINDS + ("dry",):
        assert ca[k] > 0, (k, ca)
    # a book's stream depends on (seed, book) alone: not on the batch it is hardened in
    c, _ = hs.harden(plain[5:9], D, T, 7, dry=True, book0=5)
    assert np.array_equal(c, a[5:9])
    d, _ = hs.harden(plain, D, T, 8, dry=True)
    assert not np.array_equal(d, a)
    # each kind alone, and none at all
    for k in hs.KINDS:
        one, c1 = hs.harden(plain, D, T, 7, kinds=(k,))
        assert validate(one, D, T) == (0, b"") and c1[k] > 0 and sum(c1[q] for q in hs.KINDS + ("dry",)) == c1[k], (k, c1)
    none, c0 = hs.harden(plain, D, T, 7, kinds=())
    assert np.array_equal(none, plain) and sum(c0.values()) == 0
    # what the kinds promise
    f = a.view(np.float32)
    same = a[:, 1:, 0] == a[:, :-1, 0]
    assert (((a[:, :-1, 1] & abi.EVT_FLAG_SAME_TIME) != 0) == same).all()          # flagged as lob_convert_csv flags
    assert not (a[:, -1, 1] & abi.EVT_FLAG_SAME_TIME).any()
    assert (a[:, 1:][same][:, 2 + 4 * D + T:2 + 4 * D + 2 * T] == 0).all()         # a same-timestamp row carries no trades
    dryf = (a[:, :, 1] & abi.EVT_FLAG_TAS_DRY) != 0
    assert (dryf[:, 1:] >= dryf[:, :-1]).all() and not dryf[:, 0].any()            # only ever a tail
    crossed = f[:, :, 2] < f[:, :, 2 + 2 * D]
    assert crossed[:, 1:40].any() and crossed[:, -2].any()                         # inside the warm-up, next to the last row
    grid = np.rint(f[:, :, 2:2 + D].astype(np.float64) * 10.0) / 10.0
    assert (f[:, :, 2:2 + D] != grid.astype(np.float32)).any()                     # prices with other bits than the grid's


def _params():
    p = engine.default_params()
    p.depth, p.max_trades = hs.DEPTH, hs.TRADES
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_SHARED, 1 << 20
    return p


def _play(rec, alpha=None, episodes=2, steps=60):
    """The oracle over the GPU tests' schedule -> (positions [steps, B], final cursors)."""
    p = _params()
    if alpha is not None:
        p.alpha = alpha
    o = ol.Oracle(p, rec)
    pos = []
    for ep in range(episodes):
        o.reset()
        for s in range(steps):
            o.td_step(1)
            pos.append(o.recs()["book"]["position"].copy())
        o.clear_inventory()
        o.handle_terminal()
    cur = o.recs()["book"]["cursor"].copy()
    o.close()
    return np.array(pos), cur


def test_the_gpu_batch_contains_what_it_is_for():
    """Every kind's count is positive; same_time, crossed and deep_trades rows lie below some book's final cursor (the steps
    consumed them); off_grid and jumps change some book's positions against the plain stream (alpha = 0: the books do not
    interact, so a change is the book's own stream's doing)."""
    rec, counts, rows = hs.batch("all")
    assert validate(rec, hs.DEPTH, hs.TRADES) == (0, b"")
    for k in hs.KINDS:
        assert counts[k] > 0, counts
    assert hs.batch("all+dry")[1]["dry"] > 0
    _, cur = _play(rec)
    consumed = np.arange(hs.N_EVENTS)[None, :] < cur[:, None]
    seen = {k: int((rows[k] & consumed).any(axis=1).sum()) for k in hs.KINDS}
    # multi-row events below the cursors: runs of rows that do not end an event (crossed, or the next row has the same time)
    f = rec.view(np.float32)
    cont = (f[:, :, 2] < f[:, :, 2 + 2 * hs.DEPTH]) | (np.concatenate([rec[:, 1:, 0] == rec[:, :-1, 0], np.zeros((hs.B, 1), bool)], axis=1))
    cont &= consumed
    n_multi = int((cont[:, 1:] & ~cont[:, :-1]).sum() + cont[:, 0].sum())
    print("cases per kind", counts, "books that consumed one", seen, "multi-row events consumed", n_multi)
    for k in ("same_time", "crossed", "deep_trades"):
        assert seen[k] >= hs.B // 2, (k, seen)
    # the masks say what the final records hold: a deep-trade row carries exactly one trade
    tv = rec[:, :, 2 + 4 * hs.DEPTH + hs.TRADES:2 + 4 * hs.DEPTH + 2 * hs.TRADES]
    assert ((tv[rows["deep_trades"]] > 0).sum(axis=1) == 1).all() and counts["deep_trades"] == int(rows["deep_trades"].sum())
    # trade lists merged from several rows, and those that reach exactly max_trades keys that way, below the cursors; how
    # often the mutator had to drop a trade to stay inside what lob_validate_stream checks
    full = int((rows["merged_full"] & consumed).sum())
    print("merged lists", counts["merged"], "of exactly T keys", counts["merged_full"], "consumed", full, "trades dropped", counts["trimmed"])
    # (a condition on the inputs: at least every second crossed run leaves a merged list, one book in two consumes a full one)
    assert counts["merged"] >= counts["crossed"] // 2 and full >= hs.B // 2, (counts, full)
    n_trades = int((tv > 0).sum())
    assert counts["trimmed"] < n_trades // 20, (counts["trimmed"], n_trades)
    assert n_multi >= 1000, n_multi
    # three-row events with a crossed middle row, and lanes of one wave in different states: at some row, one wave of 64 books
    # holds a crossed row, a same-timestamp row and a row past a dry tail
    mid = rows["crossed"][:, 1:-1] & cont[:, :-2] & consumed[:, 2:]
    assert mid.any()
    dry_rows = hs.batch("all+dry")[2]["dry"]
    mixed = 0
    for w in range(0, hs.B, 64):
        mixed += int((rows["crossed"][w:w + 64].any(axis=0) & rows["same_time"][w:w + 64].any(axis=0) & dry_rows[w:w + 64].any(axis=0))[:150].sum())
    assert mixed > 0
    plain_pos, _ = _play(hs.plain_batch(), alpha=0.0, episodes=1)
    for k in ("off_grid", "jumps"):
        pos, _ = _play(hs.batch(k)[0], alpha=0.0, episodes=1)
        changed = int((pos != plain_pos).any(axis=0).sum())
        print(k, "changes the positions of", changed, "books")
        assert changed >= 1, k


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref/ref_harness not built (needs the reference checkout)")
@pytest.mark.parametrize("seed", range(max(1, int(os.environ.get("LOB_REF_SWEEP", "200")) // 4)))
def test_oracle_against_the_reference_on_hardened_streams(seed):
    """One-book D = 5 streams with every kind but `dry` (the harness writes its own time-and-sales sentinels: a dry file is
    pinned by tests/test_convert_ref_sweep.py), T in {1, 2}, SARSA and Q-learning alternating: trajectory, final step count and
    the sparse weight vector, as tests/test_oracle_ref_sweep.py compares them; every fourth case over two episodes."""
    from tests.test_oracle_golden import _params_for, compare_traj, replay_multi
    from tests.test_oracle_ref_sweep import check_sparse, ref_or_failed_init
    r = np.random.default_rng(333000 + seed)
    T = 1 + seed % 2
    algo = "sarsa" if (seed // 2) % 2 else "q_learn"
    book = int(r.integers(0, 1000))
    g = engine.default_gen_params()
    g.seed = int(r.integers(0, 1 << 40))
    g.n_events = int(r.choice([200, 260, 400]))
    g.move_prob_q16 = int(r.uniform(0.1, 1.0) * 65536)
    g.trade2_prob_q16 = int(r.uniform(0.0, 0.8) * 65536) if T > 1 else 0
    g.vol_min, g.vol_max = 1, int(r.choice([50, 5000]))
    g.trade_min, g.trade_max = 1, int(r.choice([20, 3000]))
    plain = engine.gen_stream_host(g, 5, T, book, 1)
    rec, counts = hs.harden(plain, 5, T, 444000 + seed)
    assert validate(rec, 5, T) == (0, b"")
    p = _params_for({}, algo, book)
    p.max_trades, p.memory_size = T, 1 << 18
    x = {}
    multi = seed % 4 == 3
    if multi:
        x["episodes"] = 2
        if seed % 8 == 3:
            x["steps"] = 40
    tag = "hardened seed %d (%s, T = %d%s) %r" % (seed, algo, T, ", two episodes" if multi else "", counts)
    out = ref_or_failed_init(p, rec, tag, trades=T, algo=algo, mem=p.memory_size, seed=p.seed, rng_stream=book, eps=p.epsilon, extra=x)
    if out is None:
        return
    traj, info, theta = out
    o = ol.Oracle(p, rec)
    if multi:
        replay_multi({"traj": traj, "ends": np.array(info["ends"])}, o.reset, lambda: o.td_step(1), o.clear_inventory,
                     lambda: ol.load().oracle_handle_terminal(o.h), lambda: o.rec(0), tag)
    else:
        o.reset()
        r0 = o.rec(0)
        for n in r0["book"].dtype.names:
            if n != "cursor":
                assert np.array_equal(r0["book"][n], traj[0]["book"][n]), "%s reset book.%s" % (tag, n)
        compare_traj(lambda: o.td_step(1), lambda: o.rec(0), traj, tag)
        o.td_step(1)    # the reference ended on out-of-data / the close
        assert o.counters()[0] == int(info["steps"]), tag
    check_sparse(o.theta(0), theta[0], theta[1], tag)
    o.close()
