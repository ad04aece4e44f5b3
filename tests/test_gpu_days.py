"""The day library (lob_load_days): recorded days resident in HBM, a day drawn per book and episode on the device
(days_draw_kernel), the reference's training loop (src/main.cpp:51-55) and test loop (src/main.cpp:215-239).

Against the oracle a book of the library is a one-book oracle over its own day.  The oracle reads its records in place, so a
book can switch between two days of the SAME length by writing the second over the first in the oracle's buffer (the library
holds its lengths in pairs), and it changes to a day of ANOTHER length through Oracle.set_days (oracle_set_days, pinned by
tests/test_oracle_days.py) -- a day padded to a longer length with time-and-sales-dry rows is not the same day to the oracle
(tests/test_days_abi.py shows where they part).  The tests here use private theta; one weight vector over unequal days is
tests/test_gpu_days_shared.py, against the batched oracle over days."""
import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import days_ref
from tests import oracle_lib as ol
from tests.parity import assert_books_equal, dumps_to_np

pytestmark = pytest.mark.gpu

DEPTH, TRADES = 5, 2


def make_days(lengths, first_id=1000, depth=DEPTH):
    """Synthetic days of the given lengths, each its own generator book id (different content)."""
    out = []
    for i, n in enumerate(lengths):
        g = engine.default_gen_params()
        g.n_events = int(n)
        out.append(engine.gen_stream_host(g, depth, TRADES, first_id + i, 1)[0])
    return out


def params(algo=abi.ALGO_QLAMBDA, theta_mode=abi.THETA_PRIVATE, mem=1 << 16, first_book=0, seed=1994):
    p = engine.default_params()
    p.depth, p.max_trades = DEPTH, TRADES
    p.algo, p.theta_mode, p.memory_size = algo, theta_mode, mem
    p.book_id_offset, p.seed = first_book, seed
    return p


def engine_view(eng):
    """What compare_book reads of the engine, read once per step."""
    return {"books": dumps_to_np(eng.get_books()), "rng": eng.rng_counters(), "stepped": eng.stepped(), "action": eng.last_actions(),
            "reward": eng.last_rewards(), "vars": eng.learner_state(), "td": eng.last_td(), "V": eng.V}


def compare_book(ev, b, orc, tag):
    """Book b of the engine (engine_view `ev`) against the one-book oracle `orc`, private theta: exact."""
    recs = orc.recs()
    eb = ev["books"]
    assert_books_equal(eb[b:b + 1], recs["book"], tag)
    np.testing.assert_array_equal(eb["n_traces"][b:b + 1], recs["book"]["n_traces"], err_msg=tag + " n_traces")
    np.testing.assert_array_equal(ev["rng"][b], recs["rng_ctr"][0], err_msg=tag + " rng counters")
    if ev["stepped"][b]:
        assert ev["action"][b] == recs["action"][0], tag + " action"
        assert ev["reward"][b] == recs["reward"][0], tag + " reward"
        np.testing.assert_array_equal(ev["vars"][b], recs["vars"][0][:ev["V"]], err_msg=tag + " state vars")
        assert ev["td"][b] == recs["td"][0], tag + " td"


def test_explicit_days_match_oracle():
    """B = 24, private theta, 6 days of 300-900 events in three pairs of equal length; two episodes with different
    lob_days_set assignments (the other day of the pair, written over the first in the oracle's buffer), then a third whose
    assignment changes the length of every book's day (Oracle.set_days); every step against one-book oracles."""
    B, steps = 24, 200
    lengths = [310, 310, 620, 620, 900, 900]
    days = make_days(lengths)
    rng = np.random.default_rng(11)
    ep1 = rng.integers(0, 6, size=B).astype(np.int32)
    ep1[:6] = np.arange(6)
    ep2 = (ep1 ^ 1).astype(np.int32)   # the other day of the pair: same length, other content
    ep3 = ((ep2 + 2) % 6).astype(np.int32)   # the next pair: another length for every book
    assert (np.array(lengths)[ep3] != np.array(lengths)[ep2]).all()
    lib = ol.DayLibrary(days)
    p = params()
    eng = engine.Engine(p, B)
    eng.load_days(days)
    orcs = []
    for b in range(B):
        p1 = params(first_book=b)
        orcs.append(ol.Oracle(p1, days[ep1[b]][None].copy()))
    for ep, assign in enumerate((ep1, ep2, ep3)):
        eng.days_set(assign)
        if ep == 1:
            for b in range(B):
                orcs[b].records[0][...] = days[assign[b]]   # (in place: the oracle reads this buffer)
        elif ep == 2:
            for b in range(B):
                orcs[b].set_days(*lib.of(assign[b:b + 1]))
        eng.reset()
        np.testing.assert_array_equal(eng.days(), assign)
        for o in orcs:
            o.reset()
        ev = engine_view(eng)
        for b in range(B):
            compare_book(ev, b, orcs[b], "episode %d reset book %d" % (ep, b))
        for s in range(steps):
            eng.td_step(1)
            for o in orcs:
                o.td_step(1)
            ev = engine_view(eng)
            for b in range(B):
                compare_book(ev, b, orcs[b], "episode %d step %d book %d" % (ep, s, b))
        if ep == 0:
            assert (ev["books"]["terminal"][ep1 < 2] == 2).all(), "the short days run out of data inside the episode"
    for b in range(B):
        np.testing.assert_array_equal(eng.theta(b), orcs[b].theta(0), err_msg="theta of book %d" % b)


def test_equal_length_library_is_the_shared_stream():
    """A library of days of one length played through lob_days_set is lob_load_events_shared with phase = the days'
    offsets: book dumps bit for bit, theta to the last bits, over two episodes (shared theta)."""
    B, L, steps = 48, 500, 120
    flat = make_days([5 * L])[0]              # (one recorded stream: the shared loader validates it as one)
    days = [flat[i * L:(i + 1) * L] for i in range(5)]
    p = params(theta_mode=abi.THETA_SHARED, mem=1 << 20)
    a, s = engine.Engine(p, B), engine.Engine(p, B)
    a.load_days(days)
    rng = np.random.default_rng(5)
    for ep in range(2):
        assign = rng.integers(0, 5, size=B).astype(np.int32)
        a.days_set(assign)
        s.load_events_shared(flat, assign.astype(np.int64) * L, L)
        a.reset()
        s.reset()
        a.td_step(steps)
        s.td_step(steps)
        da, ds = dumps_to_np(a.get_books()), dumps_to_np(s.get_books())
        for name in da.dtype.names:
            assert np.array_equal(da[name], ds[name]), (ep, name)
        # (shared theta is a sum of f64 atomic additions in whatever order the hardware makes them: two runs of ONE
        # configuration differ in the last bits, test_gpu_replay.py / parity.py)
        np.testing.assert_allclose(a.theta(), s.theta(), rtol=1e-9, atol=1e-12, err_msg="episode %d" % ep)


def test_random_draws_are_exact():
    """lob_days_select(RANDOM): each book's days are RandomSampler's with the seed + global book id, across
    episodes; two engines of B/2 (book_id_offset 0 and B/2) draw what one engine of B draws."""
    B, n_days, first, n = 96, 7, 2, 5
    days = make_days([200 + 37 * i for i in range(n_days)])
    p = params(seed=777)
    eng = engine.Engine(p, B)
    eng.load_days(days)
    halves = []
    for off in (0, B // 2):
        h = engine.Engine(params(seed=777, first_book=off), B // 2)
        h.load_days(days)
        halves.append(h)
    want = np.array([days_ref.book_days(777, b, n, 3) for b in range(B)]) + first
    for ep in range(3):
        eng.days_select(abi.DAYS_RANDOM, first, n)
        eng.reset()
        got = eng.days()
        np.testing.assert_array_equal(got, want[:, ep], err_msg="episode %d" % ep)
        for h in halves:
            h.days_select(abi.DAYS_RANDOM, first, n)
            h.reset()
        np.testing.assert_array_equal(np.concatenate([h.days() for h in halves]), got, err_msg="sharded, episode %d" % ep)
        eng.td_step(3)
    # a reset without a new selection replays the same days
    eng.reset()
    np.testing.assert_array_equal(eng.days(), want[:, 2])


def test_in_order_days():
    B = 40
    days = make_days([150, 260, 180, 400, 220, 300])
    eng = engine.Engine(params(), B)
    eng.load_days(days)
    eng.days_select(abi.DAYS_IN_ORDER, 1, 4)
    eng.reset()
    np.testing.assert_array_equal(eng.days(), 1 + np.arange(B) % 4)
    eng.td_step(5)
    # with an offset, the global id decides
    e2 = engine.Engine(params(first_book=3), 8)
    e2.load_days(days)
    e2.days_select(abi.DAYS_IN_ORDER, 0, 6)
    e2.reset()
    np.testing.assert_array_equal(e2.days(), (3 + np.arange(8)) % 6)


@pytest.mark.parametrize("algo", [abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q, abi.ALGO_SARSA])
def test_library_at_scale_ring_mode(monkeypatch, algo):
    """16 384 books, private theta, 8 days in four pairs of unequal length, the longest longer than the track ring
    (LOB_TRACK_RING = 1024: ring mode for every book); three episodes with a fresh random draw each, every episode run until
    no book is live.  Every 8th step, against one-book oracles that carry on across the episodes, each given its book's drawn
    day through Oracle.set_days (the draws are RandomSampler's, known in advance):
      * the first book of each day of the first episode, so the short days run out of data and the long ones wrap the ring;
      * six books that change to a day of another length between episodes."""
    monkeypatch.setenv("LOB_TRACK_RING", "1024")
    B, episodes = 16384, 3
    lengths = [400, 400, 700, 700, 1000, 1000, 1500, 1500]
    days = make_days(lengths)
    p = params(algo=algo, mem=1 << 12)
    # the first draw of 16 384 consecutive seeds is one or two neighbouring days for every book (minstd_rand0's first value is
    # 16807 x seed): it is drawn and replaced before the first reset, the three episodes play draws 2-4
    draws = np.array([days_ref.book_days(p.seed, b, len(days), episodes + 1) for b in range(B)])[:, 1:]
    lib = ol.DayLibrary(days)
    steady = {}
    for k in range(len(days)):   # the first book of each day of the first episode
        books = np.nonzero(draws[:, 0] == k)[0]
        assert len(books), k
        steady[int(books[0])] = k
    movers = [int(b) for b in np.nonzero(np.ptp(np.array(lengths)[draws], axis=1) > 0)[0] if int(b) not in steady][:6]
    assert len(movers) == 6
    eng = engine.Engine(p, B)
    eng.load_days(days)
    eng.days_select(abi.DAYS_RANDOM, 0, len(days))   # (the correlated first draw, replaced below before any reset)
    orcs = {b: ol.Oracle(params(algo=algo, mem=1 << 12, first_book=b), days[draws[b, 0]][None].copy()) for b in steady}
    ones = {b: ol.Oracle(params(algo=algo, mem=1 << 12, first_book=b), days[draws[b, 0]][None].copy()) for b in movers}
    for ep in range(episodes):
        eng.days_select(abi.DAYS_RANDOM, 0, len(days))
        eng.reset()
        d = eng.days()
        np.testing.assert_array_equal(d, draws[:, ep])
        for b, o in list(orcs.items()) + list(ones.items()):
            if ep:
                o.set_days(*lib.of(d[b:b + 1]))
            o.reset()
        steps = 0
        while eng.counters()[2] > 0:
            assert steps < 4000, "episode %d does not end" % ep
            eng.td_step(8)
            steps += 8
            for o in orcs.values():
                o.td_step(8)
            for o in ones.values():
                o.td_step(8)
            ev = engine_view(eng)
            for b, o in orcs.items():
                compare_book(ev, b, o, "episode %d step %d book %d" % (ep, steps, b))
            for b, o in ones.items():
                compare_book(ev, b, o, "episode %d step %d mover %d" % (ep, steps, b))
        eb = ev["books"]
        short = np.array(lengths)[d] == 400
        assert (eb["terminal"][short] == 2).all(), "the 400-event days run out of data"
        long_ = np.array(lengths)[d] == 1500
        assert (eb["cursor"][long_] > 1024).any(), "the 1500-event days wrap the 1024-entry ring"
    for b, o in orcs.items():
        np.testing.assert_array_equal(eng.theta(b), o.theta(0), err_msg="theta of book %d" % b)
    for b, o in ones.items():
        np.testing.assert_array_equal(eng.theta(b), o.theta(0), err_msg="theta of book %d" % b)


def test_day_library_errors():
    days = make_days([300, 200, 250])
    flat = np.ascontiguousarray(np.concatenate(days))
    lib = abi.load()
    eng = engine.Engine(params(), 8)

    def load(first):
        f = np.ascontiguousarray(first, dtype=np.int64)
        return lib.lob_load_days(eng.h, engine._ptr(flat), engine._ptr(f), len(f) - 1)

    assert load([0, 300, 250, 750]) == abi.LOB_EINVAL          # not monotone
    assert load([0, 300, 301, 750]) == abi.LOB_EINVAL          # a day of one event
    # no selection yet: no reset
    eng.load_days(days)
    assert lib.lob_reset(eng.h) == abi.LOB_ESTATE
    assert lib.lob_days_select(eng.h, abi.DAYS_RANDOM, 2, 2) == abi.LOB_EINVAL   # days 2, 3 of 3
    assert lib.lob_days_select(eng.h, 7, 0, 1) == abi.LOB_EINVAL
    bad = np.zeros(8, np.int32)
    bad[5] = 3
    assert lib.lob_days_set(eng.h, engine._ptr(bad)) == abi.LOB_EINVAL
    with pytest.raises(engine.LobError):
        eng.days()                                              # no episode on the library yet
    eng.days_select(abi.DAYS_IN_ORDER, 0, 3)
    eng.reset()
    eng.td_step(2)
    # a learner step half done: no selection
    if lib.lob_td_split_supported(eng.h):
        assert lib.lob_td_step_begin(eng.h) == 0
        assert lib.lob_days_select(eng.h, abi.DAYS_RANDOM, 0, 3) == abi.LOB_ESTATE
        assert lib.lob_td_step_end(eng.h) == 0
    # no staging over a library
    per_book = np.stack([days[1][:200]] * 8)
    assert lib.lob_stage_events(eng.h, engine._ptr(per_book), 200) == abi.LOB_ESTATE
    # the old loaders still work and return the engine to their modes
    eng.load_events(per_book)
    eng.reset()
    eng.td_step(5)
    assert lib.lob_days_select(eng.h, abi.DAYS_RANDOM, 0, 1) == abi.LOB_ESTATE
