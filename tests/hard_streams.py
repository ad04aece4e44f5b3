"""TEST INFRASTRUCTURE: a record-level mutator that turns the tidy streams of gen_stream_host into what vendor depth and
trade files do -- the cases tests/test_convert_ref_sweep.py pins on crafted CSV days, as records of any depth, trade-slot
count and batch size, so that they reach the fast env-step kernels.

    rec2, counts = harden(rec, D, T, seed, kinds=ALL, dry=False)

`rec` is [B, n, W] uint32 from gen_stream_host (prices on the 0.1 grid); the result has the same shape and passes
lob_validate_stream.  Book b's stream is a function of (seed, book0 + b) alone.  Kinds, each switched on by its name:

  same_time    rows, singly and in runs of 2-3, take the previous row's timestamp (LOB_EVT_FLAG_SAME_TIME set as
               lob_convert_csv sets it: on every row whose successor shares its time).  Such a row carries no trades (the
               reference harness stamps a row's trades at t - 1, which would move them before the row they follow).
  crossed      rows, singly and in runs of up to 4, with the two sides swapped and reversed, volumes too: an invalid state
               the event runs on through.  Also inside the warm-up and next to the last row.
  off_grid     a level or trade price moved to a neighbouring float32: mostly the same 1e-4 key with other bits, now and then
               the next key.  A move that would leave a side's keys (or a row's trade keys) not strictly monotone is skipped.
  deep_trades  a row's trades replaced by ONE trade against the previous row's book: at level 3..D, beyond the last level, or
               inside a two-tick spread (exactly at the mid: it runs through both sides); sizes from 1 to well above the
               level's volume.
  jumps        from a row on, every price of the book shifted by +-1..6 ticks (the trades from the next row on: they ran
               against the book before the jump): resting orders are left far behind, or crossed by the book.
  dry          (argument `dry`, off by default) for some books the last k rows flagged LOB_EVT_FLAG_TAS_DRY: only ever a tail.

The streams are built inside the one precondition that ties rows together: the engine holds an event's merged trade list in
max_trades slots, and lob_validate_stream refuses a stream whose merging rows carry more distinct 1e-4 keys.  An event's list
is merged from the rows after the previous event's first row up to its own first row; a row ends an event when the next row's
time differs and the book is not crossed.  A trade whose key would be one too many in its list is dropped; counts["trimmed"]
says how many were, counts["merged"] how many lists are merged from several rows, counts["merged_full"] how many of those
reach exactly T keys.

`counts` = {kind: how many were applied} and the three figures above.  harden_rows() returns, besides, the boolean [B, n] row masks per kind."""
import numpy as np

from rl_markets_amd import abi

KINDS = ("same_time", "crossed", "off_grid", "deep_trades", "jumps")
ALL = KINDS


def _px(ticks):
    # float32 price on the 0.1 grid exactly as the generator makes it (lob_tick_to_price_f32)
    return (np.asarray(ticks, dtype=np.float64) / 10.0).astype(np.float32)


def _key(p):
    return np.rint(np.asarray(p, dtype=np.float64) * 10000.0).astype(np.int64)


def _runs(r, n, lo, hi, prob, max_len, weights):
    """Disjoint runs [(start, length)] in [lo, hi): a start per row with probability `prob`."""
    out, i = [], lo
    starts = r.uniform(size=n) < prob
    lens = r.choice(np.arange(1, max_len + 1), size=n, p=weights)
    while i < hi:
        if starts[i]:
            k = int(min(lens[i], hi - i))
            out.append((i, k))
            i += k + 1     # (a gap of one row: runs do not fuse)
        else:
            i += 1
    return out


def event_firsts(rec, D):
    """bool[n] of one book's records: the row starts an event.  A row ends its event when the next row's time differs and the
    book is not crossed (IsValidState; the mid-price never halves in these streams)."""
    f = rec.view(np.float32)
    ends = ~(f[:, 2] < f[:, 2 + 2 * D]) & np.concatenate([rec[1:, 0] != rec[:-1, 0], [True]])
    return np.concatenate([[True], ends[:-1]])


def _cross(rec, i, D):
    oap, oav, obp, obv = 2, 2 + D, 2 + 2 * D, 2 + 3 * D
    ap, av = rec[i, oap:oap + D].copy(), rec[i, oav:oav + D].copy()
    bp, bv = rec[i, obp:obp + D].copy(), rec[i, obv:obv + D].copy()
    rec[i, oap:oap + D], rec[i, oav:oav + D] = bp[::-1], bv[::-1]
    rec[i, obp:obp + D], rec[i, obv:obv + D] = ap[::-1], av[::-1]


def _harden_book(rec, D, T, r, kinds, dry, straddle, straddle_entry, counts, rows):
    n = rec.shape[0]
    f = rec.view(np.float32)
    oap, oav, obp, obv, otp, otv = 2, 2 + D, 2 + 2 * D, 2 + 3 * D, 2 + 4 * D, 2 + 4 * D + T
    lvl_cols = np.concatenate([np.arange(oap, oap + D), np.arange(obp, obp + D)])

    if "jumps" in kinds:
        shift = np.zeros(n, dtype=np.int64)
        for j in r.choice(np.arange(20, n - 1), size=int(r.integers(1, 4)), replace=False):
            shift[j:] += int(r.integers(1, 7)) * (1 if r.integers(0, 2) else -1)
            rows["jumps"][j] = True
            counts["jumps"] += 1
        ticks = np.rint(f[:, lvl_cols].astype(np.float64) * 10.0).astype(np.int64) + shift[:, None]
        f[:, lvl_cols] = _px(ticks)
        tshift = np.concatenate([[0], shift[:-1]])
        tp = f[:, otp:otp + T]
        tt = np.rint(tp.astype(np.float64) * 10.0).astype(np.int64) + tshift[:, None]
        f[:, otp:otp + T] = np.where(rec[:, otv:otv + T] > 0, _px(tt), np.float32(0.0))

    if "deep_trades" in kinds:
        for i in np.nonzero(r.uniform(size=n) < 0.06)[0]:
            if i == 0:
                continue
            a = np.rint(f[i - 1, oap:oap + D].astype(np.float64) * 10.0).astype(np.int64)
            b = np.rint(f[i - 1, obp:obp + D].astype(np.float64) * 10.0).astype(np.int64)
            av, bv = rec[i - 1, oav:oav + D].astype(np.int64), rec[i - 1, obv:obv + D].astype(np.int64)
            ask_side = bool(r.integers(0, 2))
            what = int(r.integers(0, 3))
            if what == 2 and a[0] - b[0] != 2:
                what = 0
            if what == 0:      # level 3..D
                l = int(r.integers(min(2, D - 1), D))
                t, ref = (a[l], av[l]) if ask_side else (b[l], bv[l])
            elif what == 1:    # beyond the book
                t = a[D - 1] + int(r.integers(1, 4)) if ask_side else b[D - 1] - int(r.integers(1, 4))
                ref = av[D - 1] if ask_side else bv[D - 1]
            else:              # inside a two-tick spread
                t, ref = b[0] + 1, max(av[0], bv[0])
            size = int(r.choice([1, max(1, ref // 7), ref, 3 * ref + 11]))
            rec[i, otp:otv + T] = 0
            f[i, otp] = _px(t)
            rec[i, otv] = size
            rows["deep_trades"][i] = True
            counts["deep_trades"] += 1

    if "crossed" in kinds:
        runs = _runs(r, n, 1, n - 1, 0.012, 4, [0.55, 0.2, 0.15, 0.1])
        taken = np.zeros(n + 1, dtype=bool)
        for s, k in runs:
            taken[max(0, s - 1):s + k + 1] = True
        extra = []
        if r.integers(0, 3) == 0:
            extra.append((int(r.integers(1, 40)), int(r.integers(1, 4))))        # inside the warm-up
        if r.integers(0, 4) == 0:
            k = int(r.integers(1, 3))
            extra.append((n - 1 - k, k))                                          # up to the row next to the last one
        if r.integers(0, 12) == 0:
            extra.append((n - 2, 2))                                              # ... and the last row itself
        if straddle is not None and r.integers(0, 2) == 0:
            extra.append((straddle - 1, 3))
        for s, k in extra:
            if not taken[max(0, s - 1):s + k + 1].any():
                runs.append((s, k))
                taken[max(0, s - 1):s + k + 1] = True
        for s, k in runs:
            for i in range(s, s + k):
                _cross(rec, i, D)
                rows["crossed"][i] = True
            counts["crossed"] += 1
            # the rows the event runs on through, and the row that ends it, hand their trades to the NEXT event: give those
            # that carry none a trade at the touch of the book before the run, so that lists merged from several rows are common
            a0, b0 = f[s - 1, oap], f[s - 1, obp]
            for i in range(s + 1, min(s + k + 1, n)):
                if not (rec[i, otv:otv + T] > 0).any():
                    f[i, otp] = a0 if r.integers(0, 2) else b0
                    rec[i, otv] = int(r.choice([1, 40, 700, 3000]))

    if "same_time" in kinds:
        runs = _runs(r, n, 1, n, 0.03, 3, [0.5, 0.3, 0.2])
        if straddle is not None and rows["crossed"][straddle - 1] and not any(s <= straddle < s + k for s, k in runs):
            runs.append((straddle, 1))     # three crossed rows, the middle one at its predecessor's time: one event up to row straddle + 2
        for s, k in runs:
            rec[s:s + k, 0] = rec[s - 1, 0]
            rec[s:s + k, otp:otv + T] = 0
            counts["deep_trades"] -= int(rows["deep_trades"][s:s + k].sum())     # (a deep trade on such a row is gone with the rest)
            rows["deep_trades"][s:s + k] = False
            rows["same_time"][s:s + k] = True
            counts["same_time"] += 1
    same_next = np.concatenate([rec[1:, 0] == rec[:-1, 0], [False]])
    rec[:, 1] = np.where(same_next, rec[:, 1] | abi.EVT_FLAG_SAME_TIME, rec[:, 1] & ~np.uint32(abi.EVT_FLAG_SAME_TIME))

    if "off_grid" in kinds:
        cols = np.concatenate([lvl_cols, np.arange(otp, otp + T)])
        for i in np.nonzero(r.uniform(size=n) < 1.0 / 3.0)[0]:
            c = int(r.choice(cols))
            up = bool(r.integers(0, 2))
            old = f[i, c]
            if not old > 0:
                continue
            f[i, c] = np.nextafter(old, np.float32(1e9 if up else 0.0))
            if c < otp:
                o = oap if c < oap + D else obp
                k = _key(f[i, o:o + D])
                ok = (np.diff(k) > 0).all() if o == oap else (np.diff(k) < 0).all()
            else:
                live = rec[i, otv:otv + T] > 0
                ok = (np.diff(_key(f[i, otp:otp + T][live])) > 0).all()
            if not ok:
                f[i, c] = old
                continue
            rows["off_grid"][i] = True
            counts["off_grid"] += 1

    if straddle_entry is not None and "crossed" in kinds and r.integers(0, 2) == 0:
        # the event with track entry straddle_entry - 1 made a run of three crossed rows and the row behind them: the next
        # entry's trade list is merged from the rows of this one
        first = np.flatnonzero(event_firsts(rec, D))
        if len(first) > straddle_entry + 4 and first[straddle_entry - 1] + 5 < n:
            s0 = int(first[straddle_entry - 1])
            for i in range(s0, s0 + 3):
                if not f[i, oap] < f[i, obp]:
                    _cross(rec, i, D)
                    rows["crossed"][i] = True
            counts["crossed"] += 1

    # An event's merged trade list within T keys: what lob_validate_stream checks (event j's list is merged from rows
    # first[j - 1] + 1 .. first[j]).  A trade whose key would be one too many is dropped -- counted in "trimmed"; the lists that
    # are merged from several rows ("merged") and reach exactly T keys that way ("merged_full") are counted too.
    first = event_firsts(rec, D)
    keys, contributing = set(), 0
    for i in range(n):
        kept = []
        n_live = 0
        for slot in range(T):
            if rec[i, otv + slot] == 0:
                continue
            n_live += 1
            k = int(_key(f[i, otp + slot]))
            if k in keys or len(keys) < T:
                keys.add(k)
                kept.append((rec[i, otp + slot], rec[i, otv + slot]))
        if len(kept) < n_live:
            counts["trimmed"] += n_live - len(kept)
            rec[i, otp:otv + T] = 0
            for slot, (px, vol) in enumerate(kept):
                rec[i, otp + slot], rec[i, otv + slot] = px, vol
            if not kept and rows["deep_trades"][i]:
                rows["deep_trades"][i] = False
                counts["deep_trades"] -= 1
        contributing += bool(kept)
        if first[i]:
            if contributing >= 2:
                counts["merged"] += 1
                if len(keys) == T:
                    counts["merged_full"] += 1
                    rows["merged_full"][i] = True
            keys, contributing = set(), 0

    if dry and r.integers(0, 5) < 2:
        k = int(r.integers(2, (3 * n) // 4))
        rec[n - k:, 1] |= abi.EVT_FLAG_TAS_DRY
        rows["dry"][n - k:] = True
        counts["dry"] += 1


BOOKKEEPING = ("trimmed", "merged", "merged_full")


def harden_rows(rec, D, T, seed, kinds=ALL, dry=False, book0=0, straddle=None, straddle_entry=None):
    """-> (hardened copy, counts, {kind: bool[B, n] of the rows it touched}).  `straddle`: a row index across which half the
    books get three crossed rows, the middle one with its predecessor's timestamp (one event over four rows or more).
    `straddle_entry`: an event index k; in half the books event k - 1 becomes such a run, so that event k's trade list is merged
    from several rows (a market-track ring refilled up to entry k - 1 stops between the two).  rows["merged_full"] marks the
    first rows of events whose list reaches exactly T keys over several rows."""
    rec = np.array(rec, dtype=np.uint32, copy=True, order="C")
    B, n, W = rec.shape
    assert W == abi.load().lob_record_words(D, T) and n >= 64
    assert set(kinds) <= set(KINDS), kinds
    counts = {k: 0 for k in KINDS + ("dry",) + BOOKKEEPING}
    rows = {k: np.zeros((B, n), dtype=bool) for k in KINDS + ("dry", "merged_full")}
    for b in range(B):
        _harden_book(rec[b], D, T, np.random.default_rng([int(seed), book0 + b]), tuple(kinds), dry, straddle, straddle_entry, counts,
                     {k: v[b] for k, v in rows.items()})
    return rec, counts, rows


def harden(rec, D, T, seed, kinds=ALL, dry=False, book0=0, straddle=None, straddle_entry=None):
    out, counts, _ = harden_rows(rec, D, T, seed, kinds, dry, book0, straddle, straddle_entry)
    return out, counts


# ---- the batch the GPU tests run (tests/test_gpu_hard_streams.py) and tests/test_hard_streams.py proves non-trivial -------------
B, N_EVENTS, DEPTH, TRADES, SEED = 200, 400, 10, 2, 20260
CASES = {k: ((k,), False) for k in KINDS}
CASES["all"] = (ALL, False)
CASES["all+dry"] = (ALL, True)
_cache = {}


def plain_batch(n_books=B, n_events=N_EVENTS, depth=DEPTH, trades=TRADES):
    from rl_markets_amd import engine
    key = ("plain", n_books, n_events, depth, trades)
    if key not in _cache:
        g = engine.default_gen_params()
        g.n_events = n_events
        rec = engine.gen_stream_host(g, depth, trades, 0, n_books)
        rec.setflags(write=False)
        _cache[key] = rec
    return _cache[key]


def batch(case, straddle=None, straddle_entry=None):
    """-> (records [B, N_EVENTS, W], counts, row masks) of one of CASES: computed once, shared, read-only."""
    key = (case, straddle, straddle_entry)
    if key not in _cache:
        kinds, dry = CASES[case]
        rec, counts, rows = harden_rows(plain_batch(), DEPTH, TRADES, SEED, kinds, dry, straddle=straddle, straddle_entry=straddle_entry)
        rec.setflags(write=False)
        _cache[key] = (rec, counts, rows)
    return _cache[key]
