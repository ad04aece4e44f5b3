"""Thin Python handle over the C ABI (include/lob_engine.h).

Only plumbing lives here (buffer allocation, error mapping); every
computation happens in liblob_engine.so on the GPU.  The class mirrors the
reference's call surface for the hot path:

    reset()            environment::Base::Initialise + Runner prologue
    step(actions)      environment::Base::performAction
    get_state()        environment::Base::getState
    get_reward()       environment::Base::getReward
    td_step(n)         experiment::serial::Learner::_step  x n
    eval_step(n)       experiment::serial::Backtester::_step x n
"""
import ctypes as C

import numpy as np

from . import abi


class LobError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lob_engine error %d: %s" % (code, msg))
        self.code = code


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def default_params():
    lib = abi.load()
    p = abi.Params()
    lib.lob_default_params(C.byref(p))
    return p


def default_gen_params():
    lib = abi.load()
    g = abi.GenParams()
    lib.lob_default_gen_params(C.byref(g))
    return g


def record_words(depth, max_trades):
    return abi.load().lob_record_words(depth, max_trades)


def gen_stream_host(gen, depth, max_trades, first_book, n_books):
    lib = abi.load()
    W = lib.lob_record_words(depth, max_trades)
    out = np.zeros((n_books, gen.n_events, W), dtype=np.uint32)
    rc = lib.lob_gen_stream_host(C.byref(gen), depth, max_trades, C.c_uint64(first_book), n_books, _ptr(out))
    if rc:
        raise LobError(rc, lib.lob_last_error().decode())
    return out


# numpy view of abi.EpisodeStats (lob_episode_record): rows of Engine.episode_stats, operands of merge_episode_stats
_STAT_F64 = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("min", "<f8"), ("max", "<f8"), ("argmin", "<i8"), ("argmax", "<i8")])
_STAT_I64 = np.dtype([("sum", "<i8"), ("sumsq", "<i8"), ("min", "<i8"), ("max", "<i8"), ("argmin", "<i8"), ("argmax", "<i8")])
EPISODE_STATS_DTYPE = np.dtype([("group", "<i4"), ("n_books", "<i4"), ("n_live", "<i4"), ("n_terminal", "<i4"),
                                ("n_out_of_data", "<i4"), ("n_rho", "<i4"), ("f", _STAT_F64, (4,)), ("i", _STAT_I64, (4,))])
assert EPISODE_STATS_DTYPE.itemsize == C.sizeof(abi.EpisodeStats)


# numpy view of abi.StepRow (lob_step_row): the elements of Engine.step_log_read
STEP_ROW_DTYPE = np.dtype([("time_ms", "<i8"), ("position", "<i8"), ("midprice", "<f8"), ("spread", "<f8"), ("ask_quote", "<f8"),
                           ("bid_quote", "<f8"), ("pnl_step", "<f8"), ("episode_pnl", "<f8"), ("episode_bandh", "<f8"),
                           ("episode_reward", "<f8"), ("step", "<i4"), ("action", "<i4"), ("ask_level", "<i4"), ("bid_level", "<i4")])
assert STEP_ROW_DTYPE.itemsize == C.sizeof(abi.StepRow) == 96


def merge_episode_stats(a, b):
    """lob_episode_stats_merge: the record of the books of `a` and `b` together (one row each, or arrays of equal length
    merged row by row) -- how the records of several engines are put together.  Host only."""
    lib = abi.load()
    a, b = np.asarray(a, dtype=EPISODE_STATS_DTYPE), np.asarray(b, dtype=EPISODE_STATS_DTYPE)
    assert a.shape == b.shape
    o, f = np.array(a.reshape(-1), copy=True), np.ascontiguousarray(b.reshape(-1))
    for k in range(o.shape[0]):
        lib.lob_episode_stats_merge(_ptr(o[k:k + 1]), _ptr(f[k:k + 1]))
    return o.reshape(a.shape)


def _take_records(lib, ptr, n, depth, max_trades):
    W = lib.lob_record_words(depth, max_trades)
    buf = (C.c_uint32 * (n * W)).from_address(ptr.value)
    out = np.frombuffer(buf, dtype=np.uint32).reshape(1, n, W).copy()
    lib.lob_free(ptr)
    return out


def convert_csv(md_path, tas_path, max_trades=2):
    """The reference's CSV pair (5-level depth + time-and-sales) -> records[1][n][W]."""
    lib = abi.load()
    ptr, n = C.c_void_p(), C.c_int32()
    rc = lib.lob_convert_csv(md_path.encode(), tas_path.encode(), max_trades, C.byref(ptr), C.byref(n))
    if rc:
        raise LobError(rc, lib.lob_last_error().decode())
    return _take_records(lib, ptr, n.value, 5, max_trades)


def convert_lobster(orderbook_path, message_path, levels_in_file, depth, max_trades=4):
    """LOBSTER orderbook + message files -> records[1][n][W] (one record per millisecond)."""
    lib = abi.load()
    ptr, n = C.c_void_p(), C.c_int32()
    rc = lib.lob_convert_lobster(orderbook_path.encode(), message_path.encode(), levels_in_file, depth, max_trades,
                                 C.byref(ptr), C.byref(n))
    if rc:
        raise LobError(rc, lib.lob_last_error().decode())
    return _take_records(lib, ptr, n.value, depth, max_trades)


class Engine:
    def __init__(self, params, n_books, device=0):
        self.lib = abi.load()
        self.params = params
        self.B = int(n_books)
        self.V = params.n_vars
        self.M = params.memory_size
        h = C.c_void_p()
        self._check(self.lib.lob_create(C.byref(params), self.B, device, C.byref(h)))
        self.h = h

    def _check(self, rc):
        if rc != abi.LOB_OK:
            raise LobError(rc, self.lib.lob_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.lob_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- streams ----
    def load_events(self, records):
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        assert rec.shape[0] == self.B
        self._check(self.lib.lob_load_events(self.h, _ptr(rec), rec.shape[1]))

    def load_events_shared(self, records, phase, n_events):
        """One recorded stream [n_total][W] replayed by every book from its own phase."""
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        assert rec.ndim == 2
        ph = np.ascontiguousarray(phase, dtype=np.int64)
        assert ph.shape == (self.B,)
        self._check(self.lib.lob_load_events_shared(self.h, _ptr(rec), rec.shape[0], _ptr(ph), n_events))

    def stage_events(self, records):
        """lob_stage_events: the next episode's streams, handed over while this one runs; the next reset() adopts them."""
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        assert rec.shape[0] == self.B
        self._staged = rec          # (the caller's buffer must outlive the hand-over)
        self._check(self.lib.lob_stage_events(self.h, _ptr(rec), rec.shape[1]))

    def stage_wait(self):
        self._check(self.lib.lob_stage_wait(self.h))

    def gen_events(self, gen):
        self._check(self.lib.lob_gen_events_device(self.h, C.byref(gen)))

    # ---- day library (lob_load_days) ----
    def load_days(self, days):
        """A library of recorded days, each records[n][W] (or [1][n][W], as convert_csv gives), resident in HBM."""
        days = [np.asarray(d, dtype=np.uint32).reshape(-1, np.asarray(d).shape[-1]) for d in days]
        first = np.zeros(len(days) + 1, dtype=np.int64)
        first[1:] = np.cumsum([d.shape[0] for d in days])
        rec = np.ascontiguousarray(np.concatenate(days, axis=0))
        self._check(self.lib.lob_load_days(self.h, _ptr(rec), _ptr(first), len(days)))
        self.day_first = first

    def days_select(self, mode, first, n):
        """Every book draws its next day from days first .. first + n - 1 (abi.DAYS_RANDOM / abi.DAYS_IN_ORDER);
        the next reset() plays it."""
        self._check(self.lib.lob_days_select(self.h, int(mode), int(first), int(n)))

    def days_set(self, days):
        """The day of every book for the next reset()."""
        d = np.ascontiguousarray(days, dtype=np.int32)
        assert d.shape == (self.B,)
        self._check(self.lib.lob_days_set(self.h, _ptr(d)))

    def days(self):
        """The day each book is playing."""
        out = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.lob_get_days(self.h, _ptr(out)))
        return out

    # ---- environment ----
    def reset(self):
        self._check(self.lib.lob_reset(self.h))

    def step(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.int32)
        assert a.shape == (self.B,)
        self._check(self.lib.lob_step(self.h, _ptr(a)))

    def get_state(self):
        out = np.zeros((self.B, self.V), np.float32)
        self._check(self.lib.lob_get_state(self.h, _ptr(out)))
        return out

    def get_reward(self):
        out = np.zeros(self.B, np.float64)
        self._check(self.lib.lob_get_reward(self.h, _ptr(out)))
        return out

    def get_terminal(self):
        out = np.zeros(self.B, np.uint8)
        self._check(self.lib.lob_get_terminal(self.h, _ptr(out)))
        return out

    def clear_inventory(self):
        self._check(self.lib.lob_clear_inventory(self.h))

    def get_books(self, first=0, n=None):
        n = self.B - first if n is None else n
        out = (abi.BookDump * n)()
        self._check(self.lib.lob_get_books(self.h, first, n, C.cast(out, C.c_void_p)))
        return out

    def episode_stats(self, by_day=False):
        """lob_episode_stats: the batch's episode statistics reduced on the device, one row (EPISODE_STATS_DTYPE) per record --
        row 0 the whole engine, with by_day row 1 + d the books playing library day d."""
        n = C.c_int32(0)
        out = np.zeros(1, dtype=EPISODE_STATS_DTYPE)
        rc = self.lib.lob_episode_stats(self.h, 1 if by_day else 0, _ptr(out), 1, C.byref(n))
        if rc == abi.LOB_EINVAL and n.value > 1:   # one record per day as well: the call has said how many
            out = np.zeros(n.value, dtype=EPISODE_STATS_DTYPE)
            rc = self.lib.lob_episode_stats(self.h, 1, _ptr(out), out.shape[0], C.byref(n))
        self._check(rc)
        return out[:n.value]

    def step_log_enable(self, books, cap_steps):
        """lob_step_log_enable: record the profit-log row of every completed step of `books` (local indices, strictly ascending;
        None: every book) on the device, up to cap_steps rows per book, from the next reset() on.  books == []: off."""
        if books is None:
            n, rc = self.B, self.lib.lob_step_log_enable(self.h, None, self.B, cap_steps)
        else:
            sel = np.ascontiguousarray(books, dtype=np.int32).reshape(-1)
            n, rc = int(sel.shape[0]), self.lib.lob_step_log_enable(self.h, _ptr(sel) if sel.shape[0] else None, sel.shape[0], cap_steps)
        if rc == abi.LOB_OK:
            self._slog_n, self._slog_cap = n, cap_steps
        elif rc == abi.LOB_ENOMEM:     # (a refused list or state leaves the log as it was; this has switched it off)
            self._slog_n = 0
        self._check(rc)

    def step_log_counts(self):
        """lob_step_log_counts: (stored rows, lost rows) of every selected book, int32[n_sel] each."""
        n = getattr(self, "_slog_n", 0)
        rows, lost = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.lib.lob_step_log_counts(self.h, _ptr(rows), _ptr(lost)))
        return rows[:n], lost[:n]

    def step_log_read(self, first_sel=0, n_sel=None, first_row=0, n_rows=None):
        """lob_step_log_read: ndarray[n_sel, n_rows] of STEP_ROW_DTYPE, element [j, k] = row first_row + k of selected book
        first_sel + j; slots beyond a book's stored count are zero (step == 0).  Defaults: the rest of the selection, and rows
        up to the longest stored count (at least one)."""
        if n_sel is None:
            n_sel = getattr(self, "_slog_n", 0) - first_sel
        if n_rows is None:
            n_rows = max(1, int(self.step_log_counts()[0].max(initial=0)) - first_row)
        out = np.zeros((max(n_sel, 1), max(n_rows, 1)), dtype=STEP_ROW_DTYPE)
        self._check(self.lib.lob_step_log_read(self.h, first_sel, n_sel, first_row, n_rows, _ptr(out)))
        return out[:max(n_sel, 0), :max(n_rows, 0)]

    # ---- vector-env interface: raw device addresses in, nothing waits (rl_markets_amd/vec_env.py is the torch-facing wrapper) ----
    def vec_step(self, actions_ptr, out):
        """lob_vec_step: performAction(actions[b]) for every live book, actions read from the int32[n_books] device buffer at
        `actions_ptr`, results written to the device buffers of `out` (abi.VecOut) -- enqueued on the engine's stream."""
        self._check(self.lib.lob_vec_step(self.h, C.c_void_p(actions_ptr), C.byref(out)))

    def vec_observe(self, out):
        """lob_vec_observe: the outputs of vec_step without a step (after reset(), after clear_inventory())."""
        self._check(self.lib.lob_vec_observe(self.h, C.byref(out)))

    def vec_status(self):
        """lob_vec_status: waits for the stream once; (return code, actions out of range since the last call).  LOB_EDATA is
        raised as every other entry point raises it; LOB_EINVAL -- bad actions -- is returned, with the count."""
        n = C.c_int64(0)
        rc = self.lib.lob_vec_status(self.h, C.byref(n))
        if rc not in (abi.LOB_OK, abi.LOB_EINVAL):
            self._check(rc)
        return rc, int(n.value)

    def look_ring(self, on):
        """lob_look_ring: the per-engine switch that lets vec_peek, vec_rollout and the branch calls run on a ring-mode stream (off
        after creation, kept across reset()).  There their `terminal` planes may hold abi.TERMINAL_AHEAD (the step would read beyond
        the track's window; dropped) and, for branch_step, abi.TERMINAL_BEHIND (the branch fell behind the window; nothing
        attempted).  Changes nothing on a resident track; the snapshots stay refused on a ring."""
        self._check(self.lib.lob_look_ring(self.h, 1 if on else 0))

    def track_window(self):
        """lob_track_window: (lo, hi, complete), int32 arrays [B] -- the entries [lo, hi) of every book's market track that a
        look-ahead can be served from (hi = the entries written so far; complete: that is all of the stream).  Waits for the stream."""
        lo, hi, comp = (np.empty(self.B, dtype=np.int32) for _ in range(3))
        self._check(self.lib.lob_track_window(self.h, lo.ctypes.data, hi.ctypes.data, comp.ctypes.data))
        return lo, hi, comp

    def look_counts(self):
        """lob_look_counts: (ahead, behind) cells of the look-aheads on a ring as the last vec_status() read and cleared them."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.lob_look_counts(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def vec_book(self, out):
        """lob_vec_book: the depth levels of every book, the agent's own sixteen words (abi.OWN_*) and the market time, written to
        the device buffers of `out` (abi.VecBookOut) -- every value what get_books() reports, as f32; enqueued on the engine's
        stream."""
        self._check(self.lib.lob_vec_book(self.h, C.byref(out)))

    def vec_history(self, K, out):
        """lob_vec_history: the last K (1 .. abi.MAX_HISTORY) event records of every book -- levels f32 [B, K, 4, depth], trades f32
        [B, K, 2, max_trades], time_ms i32 [B, K], oldest first, the record behind the current snapshot in slot K - 1, zeros before
        the start of the book's stream --, n_valid and rec i32 [B], written to the device buffers of `out` (abi.VecHistOut);
        enqueued on the engine's stream."""
        self._check(self.lib.lob_vec_history(self.h, int(K), C.byref(out)))

    def vec_act(self, mode, out):
        """lob_vec_act: Q(s, .) of every book's latest getState() under the engine's own weights and the action its policy takes there
        (mode abi.ACT_GREEDY: what eval_step plays; abi.ACT_BEHAVIOUR: the learner's epsilon-greedy / Boltzmann policy;
        abi.ACT_ARGMAX: the first maximum, nothing drawn), written to the device buffers of `out` (abi.VecActOut: action int32 [B],
        q f64 [B, 9]); enqueued on the engine's stream.  Works after snapshot_restore() as well."""
        self._check(self.lib.lob_vec_act(self.h, int(mode), C.byref(out)))

    def vec_q(self, vars_ptr, n, q_ptr):
        """lob_vec_q: q_values() with both ends in device memory -- f32 [n, n_vars] at `vars_ptr` in, f64 [n, 9] at `q_ptr` out;
        enqueued on the engine's stream."""
        self._check(self.lib.lob_vec_q(self.h, C.c_void_p(vars_ptr), int(n), C.c_void_p(q_ptr)))

    def vec_terms(self):
        """lob_vec_terms: the 27 action terms [group][action] of the tile hash, reduced mod memory_size -- a list of three lists of
        nine ints.  (sums + term) mod M is the tile index (vec_features); host-only, no device is touched."""
        buf = (C.c_int32 * 27)()
        self._check(self.lib.lob_vec_terms(self.h, buf))
        return [list(buf[g * abi.LOB_N_ACTIONS:(g + 1) * abi.LOB_N_ACTIONS]) for g in range(3)]

    def vec_features(self, vars_ptr, n, actions_ptr, out):
        """lob_vec_features: the 96 action-independent hash sums of n states' tiles (out.sums, int32 [n, 96]) and the tile indices
        of the action at `actions_ptr` (int32 [n]) per state (out.idx, int32 [n, 96]; -1 for an action out of range) into the device
        buffers of `out` (abi.VecFeatOut; 0 = not wanted).  `vars_ptr`: f32 [n, n_vars] in device memory, or None: the books' latest
        observation (n = n_books).  Enqueued on the engine's stream."""
        self._check(self.lib.lob_vec_features(self.h, C.c_void_p(vars_ptr), int(n), C.c_void_p(actions_ptr), C.byref(out)))

    def vec_update(self, vars_ptr, n, actions_ptr, step_ptr, second=False):
        """lob_vec_update: adds step[s] (f64 [n] at `step_ptr`) to each of the 96 weights of (row s, action[s]) -- the caller's whole
        per-tile amount, no alpha, no division by the tilings.  Rows as vec_features; private theta: book s's vector (the books' form)
        or book 0's (free-standing rows); second: theta_b (double Q).  Rows with an action out of range are skipped and counted
        (vec_status).  Enqueued on the engine's stream."""
        self._check(self.lib.lob_vec_update(self.h, C.c_void_p(vars_ptr), int(n), C.c_void_p(actions_ptr), C.c_void_p(step_ptr), 1 if second else 0))

    def vec_peek(self, mask, out):
        """lob_vec_peek: for every action whose bit is set in `mask` (abi.PEEK_ALL: all nine), what vec_step would write had every
        book been given that action now, into plane `action` of the device buffers of `out` (abi.VecPeekOut: obs f32 [9, B, V],
        reward f64 [9, B], terminal uint8 [9, B], stepped int32 [9, B]; 0 = not wanted) -- and nothing of the engine changes.  The
        planes of the other actions are not written.  One launch, enqueued on the engine's stream; works after snapshot_restore();
        refused on a ring-mode stream unless look_ring(True)."""
        self._check(self.lib.lob_vec_peek(self.h, int(mask), C.byref(out)))

    def vec_rollout(self, actions_ptr, n_plans, horizon, gamma, out):
        """lob_vec_rollout: for each of `n_plans` plans, what `horizon` consecutive vec_step calls would write from the books' present
        state, the h-th with the actions int32 [n_plans, horizon, B] at the DEVICE address `actions_ptr` -- into the device buffers of
        `out` (abi.VecRolloutOut: obs f32 [P, B, V] and terminal uint8 [P, B] behind the last step, reward f64 [P, H, B] of every
        step, stepped int32 [P, B] completed steps, ret f64 [P, B] the rewards discounted by `gamma` in [0, 1]; 0 = not wanted) --
        and nothing of the engine changes.  An action outside 0 .. 8 skips that step for that book and is not counted by
        vec_status.  One launch, enqueued on the engine's stream; works after snapshot_restore() and with the step log on; refused
        on a ring-mode stream unless look_ring(True).  With reward_measure NORMED and 1 < lb_pnl < horizon the first call (and one that needs more than
        any before) allocates the engine's workspace, which synchronises the device."""
        self._check(self.lib.lob_vec_rollout(self.h, C.c_void_p(actions_ptr), int(n_plans), int(horizon), float(gamma), C.byref(out)))

    def branch_fork(self, n_branches, out=None):
        """lob_branch_fork: (re)makes the engine's branch set -- `n_branches` (1 .. abi.MAX_BRANCHES) private copies of every book's
        present environment state, which stay on the device between calls.  `out` (abi.BranchOut or None: obs f32 [N, B, V], reward
        f64 [N, B], terminal uint8 [N, B], stepped int32 [N, B]; 0 = not wanted) receives the books' latest observation, their
        terminal word, reward 0 and stepped 0 in every plane.  Nothing of the engine changes.  Enqueued on the engine's stream; the
        first fork, and one that needs a larger set than any before, allocates, which synchronises the device.  Refused on a
        ring-mode stream unless look_ring(True)."""
        self._check(self.lib.lob_branch_fork(self.h, int(n_branches), None if out is None else C.byref(out)))

    def branch_step(self, actions_ptr, out):
        """lob_branch_step: one vec_step of every branch on its private state, branch n with the actions int32 [N, B] at the DEVICE
        address `actions_ptr`; `out` as in branch_fork: bit for bit what vec_step would write had the books been in the branch's
        state.  A branch that is over does not step (reward 0, its last observation); an action outside 0 .. 8 leaves the branch as
        it is and is not counted by vec_status.  One launch, enqueued on the engine's stream."""
        self._check(self.lib.lob_branch_step(self.h, C.c_void_p(actions_ptr), C.byref(out)))

    def branch_select(self, parent_ptr, out=None):
        """lob_branch_select: branch (n, b) becomes a copy of branch (parent[n, b], b) as it stood before the call (int32 [N, B] at
        the DEVICE address `parent_ptr`; outside 0 .. N - 1: keeps itself).  `out`: obs and terminal of the new arrangement are
        written, reward and stepped are not.  One launch; the first select allocates the second buffer, which synchronises the
        device."""
        self._check(self.lib.lob_branch_select(self.h, C.c_void_p(parent_ptr), None if out is None else C.byref(out)))

    def branch_close(self):
        """lob_branch_close: releases the branch set's buffers (waits for the engine's stream); close() does the same."""
        self._check(self.lib.lob_branch_close(self.h))

    def branch_book(self, out):
        """lob_branch_book: vec_book of every branch of the live set -- levels f32 [N, B, 4, depth], own f32 [N, B, 16], time_ms i64
        [N, B] at the device addresses of `out` (abi.VecBookOut; 0 = not wanted), branch-major: [n, b] is bit for bit what vec_book
        would write at [b] had the books been in branch n's state.  One launch on the engine's stream; nothing of the engine or of
        the set changes."""
        self._check(self.lib.lob_branch_book(self.h, C.byref(out)))

    def branch_history(self, K, out):
        """lob_branch_history: vec_history(K) of every branch of the live set -- levels f32 [N, B, K, 4, depth], trades f32 [N, B, K,
        2, max_trades], time_ms i32 [N, B, K], n_valid and rec i32 [N, B] at the device addresses of `out` (abi.VecHistOut; 0 = not
        wanted), branch-major: the window ends at the branch's own current record, within the book's own stream.  One launch on the
        engine's stream; nothing of the engine or of the set changes."""
        self._check(self.lib.lob_branch_history(self.h, int(K), C.byref(out)))

    def snapshot_save(self, slot, mask_ptr=None):
        """lob_snapshot_save: the environment state of the books selected by the DEVICE mask at address `mask_ptr` (uint8 [B],
        nonzero selects; None: every book, which (re)starts the slot) into snapshot slot `slot` (0 .. abi.MAX_SNAPSHOTS - 1);
        enqueued on the engine's stream.  The first save of a slot allocates its buffer."""
        self._check(self.lib.lob_snapshot_save(self.h, int(slot), mask_ptr))

    def snapshot_restore(self, slot, mask_ptr=None):
        """lob_snapshot_restore: the selected books continue exactly as they would have from the moment of the save; the others
        are not touched.  Enqueued on the engine's stream.  The learner calls are refused from here to the next reset()."""
        self._check(self.lib.lob_snapshot_restore(self.h, int(slot), mask_ptr))

    def snapshot_free(self, slot):
        """lob_snapshot_free: release the slot's buffer (an empty slot is fine)."""
        self._check(self.lib.lob_snapshot_free(self.h, int(slot)))

    def lob_stream(self):
        """lob_stream: the engine's hipStream_t as an integer."""
        return int(self.lib.lob_stream(self.h) or 0)

    # ---- learner ----
    def td_step(self, n=1):
        self._check(self.lib.lob_td_step(self.h, n))

    def td_step_begin(self):
        """First half of one learner step (action selection + performAction); a weight exchange fits before td_step_end."""
        self._check(self.lib.lob_td_step_begin(self.h))

    def td_step_end(self):
        self._check(self.lib.lob_td_step_end(self.h))

    def model_log_enable(self, on=True):
        """lob_model_log_enable: mean |delta| rows as the reference's `model_log` logger writes them (src/rl/agent.cpp:93-100)."""
        self._check(self.lib.lob_model_log_enable(self.h, 1 if on else 0))

    def model_log_read(self, cap=8192):
        rows = np.zeros(cap, np.float64)
        n, lost = C.c_int32(0), C.c_int64(0)
        self._check(self.lib.lob_model_log_read(self.h, _ptr(rows), cap, C.byref(n), C.byref(lost)))
        return rows[:n.value].copy(), int(lost.value)

    def td_split_supported(self):
        """Whether td_step_begin / td_step_end are available with this engine configuration (lob_td_split_supported)."""
        return bool(self.lib.lob_td_split_supported(self.h))

    def eval_step(self, n=1):
        self._check(self.lib.lob_eval_step(self.h, n))

    def handle_terminal(self):
        self._check(self.lib.lob_handle_terminal(self.h))

    def set_alpha(self, a):
        self._check(self.lib.lob_set_alpha(self.h, a))

    def set_epsilon(self, e):
        self._check(self.lib.lob_set_epsilon(self.h, e))

    def set_tau(self, t):
        self._check(self.lib.lob_set_tau(self.h, t))

    def features(self, vars_):
        v = np.ascontiguousarray(vars_, dtype=np.float32).reshape(-1, self.V)
        out = np.zeros((v.shape[0], 9, 96), np.int32)
        self._check(self.lib.lob_features(self.h, _ptr(v), v.shape[0], _ptr(out)))
        return out

    def q_values(self, vars_):
        v = np.ascontiguousarray(vars_, dtype=np.float32).reshape(-1, self.V)
        out = np.zeros((v.shape[0], 9), np.float64)
        self._check(self.lib.lob_q_values(self.h, _ptr(v), v.shape[0], _ptr(out)))
        return out

    def theta(self, which=0):
        out = np.zeros(self.M, np.float64)
        self._check(self.lib.lob_theta_get(self.h, which, _ptr(out), self.M))
        return out

    def set_theta(self, values, which=0):
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert v.shape == (self.M,)
        self._check(self.lib.lob_theta_set(self.h, which, _ptr(v), self.M))

    def _vec(self, fn, dtype):
        out = np.zeros(self.B, dtype)
        self._check(fn(self.h, _ptr(out)))
        return out

    def last_actions(self):
        return self._vec(self.lib.lob_get_last_actions, np.int32)

    def last_td(self):
        return self._vec(self.lib.lob_get_last_td, np.float64)

    def last_rewards(self):
        return self._vec(self.lib.lob_get_last_rewards, np.float64)

    def stepped(self):
        return self._vec(self.lib.lob_get_stepped, np.int32)

    def rng_counters(self):
        return self._vec(self.lib.lob_get_rng_counters, np.uint64)

    def learner_state(self):
        out = np.zeros((self.B, self.V), np.float32)
        self._check(self.lib.lob_get_learner_state(self.h, _ptr(out)))
        return out

    def traces(self, book):
        cap = 64 * 32  # LOB_TRACE_GENS generations of 32 tiles
        idx = np.zeros(cap, np.int32)
        e = np.zeros(cap, np.float32)
        n = C.c_int32()
        self._check(self.lib.lob_get_traces(self.h, book, _ptr(idx), _ptr(e), cap, C.byref(n)))
        return idx[:n.value].copy(), e[:n.value].copy()

    def counters(self):
        c = np.zeros(4, np.int64)
        self._check(self.lib.lob_get_counters(self.h, _ptr(c)))
        return c

    def path_stats(self):
        """lob_get_path_stats: which kernels served the books (diagnostics of the fast paths)."""
        c = np.zeros(8, np.int64)
        self._check(self.lib.lob_get_path_stats(self.h, _ptr(c)))
        return c

    def flow_stats(self):
        """lob_debug_flow (a diagnostic export, not in include/lob_engine.h): learner steps by the shape of their combined update."""
        c = np.zeros(8, np.int64)
        fn = self.lib.lob_debug_flow
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, _ptr(c)))
        return {"added_in_place": int(c[0]), "rest_on_side_stream": int(c[1]), "block_sums": int(c[2]), "every_book": int(c[3]),
                "act_inline_general": int(c[4]), "act_work_list_dense": int(c[5]), "act_work_list_other": int(c[6]),
                "dense_sums": int(c[7])}

    def launches(self):
        """lob_debug_launches (a diagnostic export): launches since lob_create of the kernels that share a timer name."""
        c = np.zeros(6, np.int64)
        fn = self.lib.lob_debug_launches
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, _ptr(c)))
        return {"env_step_kernel": int(c[0]), "env_step16_kernel": int(c[1]), "env_kernel_fused": int(c[2]),
                "learn_q_pair_kernel": int(c[3]), "learn_q_lane_kernel": int(c[4]), "learn_q_fast_kernel": int(c[5])}

    def track_cursor(self):
        """lob_debug_track_cursor (a diagnostic export): every book's cursor in events, the unit of track_window() -- int32 [B].  Waits."""
        k = np.zeros(self.B, np.int32)
        fn = self.lib.lob_debug_track_cursor
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, _ptr(k)))
        return k

    def hint_stats(self):
        """lob_debug_hint (a diagnostic export): learner steps that read the learn kernels' hand-back count, and of those the steps
        whose count had not arrived in time and that went by 0 instead (their act / update path was chosen by the host's timing)."""
        c = np.zeros(2, np.int64)
        fn = self.lib.lob_debug_hint
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, _ptr(c)))
        return {"hint_read": int(c[0]), "hint_missed": int(c[1])}

    def deferred_generations(self):
        """lob_debug_deferred (a diagnostic export): generations without a combine slot that trace_rest_kernel left to apply_kernel so far."""
        c = np.zeros(1, np.int64)
        fn = self.lib.lob_debug_deferred
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, _ptr(c)))
        return int(c[0])

    def fastpath_stats(self):
        """lob_debug_fastpath (a diagnostic export, not in include/lob_engine.h): written weights and the live books' hit-list lengths."""
        n = 4 + 257
        c = np.zeros(n, np.int64)
        fn = self.lib.lob_debug_fastpath
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]
        self._check(fn(self.h, _ptr(c), n))
        hist = c[4:]
        with_list = int(hist.sum())
        cum = np.cumsum(hist)
        def pct(q):
            return int(np.searchsorted(cum, q * with_list)) if with_list else None
        return {"written_weights": int(c[0]), "live_books": int(c[1]), "books_without_list": int(c[2]),
                "list_len_mean": round(float(c[3]) / with_list, 2) if with_list else None,
                "list_len_p50": pct(0.5), "list_len_p99": pct(0.99), "list_len_max": int(np.nonzero(hist)[0].max()) if with_list else None,
                "hist": hist}

    def fold_maps(self):
        """lob_debug_fold_maps (a diagnostic export): the pair learn kernel's written-weights maps after a stream synchronisation --
        exact map [M/32+1] u32, folded maps [2][M/32+1] u32, action masks [2][M] u16 (the padding of an odd M cut off), terms [2][9]."""
        M = int(self.M)
        words, mstride = M // 32 + 1, 2 * ((M + 1) // 2)
        nzx, nzd = np.zeros(words, np.uint32), np.zeros((2, words), np.uint32)
        nzm, terms = np.zeros((2, mstride), np.uint16), np.zeros((2, 9), np.uint32)
        fn = self.lib.lob_debug_fold_maps
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 5
        self._check(fn(self.h, _ptr(nzx), _ptr(nzd), _ptr(nzm), _ptr(terms)))
        return {"exact": nzx, "folded": nzd, "masks": nzm[:, :M], "terms": terms}

    # ---- multi-GPU weight exchange ----
    def delta_init(self):
        self._check(self.lib.lob_delta_init(self.h))

    def delta_begin(self):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self.lib.lob_delta_begin(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def delta_apply(self):
        self._check(self.lib.lob_delta_apply(self.h))

    # sparse exchange (include/lob_engine.h lob_delta_sparse_*): device pointers as ints
    def delta_sparse_supported(self):
        return bool(self.lib.lob_delta_sparse_supported(self.h))

    def delta_sparse_maps(self, world):
        own, gather, words = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self.lib.lob_delta_sparse_maps(self.h, int(world), C.byref(own), C.byref(gather), C.byref(words)))
        return own.value, gather.value, words.value

    def delta_sparse_pack(self, world):
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.lob_delta_sparse_pack(self.h, int(world), C.byref(p), C.byref(n)))
        return p.value, n.value

    def delta_sparse_apply(self):
        self._check(self.lib.lob_delta_sparse_apply(self.h))

    def exchange_debug(self):
        """lob_debug_exchange (a diagnostic export): sparse exchanges without / with a host synchronisation, unions that outgrew the fixed count."""
        c = np.zeros(5, np.int64)
        fn = self.lib.lob_debug_exchange
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, _ptr(c)))
        return {"without_host_sync": int(c[0]), "with_host_sync": int(c[1]), "unions_beyond_the_fixed_count": int(c[2]), "fixed_count": int(c[3]),
                "last_union": int(c[4])}

    def sync(self):
        self._check(self.lib.lob_sync(self.h))

    def kernel_timing(self, enable=True):
        """False / 0: off; True / 1: every launch; n > 1: the launches of every n-th step."""
        self._check(self.lib.lob_kernel_timing(self.h, int(enable)))

    def kernel_time_ms(self, name):
        ms = C.c_double()
        n = C.c_int64()
        self._check(self.lib.lob_kernel_time_ms(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value
