"""A model of the whole vector-env interface (include/lob_engine.h) on the CPU, for sequence tests: every call of
the lob_vec_* / lob_snapshot_* / lob_branch_* families, the episode statistics, the step log, the day selection and the learner steps
is applied to it as an operation, and it answers with the return code, the text of lob_last_error() for a refusal, and every output
the call writes.  It imports the oracle (tests/oracle_lib.py) and never the engine library.  Not collected by pytest; used by
tests/vec_sequences.py, tests/test_vec_model.py and tests/test_gpu_call_sequences.py.

What a book is.  The environment side is deterministic and independent per book, so the state of any book -- real, saved in a
snapshot slot, imagined in a branch -- is a function of what that book has played: its days and its actions.  NOT of the present
episode alone: the reference's window accumulators keep their sums across Initialise (quirk Q7, oracle/lob_oracle.cpp Accumulator::
clear), the two windows of the agent's own PnL among them, so the state behind the second lob_reset depends on where the first
episode stood when it ended -- on the restored state, if books had been put back.  A journal of "the day and the actions since
lob_reset" replayed on a FRESH oracle is therefore right in an engine's first episode only.  The model keeps the books themselves
instead of their journals: oracle_copy_books (pinned against a replay, bit for bit, by tests/test_vec_model.py) copies the environment
side of a book between oracles, which is exactly what the header says a snapshot holds and a branch is.

  real      one batched oracle with private weights: lob_vec_step is oracle_env_step (an action out of range skips the book), the
            learner calls are the oracle's own, in lock step, so the actions a learner step took are in the same books.
  slots     four oracles of B books; save copies real -> slot under the mask, restore copies back and leaves the learner alone.
  branches  two oracles of N * B books whose roles swap at every select, as the engine's two buffers do; a fork with a larger N
            makes larger ones.
  look-ahead  lob_vec_peek / lob_vec_rollout: copies of the real books in a scratch oracle, stepped there.  No expectation of a
            look-ahead or a branch call ever comes from an engine call.

What is compared where the header leaves a choice (the callers follow `out` as the model gives it):
  * lob_get_state, lob_get_reward and the obs / reward of lob_vec_observe are evaluated from the environment as it stands
    (oracle_state_now), not taken from the last record: after lob_clear_inventory the position has moved.  For a book that is out of
    data (terminal 2) obs is the state of its last completed step, and its state / reward getters are left out (the header pins them
    "wherever terminal != 2").
  * the cumulative counters: [0] steps and [1] events, which a restore does not wind back and no look-ahead or branch step moves;
    [2] and [3] are the learner's and are not modelled.
  * lob_vec_history's `rec` of a book that is out of data is the engine's own, pinned by the levels of that record (as
    tests/test_gpu_vec_history.py does); everywhere else it is cursor - 1.
  * between lob_td_step_begin and lob_td_step_end nothing is compared but the refusals: the header does not say what the getters
    show there.
  * the observation a call writes for a book it does not step is "the state of its last completed step" (Model.latest): behind
    lob_eval_step that is the state behind the step, as the engine has it, not the oracle's record, which holds the state the greedy
    action was chosen in (the Backtester's order).
The learner phase: private weights, where the engine is exact.  Learner calls are legal until a lob_snapshot_restore and again after
the next lob_reset; the model lets the oracle's learner run on through both (the copy leaves it alone, as the header says the restore
does).  The premise that oracle_env_step with the learner's recorded actions reproduces its books holds for every field of every
book that has data left (tests/test_vec_model.py); a learner step that runs dry records no action, which is why the learner steps in
the very oracle that holds the books.  A lob_clear_inventory refreshes the engine's latest getState() (the position has moved), and
the model's with it."""
import numpy as np

from rl_markets_amd import abi
from rl_markets_amd.engine import STEP_ROW_DTYPE
from tests import days_ref
from tests import oracle_lib as ol
from tests.test_gpu_step_log import Expect
from tests.test_gpu_vec_book import expected as book_expected
from tests.test_gpu_vec_rollout import ret_of
from tests.vec_history_expected import expected_history

NA = abi.LOB_N_ACTIONS
OK, EINVAL, ESTATE = abi.LOB_OK, abi.LOB_EINVAL, abi.LOB_ESTATE

# the refusal texts behind the function's name (tests/test_gpu_refusal_matrix.py is their source)
R = ": call lob_reset first"
H = ": a learner step is half done (lob_td_step_begin without lob_td_step_end)"
S = ": books were put back by lob_snapshot_restore in this episode; the learner runs again after the next lob_reset"
OFF = ": the step log is off (lob_step_log_enable)"
NOLIB = ": no day library loaded (lob_load_days)"
NOSTEP = ": no step begun"
NOSET = ": no live branch set (lob_branch_fork makes one; lob_reset and lob_branch_close void it)"
MASKED_SAVE = "lob_snapshot_save: a masked save needs a slot that holds a full save (NULL mask) of this episode"
LOG_ON = ("lob_snapshot_restore: the step log is enabled (a row is due where total_ticks > n_rows + n_lost: total_ticks cannot go back "
          "under it)")
BY_DAY = "lob_episode_stats: by_day without an episode on a day library (lob_load_days, a selection, lob_reset)"

# the entry point behind every operation kind (the name in front of a refusal's text)
FN = {"reset": "lob_reset", "days_set": "lob_days_set", "days_select": "lob_days_select", "vec_step": "lob_vec_step",
      "observe": "lob_vec_observe", "status": "lob_vec_status", "getters": "lob_get_state", "book": "lob_vec_book",
      "history": "lob_vec_history", "peek": "lob_vec_peek", "rollout": "lob_vec_rollout", "save": "lob_snapshot_save",
      "restore": "lob_snapshot_restore", "snapshot_free": "lob_snapshot_free", "fork": "lob_branch_fork", "bstep": "lob_branch_step",
      "select": "lob_branch_select", "close": "lob_branch_close", "stats": "lob_episode_stats", "log_enable": "lob_step_log_enable",
      "log_counts": "lob_step_log_counts", "log_read": "lob_step_log_read", "clear_inventory": "lob_clear_inventory",
      "td_step": "lob_td_step", "eval_step": "lob_eval_step", "td_begin": "lob_td_step_begin", "td_end": "lob_td_step_end"}
KINDS = tuple(FN)
# kinds whose guard wants a lob_reset / a whole step (lob_engine_impl.h `needs`)
NEEDS_RESET = {"vec_step", "observe", "getters", "book", "history", "peek", "rollout", "save", "restore", "fork", "bstep", "select",
               "stats", "clear_inventory", "td_step", "eval_step", "td_begin", "td_end"}
NEEDS_WHOLE = {"vec_step", "observe", "book", "history", "peek", "rollout", "save", "restore", "fork", "bstep", "select", "stats",
               "clear_inventory", "log_enable", "log_counts", "log_read", "days_set", "days_select"}
HALF_TEXT = {"td_step": ": a step is half done (lob_td_step_begin without lob_td_step_end)",
             "td_begin": ": the previous step has not been ended", "eval_step": ": a learner step is half done"}


class Result:
    """What one call must give: the return code, lob_last_error() for a refusal (None: not compared), and the outputs by name."""

    def __init__(self, rc=OK, err=None, **out):
        self.rc, self.err, self.out, self.refused = rc, err, out, False

    def __repr__(self):
        return "Result(rc=%d, err=%r, out=%s)" % (self.rc, self.err, sorted(self.out))


def plus_zero(reward, stepped):
    """The reward of a book that did not step is +0.0."""
    return np.where(stepped.astype(bool), reward, np.float64(0.0))


class Model:
    """`params`: the engine's parameters (private weights).  `records`: uint32 [B][n][W], the stream every book plays -- or, with
    `days` (a list of uint32 [n_d][W]), any stream of the right shape, never played: the days come by days_set / days_select."""

    def __init__(self, params, B, records=None, days=None):
        assert params.theta_mode == abi.THETA_PRIVATE
        self.p, self.B, self.V, self.D, self.T = params, B, params.n_vars, params.depth, params.max_trades
        self.lib = ol.DayLibrary(days) if days is not None else None
        self.n_days = len(days) if days is not None else 0
        if days is not None:
            records = np.stack([days[0]] * B)
        self.records = np.ascontiguousarray(records, dtype=np.uint32)
        self.n_events = self.records.shape[1]
        self.real = ol.Oracle(params, self.records)
        # the other oracles only ever step environments: one weight vector, and a stream that is never played (a copy brings its own)
        self.p_env = abi.Params.from_buffer_copy(bytes(params))
        self.p_env.theta_mode, self.p_env.memory_size = abi.THETA_SHARED, 1 << 10
        self.slot = [None] * abi.MAX_SNAPSHOTS
        self.slot_state = ["empty"] * abi.MAX_SNAPSHOTS   # empty / full / void (after lob_reset)
        self.bo, self.cur, self.N, self.branch = [None, None], 0, 0, "none"   # none / live / void
        self.scratch = None
        self.was_reset = self.restored = self.half_open = False
        self.episode = 0
        self.n_bad = 0
        self.steps = self.events = 0                       # lob_get_counters [0], [1]
        self.log_n, self.log_sel, self.log_cap, self.log_armed, self.log = 0, None, 0, False, None
        self.day_cur, self.day_next = None, None
        self.day_x = [days_ref.seed_state(int(params.seed) + int(params.book_id_offset) + b) for b in range(B)]
        self._recs = None
        # the observation of every book's last completed step (or of the reset): what a call writes for a book it does not step.  Not
        # the oracle's record: lob_eval_step records the state its action was chosen in (the Backtester's order), the engine keeps
        # the state behind the step.
        self.latest = None
        self.slot_latest = [None] * abi.MAX_SNAPSHOTS
        self.b_latest = [None, None]

    def close(self):
        for o in [self.real, self.scratch] + self.slot + self.bo:
            if o is not None:
                o.close()

    # ---- views of the real books -------------------------------------------------------------------------------------------------
    def recs(self):
        if self._recs is None:
            self._recs = self.real.recs()
        return self._recs

    def terminal(self):
        return self.recs()["book"]["terminal"].astype(np.uint8)

    def books(self):
        return self.recs()["book"]

    def rec_vars(self):
        return np.ascontiguousarray(self.recs()["vars"][:, :self.V])

    def source(self):
        """(flat records, first record of every book's stream, its length): what lob_vec_history indexes."""
        if self.lib is not None:
            return self.lib.records, self.lib.day_first[self.day_cur], self.lib.day_len[self.day_cur].astype(np.int64)
        return self.records.reshape(self.B * self.n_events, -1), np.arange(self.B, dtype=np.int64) * self.n_events, np.full(self.B, self.n_events, np.int64)

    def history_expected(self, K, rec):
        flat, start, length = self.source()
        return expected_history(flat, start, length, rec, K, self.D, self.T)

    def _env_oracle(self, n_books):
        return ol.Oracle(self.p_env, np.zeros((n_books, 2, self.records.shape[2]), np.uint32))

    def _scratch(self, n_books):
        if self.scratch is None or self.scratch.B < n_books:
            if self.scratch is not None:
                self.scratch.close()
            self.scratch = self._env_oracle(n_books)
        return self.scratch

    # ---- the guard ------------------------------------------------------------------------------------------------------------------
    def refusal(self, kind, **a):
        """The Result of the refusal the contract has for this call in the present state, or None: the call is legal."""
        fn = FN[kind]
        # argument checks stand in front of the guard
        if kind in ("save", "restore", "snapshot_free") and not 0 <= a["slot"] < abi.MAX_SNAPSHOTS:
            return Result(EINVAL, "%s: slot %d is outside [0, %d)" % (fn, a["slot"], abi.MAX_SNAPSHOTS))
        if kind == "fork" and not 1 <= a["N"] <= abi.MAX_BRANCHES:
            return Result(EINVAL, "%s: n_branches = %d is outside [1, %d]" % (fn, a["N"], abi.MAX_BRANCHES))
        if kind in ("days_set", "days_select") and self.lib is None:
            return Result(ESTATE, fn + NOLIB)
        if kind in ("log_counts", "log_read") and not self.log_n:
            return Result(ESTATE, fn + OFF)
        if kind in NEEDS_RESET and not self.was_reset:
            return Result(ESTATE, fn + R)
        if kind == "td_end":
            return None if self.half_open else Result(ESTATE, fn + NOSTEP)
        if self.half_open and kind in HALF_TEXT:
            return Result(ESTATE, fn + HALF_TEXT[kind])
        if self.half_open and kind in NEEDS_WHOLE:
            return Result(ESTATE, fn + H)
        if kind in ("td_step", "eval_step", "td_begin") and self.restored:
            return Result(ESTATE, fn + S)
        if kind == "save" and a["mask"] is not None and self.slot_state[a["slot"]] != "full":
            return Result(ESTATE, MASKED_SAVE)
        if kind == "restore":
            if self.log_n:
                return Result(ESTATE, LOG_ON)
            if self.slot_state[a["slot"]] != "full":
                return Result(ESTATE, "lob_snapshot_restore: slot %d holds no save of this episode" % a["slot"])
        if kind in ("bstep", "select") and self.branch != "live":
            return Result(ESTATE, fn + NOSET)
        if kind == "stats" and a["by_day"] and (self.lib is None or self.day_cur is None):
            return Result(ESTATE, BY_DAY)
        return None

    # ---- the operations -------------------------------------------------------------------------------------------------------------
    def apply(self, kind, **a):
        ref = self.refusal(kind, **a)
        if ref is not None:
            ref.refused = True
            return ref
        out = getattr(self, "_" + kind)(**a)
        return out if isinstance(out, Result) else Result(OK, None, **(out or {}))

    def _touch(self):
        self._recs = None

    def _real_moves(self, fn):
        """Run a call that steps the real books; the cumulative counters follow it."""
        before = self.real.counters()
        fn()
        after = self.real.counters()
        self.steps += int(after[0] - before[0])
        self.events += int(after[1] - before[1])
        self._touch()

    def _log_step(self):
        if self.log_armed:
            self.log.after_step(self.books()[self.log_sel])

    def _reset(self):
        if self.day_next is not None:
            self.day_cur, self.day_next = self.day_next, None
            self.real.set_days(*self.lib.of(self.day_cur))
        assert self.lib is None or self.day_cur is not None, "a day selection stands in front of the first lob_reset on a library"
        self._real_moves(self.real.reset)
        self.was_reset, self.half_open, self.restored = True, False, False
        self.episode += 1
        self.n_bad = 0
        self.slot_state = ["void" if s == "full" else s for s in self.slot_state]
        if self.branch == "live":
            self.branch = "void"
        if self.log_n:
            self.log_armed, self.log = True, Expect(self.books()[self.log_sel])
        self.latest = self.rec_vars()

    def _days_set(self, days):
        self.day_next = np.asarray(days, dtype=np.int32).copy()

    def _days_select(self, mode, first, n):
        if mode == abi.DAYS_IN_ORDER:
            self.day_next = (first + (int(self.p.book_id_offset) + np.arange(self.B)) % n).astype(np.int32)
        else:
            nxt = np.zeros(self.B, np.int32)
            for b in range(self.B):
                self.day_x[b], v = days_ref.draw(self.day_x[b], n)
                nxt[b] = first + v
            self.day_next = nxt

    def _step_outputs(self, o, term_before, actions, n_books, latest):
        """obs / reward / terminal / stepped of the first n_books books of oracle `o` behind an oracle_env_step with `actions`;
        `latest`: their observations in front of it, which a book that does not step keeps."""
        r = o.recs()[:n_books]
        term = r["book"]["terminal"].astype(np.uint8)
        in_range = (actions >= 0) & (actions < NA)
        stepped = ((term_before == 0) & in_range & (term != 2)).astype(np.int32)
        obs = np.where(stepped.astype(bool)[:, None], r["vars"][:, :self.V], latest).astype(np.float32)
        return {"obs": np.ascontiguousarray(obs), "reward": plus_zero(r["reward"], stepped), "terminal": term, "stepped": stepped}

    def _vec_step(self, actions):
        """actions [k][B]: k consecutive lob_vec_step calls; the outputs of every one."""
        steps = []
        for a in np.asarray(actions, np.int32).reshape(-1, self.B):
            before = self.terminal()
            self._real_moves(lambda: self.real.env_step(a))
            self.n_bad += int(((a < 0) | (a >= NA)).sum())
            out = self._step_outputs(self.real, before, a, self.B, self.latest)
            self.latest = out["obs"]
            out["n_live"] = np.array([(out["terminal"] == 0).sum()], np.int32)
            self._log_step()
            steps.append(out)
        return {"steps": steps}

    def state_now(self):
        """(lob_get_state, lob_get_reward, the books they are compared on: terminal != 2)"""
        v, r = self.real.state_now()
        return np.ascontiguousarray(v[:, :self.V]), r, self.terminal() != 2

    def _observe(self):
        v, r, not2 = self.state_now()
        term = self.terminal()
        return {"obs": np.where(not2[:, None], v, self.latest), "reward": r, "reward_books": not2, "terminal": term,
                "stepped": np.zeros(self.B, np.int32), "n_live": np.array([(term == 0).sum()], np.int32)}

    def _status(self):
        n, self.n_bad = self.n_bad, 0
        return Result(EINVAL if n else OK, None, n_bad=n)

    def _getters(self):
        v, r, not2 = self.state_now()
        return {"books": self.books(), "state": v, "reward": r, "books_compared": not2, "terminal": self.terminal(),
                "counters": np.array([self.steps, self.events], np.int64)}

    def _book(self):
        return book_expected(self.books(), self.D)

    def _history(self, K):
        return {"dump": self.books(), "K": K}

    def _copies(self, o, planes):
        """The real books copied into planes [0, planes) of oracle `o`."""
        idx = np.arange(planes * self.B, dtype=np.int32)
        o.copy_books(idx, self.real, idx % self.B)

    def _peek(self, mask):
        o = self._scratch(NA * self.B)
        self._copies(o, NA)
        acts = np.repeat(np.array([a if mask >> a & 1 else -1 for a in range(NA)], np.int32), self.B)
        pad = np.full(o.B, -1, np.int32)
        pad[:NA * self.B] = acts
        o.env_step(pad)
        out = self._step_outputs(o, np.tile(self.terminal(), NA), acts, NA * self.B, np.tile(self.latest, (NA, 1)))
        out = {k: v.reshape((NA, self.B) + v.shape[1:]) for k, v in out.items()}
        out["planes"] = np.array([a for a in range(NA) if mask >> a & 1])
        return out

    def _rollout(self, plans, gamma):
        plans = np.asarray(plans, np.int32)
        P, Hn, B = plans.shape
        o = self._scratch(P * B)
        self._copies(o, P)
        reward, stepped = np.zeros((P, Hn, B), np.float64), np.zeros((P, B), np.int32)
        term, latest = np.tile(self.terminal(), P), np.tile(self.latest, (P, 1))
        for h in range(Hn):
            acts = plans[:, h].reshape(-1)
            pad = np.full(o.B, -1, np.int32)
            pad[:P * B] = acts
            o.env_step(pad)
            got = self._step_outputs(o, term, acts, P * B, latest)
            reward[:, h], term, latest = got["reward"].reshape(P, B), got["terminal"], got["obs"]
            stepped += got["stepped"].reshape(P, B)
        return {"obs": got["obs"].reshape(P, B, self.V), "reward": reward, "terminal": term.reshape(P, B), "stepped": stepped,
                "ret": ret_of(reward, gamma)}

    def _books_of(self, mask):
        return np.arange(self.B, dtype=np.int32) if mask is None else np.flatnonzero(np.asarray(mask) != 0).astype(np.int32)

    def _save(self, slot, mask):
        if self.slot[slot] is None:
            self.slot[slot] = self._env_oracle(self.B)
        idx = self._books_of(mask)
        self.slot[slot].copy_books(idx, self.real, idx)
        if self.slot_latest[slot] is None:
            self.slot_latest[slot] = np.zeros((self.B, self.V), np.float32)
        self.slot_latest[slot][idx] = self.latest[idx]
        self.slot_state[slot] = "full"

    def _restore(self, slot, mask):
        idx = self._books_of(mask)
        before = self.terminal()
        self.real.copy_books(idx, self.slot[slot], idx)
        self.latest = self.latest.copy()
        self.latest[idx] = self.slot_latest[slot][idx]
        self.restored = True
        self._touch()
        return {"revived": int(((before != 0) & (self.terminal() == 0)).sum())}

    def _snapshot_free(self, slot):
        self.slot_state[slot] = "empty"

    def _branch_recs(self):
        return self.bo[self.cur].recs()[:self.N * self.B]

    def branch_view(self):
        """obs [N][B][V] and terminal [N][B] of the live set."""
        r = self._branch_recs()
        return {"obs": np.ascontiguousarray(self.b_latest[self.cur]).reshape(self.N, self.B, self.V),
                "terminal": r["book"]["terminal"].astype(np.uint8).reshape(self.N, self.B)}

    def _reserve(self, which, n_books):
        """Room for n_books in buffer `which`; True when a smaller one had to be replaced (the engine's regrowth)."""
        grown = self.bo[which] is not None and self.bo[which].B < n_books
        if grown:
            self.bo[which].close()
        if grown or self.bo[which] is None:
            self.bo[which] = self._env_oracle(n_books)
        return grown

    def _fork(self, N):
        grown = self._reserve(self.cur, N * self.B)
        self._copies(self.bo[self.cur], N)
        self.N, self.branch = N, "live"
        self.b_latest[self.cur] = np.tile(self.latest, (N, 1))
        out = self.branch_view()
        out.update(reward=np.zeros((N, self.B), np.float64), stepped=np.zeros((N, self.B), np.int32), grown=grown)
        return out

    def _bstep(self, actions):
        actions = np.asarray(actions, np.int32)
        assert actions.shape == (self.N, self.B), (actions.shape, self.N, self.B)
        o = self.bo[self.cur]
        before = self._branch_recs()["book"]["terminal"].astype(np.uint8)
        pad = np.full(o.B, -1, np.int32)
        pad[:self.N * self.B] = actions.reshape(-1)
        o.env_step(pad)
        out = self._step_outputs(o, before, actions.reshape(-1), self.N * self.B, self.b_latest[self.cur])
        self.b_latest[self.cur] = out["obs"]
        out = {k: v.reshape((self.N, self.B) + v.shape[1:]) for k, v in out.items()}
        out["some_over_some_live"] = bool((before != 0).any() and (before == 0).any())
        return out

    def _select(self, parent):
        parent = np.asarray(parent, np.int32)
        assert parent.shape == (self.N, self.B)
        own = np.arange(self.N, dtype=np.int64)[:, None]
        eff = np.where((parent >= 0) & (parent < self.N), parent.astype(np.int64), own)
        to = self.cur ^ 1
        self._reserve(to, self.N * self.B)
        cols = np.arange(self.B, dtype=np.int64)[None, :]
        self.bo[to].copy_books((own * self.B + cols).reshape(-1), self.bo[self.cur], (eff * self.B + cols).reshape(-1))
        self.b_latest[to] = self.b_latest[self.cur][(eff * self.B + cols).reshape(-1)]
        self.cur = to
        out = self.branch_view()
        out["differs_between_books"] = bool((eff != eff[:, :1]).any())
        return out

    def _close(self):
        self.branch = "none"
        for i in (0, 1):
            if self.bo[i] is not None:
                self.bo[i].close()
                self.bo[i] = None

    def _stats(self, by_day):
        return {"books": self.books(), "days": self.day_cur if by_day else None,
                "ids": int(self.p.book_id_offset) + np.arange(self.B, dtype=np.int64)}

    def _log_enable(self, sel, cap):
        """sel: None (every book), an ascending list of books, or an empty list (off)."""
        sel = np.arange(self.B, dtype=np.int32) if sel is None else np.asarray(sel, np.int32)
        self.log_n, self.log_sel, self.log_cap = int(len(sel)), sel, int(cap) if len(sel) else 0
        self.log_armed, self.log = False, None   # (recording starts with the next lob_reset)

    def _log_rows(self):
        rows = self.log.rows if self.log_armed else [[] for _ in range(self.log_n)]
        want = np.array([len(r) for r in rows], np.int32)
        stored = np.minimum(want, self.log_cap).astype(np.int32)
        table = np.zeros((self.log_n, self.log_cap), STEP_ROW_DTYPE)
        for j, r in enumerate(rows):
            for k in range(int(stored[j])):
                table[j, k] = r[k]
        return stored, (want - stored).astype(np.int32), table

    def _log_counts(self):
        stored, lost, _ = self._log_rows()
        return {"n_rows": stored, "n_lost": lost}

    def _log_read(self):
        return {"rows": self._log_rows()[2]}

    def _clear_inventory(self):
        self.real.clear_inventory()
        self._touch()
        v, _, not2 = self.state_now()   # (the position has moved: the engine refreshes its latest getState(), which lob_eval_step acts on)
        self.latest = np.where(not2[:, None], v, self.latest).astype(np.float32)

    def _learner_outputs(self, before):
        r = self.recs()
        term = r["book"]["terminal"].astype(np.uint8)
        stepped = (before == 0) & (term != 2)
        self.latest = np.where(stepped[:, None], self.state_now()[0], self.latest).astype(np.float32)   # (the state behind the step)
        return {"books": r["book"], "stepped": stepped.astype(np.int32), "action": r["action"], "reward": r["reward"], "td": r["td"],
                "rng": r["rng_ctr"], "vars": np.ascontiguousarray(r["vars"][:, :self.V])}

    def _td_step(self, n):
        out = {}
        for _ in range(n):
            before = self.terminal()
            self._real_moves(lambda: self.real.td_step(1))
            self._log_step()
            out = self._learner_outputs(before)
        return out

    def _eval_step(self, n):
        out = {}
        for _ in range(n):
            before = self.terminal()
            self._real_moves(lambda: self.real.eval_step(1))
            self._log_step()
            out = self._learner_outputs(before)
        out.pop("td", None)
        return out

    def _td_begin(self):
        self._half_before = (self.terminal(), self.real.counters())
        self.real.td_step_begin()
        self.half_open = True
        self._touch()

    def _td_end(self):
        before, c0 = self._half_before
        self.real.td_step_end()
        c1 = self.real.counters()
        self.steps += int(c1[0] - c0[0])
        self.events += int(c1[1] - c0[1])
        self.half_open = False
        self._touch()
        self._log_step()
        return self._learner_outputs(before)
