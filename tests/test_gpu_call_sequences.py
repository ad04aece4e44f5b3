"""Random call sequences over the whole vector-env family against the model (tests/vec_model.py): the families driven against each
other in an order nobody chose -- a fork from books a masked restore revived, a select, a real step, a peek and a lob_reset onto
another day, a restore from a slot that is void by now, a fork that regrows the set, statistics in the middle of it all.

One engine per test.  tests/vec_sequences.py chooses every operation from the model's state alone; it is applied to the engine and
to the model, and then
  * the return code is the model's, and for a refusal lob_last_error() is the model's text; behind a refused call lob_get_books,
    the cheap getters, lob_get_counters and lob_vec_status give what they gave in front of it;
  * every output the call writes equals the model's, every element of every book, floats through their integer views;
  * every 8th operation and behind the last one the whole state is swept: lob_get_books and the getters against the model's books,
    lob_vec_observe, lob_vec_book, lob_vec_history, and every live branch's obs / terminal through an identity select.
The model's expectations come from the oracle alone (tests/test_vec_model.py pins the model on the CPU and asserts what the default
seeds cover).  A failure carries the seed, the variant and the operations up to it: tests/vec_sequences.py makes the same list
again without an engine.  Nothing here can reach a kernel with bad arguments: the refused calls are the ones the header documents
as refused on the host."""
import ctypes as C
import os

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests.parity import assert_books_equal, dumps_to_np
from tests.test_gpu_episode_stats import check_record
from tests.test_gpu_vec_book import DevBook
from tests.test_gpu_vec_env import DevArray, DevVec, hip
from tests.test_gpu_vec_history import DevHist
from tests.test_gpu_vec_peek import DevPeek
from tests.test_gpu_vec_rollout import Rolls
from tests.vec_history_expected import NAMES as HIST_NAMES, assert_record_has_dump_levels
from tests.vec_sequences import Sequence

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SEEDS = int(os.environ.get("LOB_SEQ_SEEDS", "24"))
SWEEP_EVERY = 8
vp = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(vp)


def same_bits(got, want, tag):
    """Equality of every element through the integer view: -0.0 is not +0.0, and a NaN equals itself."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (tag, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        view = {4: np.uint32, 8: np.uint64}.get(got.dtype.itemsize, np.uint8) if got.dtype.kind == "f" else got.dtype
        bad = np.argwhere(got.view(view) != want.view(view))
        i = tuple(bad[0])
        raise AssertionError("%s: differs at %s: engine %r, model %r (%d of %d elements)" % (tag, i, got[i], want[i], len(bad), got.size))


def unwritten(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xAB).all())


class DevBranchMax:
    """The word and output buffers of the branch calls, sized for LOB_MAX_BRANCHES whatever the set's N: an engine whose set had another
    N than the model's could not write past them.  One guard plane in front; behind the N planes everything must still hold the fill."""
    KEYS = ("obs", "reward", "terminal", "stepped")

    def __init__(self, B, V):
        NM = abi.MAX_BRANCHES
        self.B, self.NM = B, NM
        self.words = DevArray((NM, B), np.int32)
        self.arr = {"obs": DevArray((NM + 2, B, V), np.float32), "reward": DevArray((NM + 2, B), np.float64),
                    "terminal": DevArray((NM + 2, B), np.uint8), "stepped": DevArray((NM + 2, B), np.int32)}
        self.out = abi.BranchOut(*[self.arr[k].ptr + self.arr[k].host[0].nbytes for k in self.KEYS])

    def fill(self):
        for v in self.arr.values():
            assert hip().hipMemset(v.ptr, 0xAB, max(v.host.nbytes, 16)) == 0

    def upload(self, words):
        full = np.full((self.NM, self.B), -1, np.int32)   # (-1: no step, keep yourself)
        full[:words.shape[0]] = words
        self.words.upload(full)

    def read(self, eng, N):
        eng.sync()
        got = {}
        for k, v in self.arr.items():
            a = v.download()
            assert unwritten(a[0]) and unwritten(a[N + 1:]), "%s: a plane outside the set's %d was written" % (k, N)
            got[k] = a[1:N + 1]
        return got

    def free(self):
        self.words.free()
        for v in self.arr.values():
            v.free()


class Rig:
    """The engine of one sequence and the device buffers its calls are given."""

    def __init__(self, seq):
        self.seq, self.m, v = seq, seq.m, seq.v
        self.p = v.params()
        self.B, self.V, self.D, self.T = v.B, self.p.n_vars, self.p.depth, self.p.max_trades
        rec, days = v.data()
        self.eng = engine.Engine(self.p, self.B)
        if days is None:
            self.eng.load_events(rec)
        else:
            self.eng.load_days(days)
        self.lib, self.h = abi.load(), self.eng.h
        self.dev = DevVec(self.B, self.V)
        self.mask = DevArray(self.B, np.uint8)
        self.book = DevBook(self.B, self.D)
        self.hist = {}
        self.peek = DevPeek(self.B, self.V)
        self.rolls = Rolls(self.B, self.V)
        self.bufs = DevBranchMax(self.B, self.V)
        self.log_n = self.log_cap = 0

    def close(self):
        self.eng.sync()
        for d in [self.dev, self.mask, self.book, self.peek, self.rolls, self.bufs] + list(self.hist.values()):
            d.free()
        self.eng.close()

    def error(self):
        return self.lib.lob_last_error().decode()

    def mask_ptr(self, m):
        if m is None:
            return None
        self.mask.upload(np.asarray(m, np.uint8))
        return self.mask.ptr

    # ---- the calls: -> (return code, what the call wrote) ------------------------------------------------------------------------------
    def call(self, kind, a):
        lib, h, eng = self.lib, self.h, self.eng
        if kind == "reset":
            return lib.lob_reset(h), {}
        if kind == "days_set":
            return lib.lob_days_set(h, ptr(np.ascontiguousarray(a["days"], np.int32))), {}
        if kind == "days_select":
            return lib.lob_days_select(h, a["mode"], a["first"], a["n"]), {}
        if kind == "vec_step":
            steps = []
            for act in a["actions"]:
                self.dev.actions.upload(act)
                rc = lib.lob_vec_step(h, vp(self.dev.actions.ptr), C.byref(self.dev.out))
                if rc:
                    return rc, {}
                steps.append(self.dev.read(eng))
            return abi.LOB_OK, {"steps": steps}
        if kind == "observe":
            rc = lib.lob_vec_observe(h, C.byref(self.dev.out))
            return rc, ({} if rc else self.dev.read(eng))
        if kind == "status":
            n = C.c_int64(-1)
            return lib.lob_vec_status(h, C.byref(n)), {"n_bad": int(n.value)}
        if kind == "getters":
            state, reward, term = np.zeros((self.B, self.V), np.float32), np.zeros(self.B, np.float64), np.zeros(self.B, np.uint8)
            rcs = []
            for fn, out in (("lob_get_state", state), ("lob_get_reward", reward), ("lob_get_terminal", term)):
                rcs.append((fn, getattr(lib, fn)(h, ptr(out)), self.error()))
            if rcs[0][1]:
                return rcs[0][1], {"refusals": rcs}
            assert not rcs[1][1] and not rcs[2][1], rcs
            return abi.LOB_OK, {"books": dumps_to_np(eng.get_books()), "state": state, "reward": reward, "terminal": term,
                                "counters": np.array(eng.counters()[:2], np.int64)}
        if kind == "book":
            rc = lib.lob_vec_book(h, C.byref(self.book.out))
            return rc, ({} if rc else self.book.read(eng))
        if kind == "history":
            K = a["K"]
            if K not in self.hist:
                self.hist[K] = DevHist(self.B, K, self.D, self.T)
            self.hist[K].refill()
            rc = lib.lob_vec_history(h, K, C.byref(self.hist[K].out))
            return rc, ({} if rc else self.hist[K].read(eng))
        if kind == "peek":
            self.peek.fill()
            rc = lib.lob_vec_peek(h, a["mask"], C.byref(self.peek.out))
            return rc, self.peek.read(eng)
        if kind == "rollout":
            P, H, _ = a["plans"].shape
            d = self.rolls.get(P, H)
            d.fill()
            d.plans.upload(a["plans"])
            rc = lib.lob_vec_rollout(h, vp(d.plans.ptr), P, H, a["gamma"], C.byref(d.out))
            return rc, d.read(eng)
        if kind == "save":
            return lib.lob_snapshot_save(h, a["slot"], self.mask_ptr(a["mask"])), {}
        if kind == "restore":
            return lib.lob_snapshot_restore(h, a["slot"], self.mask_ptr(a["mask"])), {}
        if kind == "snapshot_free":
            return lib.lob_snapshot_free(h, a["slot"]), {}
        if kind == "fork":
            db = self.bufs
            db.fill()
            rc = lib.lob_branch_fork(h, a["N"], C.byref(db.out))
            return rc, db.read(eng, a["N"] if 1 <= a["N"] <= abi.MAX_BRANCHES else 0)
        if kind in ("bstep", "select"):
            words = a["actions" if kind == "bstep" else "parent"]
            db = self.bufs
            db.fill()
            db.upload(words)
            rc = (lib.lob_branch_step if kind == "bstep" else lib.lob_branch_select)(h, vp(db.words.ptr), C.byref(db.out))
            return rc, db.read(eng, 0 if rc else words.shape[0])
        if kind == "close":
            return lib.lob_branch_close(h), {}
        if kind == "stats":
            out, n = np.zeros(1 + max(self.m.n_days, 1), engine.EPISODE_STATS_DTYPE), C.c_int32(0)
            rc = lib.lob_episode_stats(h, 1 if a["by_day"] else 0, ptr(out), len(out), C.byref(n))
            return rc, {"records": out[:n.value]}
        if kind == "log_enable":
            sel = a["sel"]
            n = self.B if sel is None else len(sel)
            rc = lib.lob_step_log_enable(h, None if sel is None or n == 0 else ptr(np.ascontiguousarray(sel, np.int32)), n, a["cap"])
            if rc == abi.LOB_OK:
                self.log_n, self.log_cap = n, a["cap"] if n else 0
            return rc, {}
        if kind == "log_counts":
            rows, lost = np.zeros(max(self.log_n, 1), np.int32), np.zeros(max(self.log_n, 1), np.int32)
            rc = lib.lob_step_log_counts(h, ptr(rows), ptr(lost))
            return rc, {"n_rows": rows[:self.log_n], "n_lost": lost[:self.log_n]}
        if kind == "log_read":
            n, cap = max(self.log_n, 1), max(self.log_cap, 1)
            out = np.zeros((n, cap), engine.STEP_ROW_DTYPE)
            rc = lib.lob_step_log_read(h, 0, n, 0, cap, ptr(out))
            return rc, {"rows": out[:self.log_n, :self.log_cap]}
        if kind == "clear_inventory":
            return lib.lob_clear_inventory(h), {}
        if kind in ("td_step", "eval_step", "td_begin", "td_end"):
            rc = {"td_step": lambda: lib.lob_td_step(h, a["n"]), "eval_step": lambda: lib.lob_eval_step(h, a["n"]),
                  "td_begin": lambda: lib.lob_td_step_begin(h), "td_end": lambda: lib.lob_td_step_end(h)}[kind]()
            if rc or kind == "td_begin":
                return rc, {}
            return rc, {"books": dumps_to_np(eng.get_books()), "stepped": eng.stepped(), "action": eng.last_actions(), "reward": eng.last_rewards(),
                        "td": eng.last_td(), "rng": eng.rng_counters(), "vars": eng.learner_state()}
        raise AssertionError("no such operation: " + kind)

    # ---- the comparisons --------------------------------------------------------------------------------------------------------------
    def step_like(self, got, want, tag, keys=("obs", "reward", "terminal", "stepped")):
        for k in keys:
            same_bits(got[k], want[k].astype(got[k].dtype), "%s: %s" % (tag, k))

    def compare(self, kind, a, got, want, tag):
        w = want.out
        if kind == "vec_step":
            assert len(got["steps"]) == len(w["steps"])
            for k, (g, e) in enumerate(zip(got["steps"], w["steps"])):
                self.step_like(g, e, "%s call %d" % (tag, k), ("obs", "reward", "terminal", "stepped", "n_live"))
        elif kind == "observe":
            self.step_like(got, w, tag, ("obs", "terminal", "stepped", "n_live"))
            same_bits(got["reward"][w["reward_books"]], w["reward"][w["reward_books"]], tag + ": reward where terminal != 2")
        elif kind == "status":
            assert got["n_bad"] == w["n_bad"], "%s: %d actions out of range, the model counts %d" % (tag, got["n_bad"], w["n_bad"])
        elif kind == "getters":
            assert_books_equal(got["books"], w["books"], tag + ": lob_get_books")
            m = w["books_compared"]
            same_bits(got["state"][m], w["state"][m], tag + ": lob_get_state where terminal != 2")
            same_bits(got["reward"][m], w["reward"][m], tag + ": lob_get_reward where terminal != 2")
            same_bits(got["terminal"], w["terminal"], tag + ": lob_get_terminal")
            same_bits(got["counters"], w["counters"], tag + ": lob_get_counters [0], [1]")
        elif kind == "book":
            for k in ("levels", "own", "time_ms"):
                same_bits(got[k], w[k], "%s: %s" % (tag, k))
        elif kind == "history":
            dump, rec = w["dump"], got["rec"]
            flat, start, length = self.m.source()
            assert ((rec >= -1) & (rec < length)).all(), tag + ": rec within the book's stream"
            strong = dump["terminal"] != 2
            same_bits(rec[strong], (dump["cursor"][strong] - 1).astype(np.int32), tag + ": rec against cursor - 1 where terminal != 2")
            assert_record_has_dump_levels(flat, start, rec, dump, self.D, tag + ": record rec against the model's book")
            exp = self.m.history_expected(a["K"], rec)
            for k in HIST_NAMES:
                same_bits(got[k], exp[k], "%s: %s" % (tag, k))
        elif kind == "peek":
            for p in range(abi.LOB_N_ACTIONS):
                if p in w["planes"]:
                    self.step_like({k: v[p] for k, v in got.items()}, {k: w[k][p] for k in got}, "%s plane %d" % (tag, p))
                else:
                    assert all(unwritten(v[p]) for v in got.values()), "%s: plane %d is not in the mask and was written" % (tag, p)
        elif kind == "rollout":
            self.step_like(got, w, tag, ("obs", "reward", "terminal", "stepped", "ret"))
        elif kind in ("fork", "bstep"):
            self.step_like(got, w, tag)
        elif kind == "select":
            self.step_like(got, w, tag, ("obs", "terminal"))
            assert unwritten(got["reward"]) and unwritten(got["stepped"]), tag + ": select writes no reward / stepped"
        elif kind == "stats":
            rec, books, ids = got["records"], w["books"], w["ids"]
            check_record(rec[0], books, ids, -1, tag + " whole")
            if w["days"] is not None:
                assert len(rec) == 1 + self.m.n_days, tag
                for d in range(self.m.n_days):
                    sel = w["days"] == d
                    check_record(rec[1 + d], books[sel], ids[sel], d, "%s day %d" % (tag, d))
            else:
                assert len(rec) == 1, tag
        elif kind == "log_counts":
            same_bits(got["n_rows"], w["n_rows"], tag + ": stored rows")
            same_bits(got["n_lost"], w["n_lost"], tag + ": lost rows")
        elif kind == "log_read":
            assert got["rows"].shape == w["rows"].shape, tag
            for j in range(got["rows"].shape[0]):
                for k in range(got["rows"].shape[1]):
                    assert got["rows"][j, k].tobytes() == w["rows"][j, k].tobytes(), "%s: selected book %d row %d:\n  log   %r\n  model %r" % (
                        tag, j, k, got["rows"][j, k], w["rows"][j, k])
        elif kind in ("td_step", "eval_step", "td_end"):
            assert_books_equal(got["books"], w["books"], tag + ": lob_get_books")
            st = w["stepped"].astype(bool)
            same_bits(got["action"][st], w["action"][st].astype(got["action"].dtype), tag + ": actions")
            same_bits(got["books"]["n_traces"], w["books"]["n_traces"], tag + ": n_traces")
            same_bits(got["stepped"], w["stepped"].astype(got["stepped"].dtype), tag + ": lob_get_stepped")
            same_bits(got["rng"], w["rng"].astype(got["rng"].dtype), tag + ": random counters")
            same_bits(got["reward"][st], w["reward"][st], tag + ": rewards")
            if kind != "eval_step":   # (a greedy step records the state its action was chosen in and has no TD error)
                same_bits(got["vars"][st], w["vars"][st], tag + ": learner state")
                same_bits(got["td"][st], w["td"][st], tag + ": TD errors")

    def cheap_state(self):
        """What must be the same in front of and behind a refused call."""
        rc, n = self.eng.vec_status()
        s = {"status": (rc, n), "books": bytes(self.eng.get_books()), "counters": tuple(self.eng.counters()),
             "state": self.eng.get_state().tobytes(), "reward": self.eng.get_reward().tobytes(), "terminal": self.eng.get_terminal().tobytes()}
        return s

    def do(self, kind, a, want, tag):
        """The call on the engine (the model is behind it already), compared with `want`."""
        m = self.m
        watch = want.refused and m.was_reset
        if watch:
            before = self.cheap_state()
            assert before["status"][1] == m.n_bad, "%s: %d actions out of range in front of the call, the model counts %d" % (tag, before["status"][1], m.n_bad)
            m.n_bad = 0   # (lob_vec_status has cleared the engine's word)
        rc, got = self.call(kind, a)
        text = self.error()
        assert rc == want.rc, "%s: return code %d (%s), the model says %d (%s)" % (tag, rc, text if rc else "", want.rc, want.err)
        if want.refused:
            if kind == "getters":
                for fn, rc_fn, text_fn in got["refusals"]:
                    assert rc_fn == want.rc and text_fn == fn + want.err[len("lob_get_state"):], "%s: %s: %d (%s)" % (tag, fn, rc_fn, text_fn)
            else:
                assert text == want.err, "%s: lob_last_error() is\n  %s\nthe model says\n  %s" % (tag, text, want.err)
                assert all(unwritten(v) for k, v in got.items() if isinstance(v, np.ndarray) and kind in ("peek", "rollout", "fork", "bstep", "select")), \
                    tag + ": a refused call wrote"
            if watch:
                after = self.cheap_state()
                assert after["status"] == (abi.LOB_OK, 0), "%s: lob_vec_status behind a refused call: %s" % (tag, after["status"])
                for k in ("books", "counters", "state", "reward", "terminal"):
                    assert after[k] == before[k], "%s: a refused call changed %s" % (tag, k)
            return
        self.compare(kind, a, got, want, tag)

    def sweep(self, tag):
        m = self.m
        if not m.was_reset or m.half_open:
            return 0
        todo = [("getters", {}), ("observe", {}), ("book", {}), ("history", {"K": 3})]
        if m.branch == "live":   # an identity select changes nothing: every live branch's obs / terminal
            todo.append(("select", {"parent": np.broadcast_to(np.arange(m.N, dtype=np.int32)[:, None], (m.N, m.B)).copy()}))
        for kind, a in todo:
            self.do(kind, a, m.apply(kind, **a), "%s sweep %s" % (tag, kind))
        return len(todo)


COUNTS = {"ops": 0, "refused": 0, "sweep_ops": 0, "sequences": 0}


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_call_sequence(seed, monkeypatch):
    seq = Sequence(seed)
    if seq.v.env16_off:
        monkeypatch.setenv("LOB_ENV16_MAX", "0")
    rig = Rig(seq)
    where = "seed %d (%s)" % (seed, seq.v.label())
    try:
        i = -1
        for i, kind, a, want in seq:
            rig.do(kind, a, want, "%s op %d %s" % (where, i, kind))
            COUNTS["ops"] += 1
            COUNTS["refused"] += want.refused
            if (i + 1) % SWEEP_EVERY == 0 or i == seq.length - 1:
                COUNTS["sweep_ops"] += rig.sweep("%s behind op %d" % (where, i))
    except Exception as e:
        raise AssertionError("%s failed at op %d: %s\nthe operations up to it (tests/vec_sequences.py makes them again):\n  %s" % (
            where, i, e, "\n  ".join("%3d %s" % (k, line) for k, line in enumerate(seq.log)))) from e
    finally:
        rig.close()
        seq.m.close()
    COUNTS["sequences"] += 1
    assert rig.eng.h is None


def test_zz_what_ran():
    print("call sequences: %s" % COUNTS)
