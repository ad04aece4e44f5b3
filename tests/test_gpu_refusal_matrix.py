"""Which call is legal in which engine state: the return code and the whole text of lob_last_error() of every entry point that checks
the engine's state, in each of five states -- before the first lob_reset, after it, between lob_td_step_begin and lob_td_step_end,
after a lob_snapshot_restore, and on a stream whose market track is a ring.

The table below is the contract of include/lob_engine.h as the library spoke it before the state checks were gathered into one
guard (lob_engine_impl.h); it was written from that source and run against that library.  A legal call runs with all-NULL output
structs or one row, so nothing here is about what the calls compute: the per-family tests are (test_return_codes, test_refusals,
test_state_rules_and_null_members, test_call_sequence_errors)."""
import ctypes as C

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests.test_gpu_days import make_days
from tests.test_gpu_vec_env import DevArray, gen, make_params

pytestmark = pytest.mark.gpu
B, N_EVENTS = 4, 300
STATES = ("fresh", "reset", "mid", "restored", "ring")

OK = None
R = ": call lob_reset first"
H = ": a learner step is half done (lob_td_step_begin without lob_td_step_end)"
S = ": books were put back by lob_snapshot_restore in this episode; the learner runs again after the next lob_reset"
G = ": the market track of this stream is a ring (longer than LOB_TRACK_RING events)"
GB = G + ": entries before the cursor are gone, no earlier state can be served"
OFF = ": the step log is off (lob_step_log_enable)"
NOLIB = ": no day library loaded (lob_load_days)"
NOSTEP = ": no step begun"

# row: (case, function, the refusal behind the function's name per state -- OK: LOB_OK); every refusal is LOB_ESTATE
#                                                     fresh   reset   mid     restored ring
TABLE = [
    ("lob_step",                 "lob_step",             (R,     OK,     H,      OK,      OK)),
    ("lob_vec_step",             "lob_vec_step",         (R,     OK,     H,      OK,      OK)),
    ("lob_vec_observe",          "lob_vec_observe",      (R,     OK,     H,      OK,      OK)),
    ("lob_vec_book",             "lob_vec_book",         (R,     OK,     H,      OK,      OK)),
    ("lob_vec_history",          "lob_vec_history",      (R,     OK,     H,      OK,      OK)),
    ("lob_vec_act",              "lob_vec_act",          (R,     OK,     H,      OK,      OK)),
    ("lob_vec_peek",             "lob_vec_peek",         (R,     OK,     H,      OK,      G)),
    ("lob_vec_rollout",          "lob_vec_rollout",      (R,     OK,     H,      OK,      G)),
    ("lob_vec_features books",   "lob_vec_features",     (R,     OK,     H,      OK,      OK)),
    ("lob_vec_features rows",    "lob_vec_features",     (OK,    OK,     H,      OK,      OK)),
    ("lob_vec_update books",     "lob_vec_update",       (R,     OK,     H,      OK,      OK)),
    ("lob_vec_update rows",      "lob_vec_update",       (OK,    OK,     H,      OK,      OK)),
    ("lob_snapshot_save",        "lob_snapshot_save",    (R,     OK,     H,      OK,      GB)),
    ("lob_snapshot_restore",     "lob_snapshot_restore", (R,     OK,     H,      OK,      GB)),
    ("lob_get_state",            "lob_get_state",        (R,     OK,     OK,     OK,      OK)),
    ("lob_get_reward",           "lob_get_reward",       (R,     OK,     OK,     OK,      OK)),
    ("lob_get_terminal",         "lob_get_terminal",     (R,     OK,     OK,     OK,      OK)),
    ("lob_clear_inventory",      "lob_clear_inventory",  (R,     OK,     H,      OK,      OK)),
    ("lob_episode_stats",        "lob_episode_stats",    (R,     OK,     H,      OK,      OK)),
    ("lob_td_step",              "lob_td_step",          (R,     OK,     ": a step is half done (lob_td_step_begin without lob_td_step_end)", S, OK)),
    ("lob_td_step_begin",        "lob_td_step_begin",    (R,     OK,     ": the previous step has not been ended", S, OK)),
    ("lob_td_step_end",          "lob_td_step_end",      (R,     NOSTEP, OK,     NOSTEP,  NOSTEP)),
    ("lob_eval_step",            "lob_eval_step",        (R,     OK,     ": a learner step is half done", S, OK)),
    ("lob_handle_terminal",      "lob_handle_terminal",  (OK,    OK,     H,      S,       OK)),
    ("lob_theta_set",            "lob_theta_set",        (OK,    OK,     H,      OK,      OK)),
    ("lob_step_log_enable",      "lob_step_log_enable",  (OK,    OK,     H,      OK,      OK)),
    ("lob_step_log_counts off",  "lob_step_log_counts",  (OFF,   OFF,    OFF,    OFF,     OFF)),
    ("lob_step_log_read off",    "lob_step_log_read",    (OFF,   OFF,    OFF,    OFF,     OFF)),
    ("lob_step_log_counts on",   "lob_step_log_counts",  (OK,    OK,     H,      OK,      OK)),
    ("lob_step_log_read on",     "lob_step_log_read",    (OK,    OK,     H,      OK,      OK)),
    ("lob_days_select no lib",   "lob_days_select",      (NOLIB, NOLIB,  NOLIB,  NOLIB,   NOLIB)),
    ("lob_days_set no lib",      "lob_days_set",         (NOLIB, NOLIB,  NOLIB,  NOLIB,   NOLIB)),
]


class Rig:
    """One engine of B books with its stream loaded, and the few buffers the calls are given."""

    def __init__(self):
        self.p = make_params(5, 2)
        self.V = self.p.n_vars
        self.rec = engine.gen_stream_host(gen(N_EVENTS, "dry", self.p), self.p.depth, self.p.max_trades, 0, B)
        self.eng = engine.Engine(self.p, B)
        self.eng.load_events(self.rec)
        self.lib, self.h = abi.load(), self.eng.h
        self.actions = DevArray(B, np.int32, fill=0)            # action 0 for every book; also the one plan of lob_vec_rollout
        self.rows = DevArray((1, self.V), np.float32, fill=0)   # one free-standing state
        self.step0 = DevArray(B, np.float64, fill=0)            # increments of 0.0: lob_vec_update writes nothing
        self.host_i32 = np.zeros(B, np.int32)
        self.host_f64 = np.zeros(max(B, 1), np.float64)
        self.host_f32 = np.zeros((B, self.V), np.float32)
        self.host_u8 = np.zeros(B, np.uint8)
        self.stats = np.zeros(1, engine.EPISODE_STATS_DTYPE)
        self.row = np.zeros(1, engine.STEP_ROW_DTYPE)
        self.n = C.c_int32(0)

    def ptr(self, a):
        return a.ctypes.data_as(C.c_void_p)

    def log(self, on):
        rc = self.lib.lob_step_log_enable(self.h, None, B if on else 0, 4)
        assert rc == abi.LOB_OK, self.lib.lob_last_error()

    def enter(self, state, log_on):
        """The engine in `state`, whatever the call before left behind.  The step log is off unless the case wants it on; it goes on
        in front of a lob_td_step_begin (refused behind it) and behind a lob_snapshot_restore (refused while the log is on)."""
        if state == "fresh":
            self.eng.load_events(self.rec)   # (a stream just loaded has seen no lob_reset)
            self.log(log_on)
            return
        self.eng.reset()   # (ends a half-done step and the restored state; "ring": a reset engine whose stream outgrows the ring)
        self.log(log_on and state != "restored")
        if state in ("reset", "restored"):
            self.eng.snapshot_save(0)        # (so that a lob_snapshot_restore finds its slot)
        if state == "mid":
            self.eng.td_step_begin()
        if state == "restored":
            self.eng.snapshot_restore(0)
            self.log(log_on)

    def call(self, case):
        lib, h, vp = self.lib, self.h, C.c_void_p
        books = case.endswith("books")
        rows, n = (None, B) if books else (vp(self.rows.ptr), 1)
        calls = {
            "lob_step": lambda: lib.lob_step(h, self.ptr(self.host_i32)),
            "lob_vec_step": lambda: lib.lob_vec_step(h, vp(self.actions.ptr), C.byref(abi.VecOut())),
            "lob_vec_observe": lambda: lib.lob_vec_observe(h, C.byref(abi.VecOut())),
            "lob_vec_book": lambda: lib.lob_vec_book(h, C.byref(abi.VecBookOut())),
            "lob_vec_history": lambda: lib.lob_vec_history(h, 1, C.byref(abi.VecHistOut())),
            "lob_vec_act": lambda: lib.lob_vec_act(h, abi.ACT_ARGMAX, C.byref(abi.VecActOut())),
            "lob_vec_peek": lambda: lib.lob_vec_peek(h, abi.PEEK_ALL, C.byref(abi.VecPeekOut())),
            "lob_vec_rollout": lambda: lib.lob_vec_rollout(h, vp(self.actions.ptr), 1, 1, 1.0, C.byref(abi.VecRolloutOut())),
            "lob_vec_features": lambda: lib.lob_vec_features(h, rows, n, None, C.byref(abi.VecFeatOut())),
            "lob_vec_update": lambda: lib.lob_vec_update(h, rows, n, vp(self.actions.ptr), vp(self.step0.ptr), 0),
            "lob_snapshot_save": lambda: lib.lob_snapshot_save(h, 0, None),
            "lob_snapshot_restore": lambda: lib.lob_snapshot_restore(h, 0, None),
            "lob_get_state": lambda: lib.lob_get_state(h, self.ptr(self.host_f32)),
            "lob_get_reward": lambda: lib.lob_get_reward(h, self.ptr(self.host_f64)),
            "lob_get_terminal": lambda: lib.lob_get_terminal(h, self.ptr(self.host_u8)),
            "lob_clear_inventory": lambda: lib.lob_clear_inventory(h),
            "lob_episode_stats": lambda: lib.lob_episode_stats(h, 0, self.ptr(self.stats), 1, C.byref(self.n)),
            "lob_td_step": lambda: lib.lob_td_step(h, 1),
            "lob_td_step_begin": lambda: lib.lob_td_step_begin(h),
            "lob_td_step_end": lambda: lib.lob_td_step_end(h),
            "lob_eval_step": lambda: lib.lob_eval_step(h, 1),
            "lob_handle_terminal": lambda: lib.lob_handle_terminal(h),
            "lob_theta_set": lambda: lib.lob_theta_set(h, 0, self.ptr(self.host_f64), 1),
            "lob_step_log_enable": lambda: lib.lob_step_log_enable(h, None, B, 4),
            "lob_step_log_counts": lambda: lib.lob_step_log_counts(h, self.ptr(self.host_i32), None),
            "lob_step_log_read": lambda: lib.lob_step_log_read(h, 0, 1, 0, 1, self.ptr(self.row)),
            "lob_days_select": lambda: lib.lob_days_select(h, abi.DAYS_RANDOM, 0, 1),
            "lob_days_set": lambda: lib.lob_days_set(h, self.ptr(self.host_i32)),
        }
        return calls[case.split()[0]]()

    def close(self):
        self.eng.sync()
        for d in (self.actions, self.rows, self.step0):
            d.free()
        self.eng.close()


@pytest.mark.parametrize("state", STATES)
def test_refusal_matrix(state, monkeypatch):
    if state == "ring":   # (tests/test_gpu_snapshot.py's switches: the 300 events are more than the ring holds)
        monkeypatch.setenv("LOB_TRACK_RING", "256")
        monkeypatch.setenv("LOB_TRACK_REFILL", "16")
    rig = Rig()
    if state == "mid" and not rig.eng.td_split_supported():
        rig.close()
        return
    col = STATES.index(state)
    wrong = []
    for case, fn, expect in TABLE:
        rig.enter(state, case.endswith(" on"))
        rc = rig.call(case)
        text = rig.lib.lob_last_error().decode()
        want = expect[col]
        if want is OK:
            if rc != abi.LOB_OK:
                wrong.append("%s, %s: %d (%s), expected LOB_OK" % (case, state, rc, text))
        elif rc != abi.LOB_ESTATE or text != fn + want:
            wrong.append("%s, %s: %d (%s), expected LOB_ESTATE (%s)" % (case, state, rc, text, fn + want))
    rig.close()
    assert not wrong, "\n".join(wrong)


def test_day_selection_in_a_half_done_step():
    """lob_days_select / lob_days_set with a library loaded: legal before the first lob_reset and after it, refused inside a step."""
    p = make_params(5, 2)
    eng = engine.Engine(p, B)
    eng.load_days(make_days([N_EVENTS, N_EVENTS]))
    lib, days = abi.load(), np.zeros(B, np.int32)
    sel = lambda: lib.lob_days_select(eng.h, abi.DAYS_IN_ORDER, 0, 2)
    put = lambda: lib.lob_days_set(eng.h, days.ctypes.data_as(C.c_void_p))
    assert sel() == abi.LOB_OK and put() == abi.LOB_OK, lib.lob_last_error()
    eng.reset()
    assert sel() == abi.LOB_OK and put() == abi.LOB_OK, lib.lob_last_error()
    if eng.td_split_supported():
        eng.td_step_begin()
        assert sel() == abi.LOB_ESTATE and lib.lob_last_error().decode() == "lob_days_select" + H
        assert put() == abi.LOB_ESTATE and lib.lob_last_error().decode() == "lob_days_set" + H
        eng.td_step_end()
    eng.sync()
    eng.close()
