"""lob_vec_act / lob_vec_q: the engine's own Q values and policy actions, from device memory to device memory.

The yardsticks are the oracle (tests/oracle_lib.py: oracle_tiles, the oracle's weights, oracle_eval_step, oracle_td_step_begin) and
the getters the rest of the suite pins to it (lob_get_books, lob_get_state, lob_get_terminal, lob_get_rng_counters, lob_q_values,
lob_theta_get) -- never a second engine, never the kernel under test.  Everything is compared for equality.  The device buffers are
plain hipMalloc memory (no torch in this process: one HIP runtime per process, rl_markets_amd/abi.py); the torch-facing wrapper runs
in a process of its own (tests/vec_act_torch_child.py).

Three properties of the oracle shape the comparisons:
  * oracle_eval_step records the State the action was computed from (it calls new_state BEFORE the action, Backtester::_step), so
    its `vars` are compared with the observation the engine had BEFORE the step; the observation after it is compared with
    lob_get_state, and with the oracle's record one step later.
  * A step that runs out of data leaves the oracle's record of the book as it was (action, counter), although the action's draws
    were made.  For such a book the counter expected is the one before plus the draws Greedy::Sample makes on the expected values
    (one per tie met, a function of the row alone), and the action must lie among the row's maxima.
  * oracle_td_step_begin records nothing; oracle_td_step_end does, with the counter after the second half's draws.  The behaviour
    test uses Q(lambda) on learning.random_init weights, where the second half draws only to break ties, and asserts on the expected
    values that there are none.
Under shared theta the engine's weights after training are the oracle's up to the order of the f64 additions (tests/parity.py): the
expected values are then summed over lob_theta_get's weights, which are first compared with the oracle's at that tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from rl_markets_amd.engine import LobError
from tests import oracle_lib as ol
from tests.parity import assert_books_equal, compare_learner_step, dumps_to_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H2D, D2H = 1, 2
NA = abi.LOB_N_ACTIONS
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return _hip


class DevArray:
    """A device buffer with a numpy face: upload() / download() are whole-buffer hipMemcpy calls."""

    def __init__(self, shape, dtype, fill=0xAB):
        self.host = np.zeros(shape, dtype)
        p = C.c_void_p()
        assert hip().hipMalloc(C.byref(p), max(self.host.nbytes, 16)) == 0
        self.ptr = p.value
        assert hip().hipMemset(self.ptr, fill, max(self.host.nbytes, 16)) == 0   # (a value no output takes: an unwritten slot shows)

    def upload(self, a):
        a = np.ascontiguousarray(a, self.host.dtype).reshape(self.host.shape)
        assert hip().hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0

    def download(self):
        assert hip().hipMemcpy(self.host.ctypes.data_as(C.c_void_p), self.ptr, self.host.nbytes, D2H) == 0
        return self.host.copy()

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = None


class DevVec:
    """The five output buffers of lob_vec_step / lob_vec_observe."""

    def __init__(self, B, V):
        self.arr = {"obs": DevArray((B, V), np.float32), "reward": DevArray(B, np.float64), "terminal": DevArray(B, np.uint8),
                    "stepped": DevArray(B, np.int32), "n_live": DevArray(1, np.int32)}
        self.out = abi.VecOut(*[self.arr[k].ptr for k in ("obs", "reward", "terminal", "stepped", "n_live")])

    def read(self, eng):
        eng.sync()
        return {k: v.download() for k, v in self.arr.items()}

    def free(self):
        for v in self.arr.values():
            v.free()


class DevAct:
    """The two output buffers of lob_vec_act."""

    def __init__(self, B, want=("action", "q")):
        self.action, self.q = DevArray(B, np.int32), DevArray((B, NA), np.float64)
        self.out = abi.VecActOut(self.action.ptr if "action" in want else None, self.q.ptr if "q" in want else None)

    def read(self, eng):
        eng.sync()
        return self.action.download(), self.q.download()

    def free(self):
        self.action.free()
        self.q.free()


def make_params(algo=abi.ALGO_SARSA, theta_mode=abi.THETA_PRIVATE, mem=1 << 16, random_init=0):
    p = engine.default_params()
    p.depth, p.max_trades = 5, 2
    p.algo, p.theta_mode, p.memory_size, p.random_init = algo, theta_mode, mem, random_init
    return p


def gen(n_events, ending, p):
    """tests/test_gpu_vec_env.py's two endings: "dry", the data ends hours before the session does; "session", the clock starts 150
    events before the session's last half hour, so isTerminal() comes true in the middle of the data."""
    g = engine.default_gen_params()
    g.n_events = n_events
    if ending == "session":
        g.t0_ms = int(p.market.close_ms - 30 * 60000 - 150 * g.dt_ms)
    return g


def streams(p, B, n_events=300):
    """The first books end with the session, the rest run out of data: both endings in one batch (one book: the session's)."""
    n_dry = B // 2
    parts = [engine.gen_stream_host(gen(n_events, "session", p), p.depth, p.max_trades, 0, B - n_dry)]
    if n_dry:
        parts.append(engine.gen_stream_host(gen(n_events, "dry", p), p.depth, p.max_trades, B - n_dry, n_dry))
    return np.ascontiguousarray(np.concatenate(parts))


def make(B, p, n_events=300):
    rec = streams(p, B, n_events)
    eng = engine.Engine(p, B)
    eng.load_events(rec)
    return eng, ol.Oracle(p, rec)


def is_double(p):
    return p.algo in (abi.ALGO_DOUBLE_Q, abi.ALGO_DOUBLE_R_LEARN)


def weights(eng, orc, p, second=False):
    """The weight vector of every book's agent: [B] views (private theta) or one vector.  The oracle's; under shared theta the
    engine's own (lob_theta_get) when the two differ in the order of their additions -- after they have been compared."""
    B = eng.B
    get = orc.theta_b if second else orc.theta
    if p.theta_mode == abi.THETA_PRIVATE:
        return [get(b) for b in range(B)]
    mine, theirs = eng.theta(1 if second else 0), get(0)
    if np.array_equal(mine, theirs):
        return theirs
    np.testing.assert_allclose(mine, theirs, rtol=1e-9, atol=1e-12, err_msg="shared theta against the oracle's")
    return mine


def cpu_sum(p, obs, th):
    """tests/test_gpu_parity.py::test_q_values_bitwise's sum for every row: oracle_tiles, then the reference's order term by term
    (32 x w0, 32 x w1, 64 x w2: quirk Q3), each product rounded before it is added.  th: one vector, or one per row."""
    obs = np.ascontiguousarray(obs, np.float32)
    n, V = obs.shape
    f = np.zeros((n, NA, 96), np.int32)
    ol.load().oracle_tiles(p.memory_size, ol.ptr(obs), V, n, ol.ptr(f))
    vals = np.stack([th[i][f[i]] for i in range(n)]) if isinstance(th, list) else th[f]
    w = [float(x) for x in p.group_weights]
    Q = np.zeros((n, NA), np.float64)
    for k in range(32):
        Q = Q + w[0] * vals[:, :, k]
    for k in range(32, 64):
        Q = Q + w[1] * vals[:, :, k]
    for k in range(32, 96):
        Q = Q + w[2] * vals[:, :, k]
    return Q


def expected_q(eng, orc, p, obs):
    q = cpu_sum(p, obs, weights(eng, orc, p))
    if is_double(p):
        q = (q + cpu_sum(p, obs, weights(eng, orc, p, second=True))) / 2.0   # DoubleAgent::action
    return q


def greedy_draws(q):
    """Draws Greedy::Sample (policy.cpp:37-55) makes on each row: one for every value that equals the best so far."""
    best, n = q[:, 0].copy(), np.zeros(q.shape[0], np.uint64)
    for a in range(1, NA):
        n += (q[:, a] == best).astype(np.uint64)
        best = np.maximum(best, q[:, a])
    return n


def among_maxima(a, q):
    return q[np.arange(q.shape[0]), a] == q.max(axis=1)


# ---- 1. Q against the CPU -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta_mode", [abi.THETA_PRIVATE, abi.THETA_SHARED], ids=["private", "shared"])
@pytest.mark.parametrize("algo", [abi.ALGO_SARSA, abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q], ids=["sarsa", "qlambda", "double_q"])
def test_q_is_the_cpu_sum_and_argmax_touches_nothing(algo, theta_mode):
    B = 70
    p = make_params(algo, theta_mode)
    V = p.n_vars
    exact = theta_mode == abi.THETA_PRIVATE
    eng, orc = make(B, p)
    act = DevAct(B)
    eng.reset()
    orc.reset()
    eng.td_step(12)
    orc.td_step(12)
    compare_learner_step(eng, orc, "12 learner steps", exact=exact, rtol=0.0 if exact else 1e-9)
    recs = orc.recs()
    obs = recs["vars"][:, :V].copy()
    term = eng.get_terminal()
    np.testing.assert_array_equal(term, recs["book"]["terminal"])
    np.testing.assert_array_equal(eng.get_state()[term != 2], obs[term != 2], err_msg="the oracle's latest getState() is lob_get_state's row")
    ctr = eng.rng_counters().copy()
    eng.vec_act(abi.ACT_ARGMAX, act.out)
    a, q = act.read(eng)
    want = expected_q(eng, orc, p, obs)
    print("max |q| %.3g, rows with a non-zero value %d of %d" % (np.abs(want).max(), int((want != 0).any(axis=1).sum()), B))
    assert (want != 0).any(), "training has left weights behind: a condition on the inputs"
    np.testing.assert_array_equal(q.view(np.uint64), want.view(np.uint64), err_msg="q, bit for bit")
    np.testing.assert_array_equal(a, np.where(term == 0, want.argmax(axis=1), 0), err_msg="the first maximum of a live book, 0 elsewhere")
    np.testing.assert_array_equal(eng.rng_counters(), ctr, err_msg="LOB_ACT_ARGMAX draws nothing")
    for step in range(3):
        eng.td_step(1)
        orc.td_step(1)
        compare_learner_step(eng, orc, "learner step %d after lob_vec_act" % step, exact=exact, rtol=0.0 if exact else 1e-9)
    act.free()
    eng.close()
    orc.close()


# ---- 2. a greedy episode against oracle_eval_step -----------------------------------------------------------------------------------

def greedy_episode(eng, orc, p, dev, act, exp_ctr, obs, tag, cap=300):
    """lob_vec_act(GREEDY) + lob_vec_step(action) against oracle_eval_step(1), every step, until no book is live."""
    B, V = eng.B, p.n_vars
    th = (weights(eng, orc, p), weights(eng, orc, p, second=True) if is_double(p) else None)   # (nothing learns from here on)
    term = eng.get_terminal()
    steps, seen_dry, seen_over, drawn = 0, False, False, 0
    while (term == 0).any():
        assert steps < cap, tag + ": the episode did not end"
        t = "%s step %d" % (tag, steps)
        before = orc.counters()[0]
        live = term == 0
        eng.vec_act(abi.ACT_GREEDY, act.out)
        eng.vec_step(act.action.ptr, dev.out)
        orc.eval_step(1)
        a, q = act.read(eng)
        got = dev.read(eng)
        recs = orc.recs()
        want = cpu_sum(p, obs, th[0])
        if th[1] is not None:
            want = (want + cpu_sum(p, obs, th[1])) / 2.0
        np.testing.assert_array_equal(q.view(np.uint64), want.view(np.uint64), err_msg=t + ": q of every book, bit for bit")
        oterm = recs["book"]["terminal"]
        dry = live & (oterm == 2)          # performAction ran out of data: the oracle's record of the book stays as it was
        st = live & ~dry
        np.testing.assert_array_equal(got["stepped"].astype(bool), st, err_msg=t + ": stepped")
        np.testing.assert_array_equal(a[st], recs["action"][st], err_msg=t + ": action of the books that stepped")
        assert among_maxima(a[live], want[live]).all(), t + ": a greedy action is one of the maxima"
        assert (a[~live] == 0).all(), t + ": action of a book that is over"
        np.testing.assert_array_equal(obs[st], recs["vars"][st][:, :V], err_msg=t + ": the state the oracle acted on")
        exp_ctr = np.where(st, recs["rng_ctr"], exp_ctr + np.where(dry, greedy_draws(want), 0).astype(np.uint64))
        np.testing.assert_array_equal(eng.rng_counters(), exp_ctr, err_msg=t + ": rng counters of all books")
        drawn += int(greedy_draws(want)[live].sum())
        # obs, books, reward and terminal, as tests/test_gpu_vec_env.py check_step compares them
        assert_books_equal(dumps_to_np(eng.get_books()), recs["book"], t)
        term = eng.get_terminal()
        np.testing.assert_array_equal(got["terminal"], term, err_msg=t + ": terminal against lob_get_terminal")
        np.testing.assert_array_equal(got["terminal"], oterm, err_msg=t + ": terminal against the oracle")
        assert int(got["n_live"][0]) == int((term == 0).sum()), t + ": n_live"
        np.testing.assert_array_equal(got["obs"][term != 2], eng.get_state()[term != 2], err_msg=t + ": obs against lob_get_state")
        np.testing.assert_array_equal(got["reward"][st], recs["reward"][st], err_msg=t + ": reward of the stepped books")
        assert (got["reward"][~st].view(np.uint64) == 0).all(), t + ": reward of a book that did not step is +0.0"
        assert int(st.sum()) == int(orc.counters()[0] - before), t + ": stepped books against the oracle's step counter"
        seen_dry |= bool(dry.any())
        seen_over |= bool((~live).any() and st.any())
        obs = got["obs"]
        steps += 1
    assert eng.vec_status() == (abi.LOB_OK, 0), tag + ": no action was out of range"
    return steps, seen_dry, seen_over, drawn, term


SA, DQ, PRIV, SHARED = abi.ALGO_SARSA, abi.ALGO_DOUBLE_Q, abi.THETA_PRIVATE, abi.THETA_SHARED
EPISODES = [(70, algo, mode, start) for algo in (SA, DQ) for mode in (PRIV, SHARED) for start in ("zero", "random_init", "trained")]
EPISODES += [(1, SA, SHARED, "zero"), (1, SA, SHARED, "random_init"), (1, DQ, SHARED, "zero"), (1, DQ, PRIV, "trained")]   # one book


@pytest.mark.parametrize("B,algo,theta_mode,start", EPISODES,
                         ids=["B%d-%s-%s-%s" % (B, "sarsa" if a == SA else "double_q", "private" if m == PRIV else "shared", s) for B, a, m, s in EPISODES])
def test_greedy_episode_against_oracle_eval_step(B, algo, theta_mode, start):
    p = make_params(algo, theta_mode, random_init=1 if start == "random_init" else 0)
    V = p.n_vars
    eng, orc = make(B, p)
    dev, act = DevVec(B, V), DevAct(B)
    eng.reset()
    orc.reset()
    if start == "trained":
        exact = theta_mode == abi.THETA_PRIVATE
        eng.td_step(12)
        orc.td_step(12)
        compare_learner_step(eng, orc, "12 learner steps", exact=exact, rtol=0.0 if exact else 1e-9)
    recs = orc.recs()
    np.testing.assert_array_equal(eng.rng_counters(), recs["rng_ctr"])
    assert (eng.get_terminal() == 0).all(), "every book is live at the start: a condition on the inputs"
    tag = "B=%d algo=%d theta=%d %s" % (B, algo, theta_mode, start)
    steps, seen_dry, seen_over, drawn, term = greedy_episode(eng, orc, p, dev, act, recs["rng_ctr"].copy(), recs["vars"][:, :V].copy(), tag)
    print("%s: %d steps, %d draws" % (tag, steps, drawn))
    assert steps > 10
    if B > 1:
        assert seen_dry and seen_over and set(np.unique(term)) == {1, 2}, "books ended both ways, and were left alone while others stepped"
    if start == "zero":
        assert drawn >= 8 * steps, "all nine values tie: eight draws per book and step"
    dev.free()
    act.free()
    eng.close()
    orc.close()


# ---- 3. the behaviour policy against oracle_td_step_begin ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 7, 25])
@pytest.mark.parametrize("case", ["eps03", "eps0", "boltzmann"])
def test_behaviour_policy_against_oracle_td_step_begin(case, k):
    B = 70
    p = make_params(abi.ALGO_QLAMBDA, abi.THETA_PRIVATE, random_init=1)
    V = p.n_vars
    if case == "boltzmann":
        p.policy, p.tau = abi.POLICY_BOLTZMANN, 1.0
    else:
        p.epsilon = 0.3 if case == "eps03" else 0.0
    eng, orc = make(B, p)
    dev, act = DevVec(B, V), DevAct(B)
    eng.reset()
    orc.reset()
    eng.td_step(k)
    orc.td_step(k)
    compare_learner_step(eng, orc, "%d learner steps" % k)
    recs0 = orc.recs()
    obs = recs0["vars"][:, :V].copy()
    live = eng.get_terminal() == 0
    assert live.all(), "every book is still live: a condition on the inputs"
    want = expected_q(eng, orc, p, obs)
    eng.vec_act(abi.ACT_BEHAVIOUR, act.out)
    eng.vec_step(act.action.ptr, dev.out)
    orc.td_step_begin()
    a, q = act.read(eng)
    got = dev.read(eng)
    ctr = eng.rng_counters().copy()
    np.testing.assert_array_equal(q.view(np.uint64), want.view(np.uint64), err_msg="q, bit for bit")
    # the first half has drawn for the action only; the second half of Q(lambda) draws to break ties and for nothing else
    want_to = expected_q(eng, orc, p, got["obs"])
    assert (greedy_draws(want) == 0).all() and (greedy_draws(want_to) == 0).all(), "no ties on random_init weights: a condition on the inputs"
    orc.td_step_end()
    recs = orc.recs()
    st = got["stepped"].astype(bool)
    assert st.any() and int(st.sum()) == int(orc.counters()[0] - k * B), "stepped books against the oracle's step counter"
    np.testing.assert_array_equal(a[st], recs["action"][st], err_msg="the behaviour policy's action")
    np.testing.assert_array_equal(ctr, recs["rng_ctr"], err_msg="rng counters of all books")
    np.testing.assert_array_equal(got["obs"][st], recs["vars"][st][:, :V], err_msg="obs")
    assert_books_equal(dumps_to_np(eng.get_books()), recs["book"], "books")
    np.testing.assert_array_equal(got["reward"][st], recs["reward"][st], err_msg="reward")
    moved = ctr - recs0["rng_ctr"]
    if case == "eps0":
        assert (moved == 1).all(), "epsilon = 0: one draw more than greedy (the uniform), none for a tie"
        np.testing.assert_array_equal(a, want.argmax(axis=1), err_msg="epsilon = 0: the greedy action")
    elif case == "eps03":
        assert set(np.unique(moved)) == {1, 2}, "epsilon = 0.3: the uniform, and a second draw where it explores"
        np.testing.assert_array_equal(a[moved == 1], want.argmax(axis=1)[moved == 1])
    else:
        assert (moved == 1).all() and (a != want.argmax(axis=1)).any(), "Boltzmann: one uniform draw, and not the greedy policy"
    dev.free()
    act.free()
    eng.close()
    orc.close()


# ---- 4. the strided grid ------------------------------------------------------------------------------------------------------------

def test_more_states_than_the_grid_has_waves():
    """8 262 books: more than the 2 048 x 4 waves of the largest grid, and two books into a last partial block.  20 003 free-standing
    rows: the same for lob_vec_q, an odd count."""
    B, n = 8262, 20003
    p = make_params(abi.ALGO_SARSA, abi.THETA_SHARED)
    V = p.n_vars
    g = engine.default_gen_params()
    g.n_events = 200
    eng = engine.Engine(p, B)
    eng.gen_events(g)
    rng = np.random.default_rng(11)
    eng.set_theta(rng.standard_normal(p.memory_size))
    rows = rng.uniform(-12, 12, size=(n, V)).astype(np.float32)
    dv, dq = DevArray((n, V), np.float32), DevArray((n, NA), np.float64)
    dv.upload(rows)
    eng.vec_q(dv.ptr, n, dq.ptr)        # (before the first lob_reset: it needs none)
    eng.sync()
    np.testing.assert_array_equal(dq.download().view(np.uint64), eng.q_values(rows).view(np.uint64), err_msg="lob_vec_q against lob_q_values")
    eng.reset()
    act = DevAct(B)
    eng.vec_act(abi.ACT_ARGMAX, act.out)
    a, q = act.read(eng)
    term = eng.get_terminal()
    assert (term == 0).all()
    want = eng.q_values(eng.get_state())
    np.testing.assert_array_equal(q[term != 2].view(np.uint64), want[term != 2].view(np.uint64), err_msg="lob_vec_act's q against lob_q_values")
    np.testing.assert_array_equal(a, want.argmax(axis=1))
    assert len(np.unique(a)) > 1
    eng.vec_q(dv.ptr, n, dq.ptr)
    eng.sync()
    np.testing.assert_array_equal(dq.download().view(np.uint64), eng.q_values(rows).view(np.uint64), err_msg="lob_vec_q after the reset")
    for d in (dv, dq, act):
        d.free()
    eng.close()


# ---- 5. after a restore -------------------------------------------------------------------------------------------------------------

def test_the_policy_plays_on_restored_books():
    B = 70
    p = make_params(abi.ALGO_SARSA, abi.THETA_SHARED, random_init=1)
    V = p.n_vars
    eng, orc = make(B, p)
    dev, act = DevVec(B, V), DevAct(B)
    eng.reset()
    orc.reset()
    for step in range(4):
        eng.vec_act(abi.ACT_GREEDY, act.out)
        eng.vec_step(act.action.ptr, dev.out)
        orc.eval_step(1)
    eng.snapshot_save(0)
    assert_books_equal(dumps_to_np(eng.get_books()), orc.recs()["book"], "at the save")
    obs_saved, term_saved = dev.read(eng)["obs"], eng.get_terminal()
    for step in range(5):
        eng.vec_act(abi.ACT_GREEDY, act.out)
        eng.vec_step(act.action.ptr, dev.out)
    moved = dev.read(eng)["obs"]
    assert (moved != obs_saved).any(axis=1).sum() > B // 2, "the books have moved on since the save"
    eng.snapshot_restore(0)
    with pytest.raises(LobError) as ei:
        eng.eval_step(1)
    assert ei.value.code == abi.LOB_ESTATE, "lob_eval_step after a restore"
    eng.vec_observe(dev.out)
    np.testing.assert_array_equal(dev.read(eng)["obs"], obs_saved, err_msg="the restored observation")
    assert_books_equal(dumps_to_np(eng.get_books()), orc.recs()["book"], "the restored books are the oracle's at the save")
    eng.vec_act(abi.ACT_GREEDY, act.out)
    a, q = act.read(eng)
    want = expected_q(eng, orc, p, obs_saved)
    np.testing.assert_array_equal(q.view(np.uint64), want.view(np.uint64), err_msg="q on the restored observation")
    live = term_saved == 0
    assert live.any() and among_maxima(a[live], want[live]).all() and (a[~live] == 0).all()
    # ... and the oracle, which stands at the save, takes the same step
    eng.vec_step(act.action.ptr, dev.out)
    orc.env_step(a)
    got = dev.read(eng)
    assert_books_equal(dumps_to_np(eng.get_books()), orc.recs()["book"], "one step of the policy from the restored books")
    assert got["stepped"].sum() > 0 and eng.vec_status() == (abi.LOB_OK, 0)
    dev.free()
    act.free()
    eng.close()
    orc.close()


# ---- 6. contract --------------------------------------------------------------------------------------------------------------------

def test_state_rules_and_null_members():
    B = 70
    p = make_params(abi.ALGO_SARSA, abi.THETA_SHARED)   # (theta = 0: every greedy action draws eight times)
    eng, orc = make(B, p)
    lib = abi.load()
    act = DevAct(B)
    with pytest.raises(LobError) as ei:
        eng.vec_act(abi.ACT_GREEDY, act.out)
    assert ei.value.code == abi.LOB_ESTATE, "before lob_reset"
    eng.reset()
    orc.reset()
    for mode in (3, -1):
        assert lib.lob_vec_act(eng.h, mode, C.byref(act.out)) == abi.LOB_EINVAL
        assert b"lob_vec_act" in lib.lob_last_error()
    assert lib.lob_vec_act(eng.h, abi.ACT_GREEDY, None) == abi.LOB_EINVAL
    dv = DevArray((4, p.n_vars), np.float32)
    assert lib.lob_vec_q(eng.h, C.c_void_p(dv.ptr), 0, C.c_void_p(act.q.ptr)) == abi.LOB_EINVAL
    assert lib.lob_vec_q(eng.h, None, 4, C.c_void_p(act.q.ptr)) == abi.LOB_EINVAL
    assert lib.lob_vec_q(eng.h, C.c_void_p(dv.ptr), 4, None) == abi.LOB_EINVAL
    ctr = eng.rng_counters().copy()
    # both members NULL: LOB_OK, nothing launched, nothing written
    eng.kernel_timing(True)
    none = DevAct(B, want=())
    eng.vec_act(abi.ACT_GREEDY, none.out)
    eng.sync()
    assert eng.kernel_time_ms("vec_act_kernel")[1] == 0
    for arr in (none.action, none.q, act.action, act.q):
        assert (arr.download().view(np.uint8) == 0xAB).all(), "untouched"
    # action NULL: q is written, no counter moves in mode GREEDY
    only_q = DevAct(B, want=("q",))
    eng.vec_act(abi.ACT_GREEDY, only_q.out)
    _, q0 = only_q.read(eng)
    assert (only_q.action.download().view(np.uint8) == 0xAB).all()
    assert (q0 == 0.0).all(), "theta = 0"
    np.testing.assert_array_equal(eng.rng_counters(), ctr, err_msg="action == NULL: nothing is sampled")
    # q NULL: the action alone, the draws and the counters of the full call -- which the oracle's first greedy step makes
    only_a = DevAct(B, want=("action",))
    eng.vec_act(abi.ACT_GREEDY, only_a.out)
    a_only, _ = only_a.read(eng)
    assert (only_a.q.download().view(np.uint8) == 0xAB).all()
    orc.eval_step(1)
    recs = orc.recs()
    assert (recs["action"] >= 0).all(), "every book took the oracle's first step: a condition on the inputs"
    np.testing.assert_array_equal(a_only, recs["action"], err_msg="q == NULL: the action")
    np.testing.assert_array_equal(eng.rng_counters(), recs["rng_ctr"], err_msg="q == NULL: the counters")
    assert (eng.rng_counters() == ctr + 8).all(), "nine equal values: eight draws per book"
    assert len(np.unique(a_only)) > 1, "the ties are broken by the books' own streams"
    assert eng.kernel_time_ms("vec_act_kernel")[1] == 2
    eng.td_step_begin()
    with pytest.raises(LobError) as ei:
        eng.vec_act(abi.ACT_GREEDY, act.out)
    assert ei.value.code == abi.LOB_ESTATE, "between lob_td_step_begin and lob_td_step_end"
    eng.td_step_end()
    eng.vec_act(abi.ACT_BEHAVIOUR, act.out)
    eng.sync()
    for d in (act, none, only_q, only_a, dv):
        d.free()
    eng.close()
    orc.close()


# ---- the torch face -----------------------------------------------------------------------------------------------------------------

def test_vec_env_act_through_torch(tmp_path):
    """VecEnv.act() / VecEnv.q_values() at B = 70: tests/vec_act_torch_child.py plays env.step(env.act()) to the end of the episode
    in a fresh process of its own (torch must be imported before the engine library is loaded: one HIP runtime per process) and
    leaves what it saw in an .npz; the oracle's eval_step run of the same streams is compared with it here."""
    out = str(tmp_path / "vec_act.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vec_act_torch_child.py"), out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    sys.stdout.write(res.stdout[-4000:])
    assert res.returncode == 0, "vec_act_torch_child.py failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-4000:], res.stderr[-4000:])
    assert "vec act OK" in res.stdout
    z = np.load(out)
    B, V = 70, 8
    p = make_params(abi.ALGO_SARSA, abi.THETA_SHARED, random_init=1)
    assert p.n_vars == V
    orc = ol.Oracle(p, streams(p, B))
    orc.reset()
    actions, stepped = z["actions"], z["stepped"].astype(bool)
    assert actions.shape == stepped.shape and actions.shape[1] == B and actions.shape[0] > 10
    for k in range(actions.shape[0]):
        orc.eval_step(1)
        recs = orc.recs()
        before = stepped[k]
        np.testing.assert_array_equal(actions[k][before], recs["action"][before], err_msg="torch child, step %d: actions" % k)
    recs = orc.recs()
    assert (recs["book"]["terminal"] != 0).all(), "the child played to the end of the episode"
    assert_books_equal(np.frombuffer(z["books"].tobytes(), dtype=ol.BOOK_DTYPE), recs["book"], "torch child: final books")
    th = orc.theta(0)
    np.testing.assert_array_equal(z["q_values"].view(np.uint64), cpu_sum(p, z["obs"], th).view(np.uint64), err_msg="VecEnv.q_values of the final obs")
    np.testing.assert_array_equal(z["act_q"].view(np.uint64), z["q_values"].view(np.uint64), err_msg="act_q is q_values of the same obs")
    orc.close()
