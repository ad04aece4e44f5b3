"""The look-ahead family -- lob_vec_peek, lob_vec_rollout, lob_branch_fork / _step / _select, lob_branch_book / _history -- at the edges
of what lob_create accepts.  tests/test_gpu_edges.py takes the learner and the env step there; this file takes the private step of
rl_markets_amd/csrc/lob_peek.h, which restates half of a step over registers:

  1. depth x trade slots, one step      D in {1, 2, 4, 6, 7, 9, 10} (rows that are no multiple of 16 bytes), T = 1 (the <true> form with one
                                        slot) and T in {3, 5, 8} (step_event<LOB_MAX_TRADES>), on hardened streams with a dry tail: the
                                        real step against the oracle at every step, peek against the nine real steps, under both
                                        env-step forms of the yardstick
  2. depth x trade slots, several steps roll-out (P = 3, H = 6, padded plans, an action out of range) against the composed route; a
                                        branch set of 3 against the roll-out and the real steps, with a select; lob_branch_book /
                                        _history against lob_vec_book / _history of the real books stepped from a snapshot
  3. eight keys                         merged trade lists of exactly eight keys inside peek, roll-out and branch steps
  4. the PnL window against the horizon roll_rm_prep's three sources of the replaced entry: lb_pnl below, at and above H, up to 256
  5. windows of 2 / 101 / 256           through peek, and through branch sets with selects and a fork of 64
  6. market look-backs of 256           the observation a look-ahead derives from the track

Every comparison is for equality of every element of every book, floats through their integer views; the helpers are those of
tests/test_gpu_vec_peek.py, _vec_rollout.py, _vec_branch.py and _branch_obs.py, guard planes included.  Behind every checked look-ahead
lob_vec_status reports no error and no action out of range; behind the yardstick's real steps it reports what the plans put in.  The
cases, their scripted actions and their schedules are tests/lookahead_edge_cases.py; tests/test_lookahead_edge_cases.py reaches every
coverage assertion made here with the oracle alone."""
import numpy as np
import pytest

from rl_markets_amd import abi
from tests import lookahead_edge_cases as lc
from tests import test_gpu_branch_obs as bo
from tests.parity import dumps_to_np
from tests.test_gpu_snapshot import Run
from tests.test_gpu_vec_branch import DevBranch, bits, check_fork, steps_against_the_real_steps
from tests.test_gpu_vec_env import check_step
from tests.test_gpu_vec_peek import DevPeek, peek_against_the_step
from tests.test_gpu_vec_peek import new_seen as peek_seen
from tests.test_gpu_vec_rollout import DevRoll, assert_equal, composed

pytestmark = pytest.mark.gpu
GAMMA = 0.97


def start(p, rec, seed):
    """-> (Run on the case's records, and the episode its generator scouts: actions, ends, cursors, terminal words)"""
    r = Run(rec.shape[0], seed=seed, p=p, rec=rec)
    sc = r.new_oracle()
    sc.reset()
    acts, ends, cur, term = lc.scout(sc, r.rng, r.B)
    sc.close()
    return r, acts, ends, cur, term


def books(r):
    return dumps_to_np(r.eng.get_books())


def clean(r, tag):
    assert r.eng.vec_status() == (abi.LOB_OK, 0), tag + ": a look-ahead raises no flag and counts no action"


def counted(r, n, tag):
    assert r.eng.vec_status() == ((abi.LOB_EINVAL, n) if n else (abi.LOB_OK, 0)), tag + ": the real steps count the plans' actions out of range"


def everything(r):
    return {"books": bytes(r.eng.get_books()), "state": r.eng.get_state().tobytes(), "reward": r.eng.get_reward().tobytes(),
            "terminal": r.eng.get_terminal().tobytes(), "counters": tuple(r.eng.counters())}


def unchanged(r, before, tag):
    after = everything(r)
    for k in before:
        assert after[k] == before[k], "%s: the look-ahead changed %s" % (tag, k)


def real_step(r, a, cur_want, tag, check=True):
    """The scouted action on the engine -> (its outputs, the cursors behind it); `check` (the steps behind a checked look-ahead): the
    cursors are read from the engine and are those of the scouted episode."""
    r.dev.step(r.eng, a)
    got = r.dev.read(r.eng)
    cur = books(r)["cursor"] if check else None
    if check:
        np.testing.assert_array_equal(cur, cur_want, err_msg=tag + ": the engine's cursors are the scouted episode's")
    return got, cur


def branch_steps(r, db, plans, ref, tag, obs=None):
    """fork, then the H branch steps of `plans` against a yardstick's reward [P][H][B] and obs / terminal / stepped behind the last.
    `obs` (a DevObs of K = 1): -> the branches' terminal words and cursors [H + 1][P][B] behind the fork and behind every step, the
    cursor from lob_branch_history's rec (the record behind it)."""
    got = db.fork(r.eng)
    check_fork(r, got, tag)
    term, cur = [got["terminal"]], [obs.call(r.eng)["hist.rec"] + 1] if obs else []
    stepped = np.zeros(ref["stepped"].shape, np.int32)
    for h in range(plans.shape[1]):
        got = db.step(r.eng, plans[:, h])
        np.testing.assert_array_equal(bits(got["reward"]), bits(ref["reward"][:, h]), err_msg="%s: reward of branch step %d" % (tag, h))
        stepped += got["stepped"]
        term.append(got["terminal"])
        if obs:
            cur.append(obs.call(r.eng)["hist.rec"] + 1)
    np.testing.assert_array_equal(got["obs"], ref["obs"], err_msg=tag + ": obs behind the last branch step")
    np.testing.assert_array_equal(got["terminal"], ref["terminal"], err_msg=tag + ": terminal behind the last branch step")
    np.testing.assert_array_equal(stepped, ref["stepped"], err_msg=tag + ": the sum of the stepped words")
    return np.array(term).astype(np.int32), np.array(cur)


# ---- 1. depth x trade slots, one step ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", ["env16", "env64"])
@pytest.mark.parametrize("D,T", lc.SHAPES)
def test_one_step(D, T, env, monkeypatch):
    """env64: the yardstick's steps go through env_kernel<64> instead of env_kernel<16>.  lob_vec_step's env kernel takes its lanes
    per wave from LOB_ENV_LANES (16 by the batch's size here; tests/test_gpu_parity.py test_books_per_wave_and_group_choices);
    LOB_ENV16_MAX=0, which tests/test_gpu_call_sequences.py sets, moves the learner's fused env step only and is set beside it.  Both
    forms share one timer name and no export tells them apart, so which one ran is not asserted."""
    if env == "env64":
        monkeypatch.setenv("LOB_ENV_LANES", "64")
        monkeypatch.setenv("LOB_ENV16_MAX", "0")
    p, rec, counts, rows = lc.shape_case(D, T)
    r, acts, ends, cur, term = start(p, rec, lc.SEED_ONE_STEP)
    dp = DevPeek(r.B, r.V)
    sched = set(lc.one_step_schedule(ends))
    seen, cov = peek_seen(), lc.Coverage(rows, rec.shape[1])
    tag = "D=%d T=%d %s" % (D, T, env)
    ones, extra = np.ones(r.B, bool), np.zeros(2, np.int64)   # (the yardstick's nine steps are counted by the engine, not by the oracle)
    for s, a in enumerate(acts):
        if s in sched:
            c0 = r.eng.counters()
            peek_against_the_step(r, dp, "%s before step %d" % (tag, s + 1), seen)
            clean(r, tag)
            extra += (r.eng.counters() - c0)[:2]
        r.orc.env_step(a)
        got, cur1 = real_step(r, a, cur[s + 1], tag, s in sched)
        check_step(r.eng, r.orc, got, r.V, 0, "%s step %d" % (tag, s + 1), books=ones)
        c, oc = r.eng.counters(), r.orc.counters()
        assert c[0] - extra[0] == oc[0] and c[1] - extra[1] == oc[1], (tag, s, c, oc, extra)
        if s in sched:
            cov.step(term[s], cur[s], got["terminal"].astype(np.int32), cur1)
    assert (r.eng.get_terminal() == 2).all() and len(acts) > 150
    peek_against_the_step(r, dp, tag + " at the end", seen)
    clean(r, tag)
    assert seen["checked"] == len(sched) and seen["over"]
    assert seen["reward_differs"] and seen["obs_differs"] and seen["dry"], (tag, seen)
    assert cov.missing(D) == [], (tag, cov.seen)
    dp.free()
    r.close()


# ---- 2. depth x trade slots, several steps -----------------------------------------------------------------------------------------------

def select_against_the_rollout(r, db, dr, plans, parent, tag):
    """fork, the first half of the plans, a select by `parent` (in range), the second half: every branch equals the roll-out of its
    ancestor's first half followed by its own second (tests/test_gpu_vec_branch.py test_select)."""
    P, H, B = plans.shape
    half = H // 2
    cols = np.arange(B)[None, :]
    db.fork(r.eng)
    first = np.zeros((P, B), np.int32)
    for h in range(half):
        got = db.step(r.eng, plans[:, h])
        first += got["stepped"]
    sel = db.select(r.eng, parent)
    np.testing.assert_array_equal(sel["obs"], got["obs"][parent, cols], err_msg=tag + ": out.obs of select is the gather")
    np.testing.assert_array_equal(sel["terminal"], got["terminal"][parent, cols], err_msg=tag + ": out.terminal of select is the gather")
    joined = np.concatenate([lc.ancestry(plans[:, :half], parent), plans[:, half:]], axis=1)
    ref = dr.rollout(r.eng, joined, 1.0)
    last = np.zeros((P, B), np.int32)
    for h in range(half, H):
        got = db.step(r.eng, plans[:, h])
        np.testing.assert_array_equal(bits(got["reward"]), bits(ref["reward"][:, h]), err_msg="%s: reward of step %d behind the select" % (tag, h))
        last += got["stepped"]
    np.testing.assert_array_equal(got["obs"], ref["obs"], err_msg=tag + ": obs behind the select")
    np.testing.assert_array_equal(got["terminal"], ref["terminal"], err_msg=tag + ": terminal behind the select")
    np.testing.assert_array_equal(first[parent, cols] + last, ref["stepped"], err_msg=tag + ": stepped of the ancestor's half + the own half")


@pytest.mark.parametrize("D,T", lc.SHAPES)
def test_several_steps(D, T):
    p, rec, counts, rows = lc.shape_case(D, T)
    r, acts, ends, cur, term = start(p, rec, lc.SEED_SEVERAL)
    script = lc.several_script(r.rng, len(acts))
    P, H, K = lc.ROLL_P, lc.ROLL_H, lc.HISTORY_K[(D, T)]
    dr, db = DevRoll(r.B, r.V, P, H), DevBranch(r.B, r.V, P)
    obs, real = bo.DevObs(r.B, D, T, P, K), bo.Real(r, K)
    cov = lc.Coverage(rows, rec.shape[1])
    seen = {"dry_inside": False, "ends_inside": False, "ret_differs": False, "stepped_less": False, "hist_differs": False}
    for s, a in enumerate(acts):
        if s in script:
            plans, parent = script[s]
            tag = "D=%d T=%d before step %d" % (D, T, s + 1)
            np.testing.assert_array_equal(books(r)["cursor"], cur[s], err_msg=tag + ": the engine's cursors are the scouted episode's")
            r.eng.vec_status()
            got = dr.rollout(r.eng, plans, GAMMA)
            clean(r, tag)
            ref = composed(r, plans, GAMMA)
            counted(r, lc.n_bad(plans), tag)
            assert_equal(got, ref, tag + ": the roll-out against the composed route")
            # the branch set under the same plans: against the real steps, every output of every step, and against the roll-out
            stepwise = steps_against_the_real_steps(r, db, plans, tag + ": the branches against the real steps")
            clean(r, tag)
            np.testing.assert_array_equal(bits(stepwise["reward"]), bits(got["reward"]), err_msg=tag + ": the real steps against the roll-out")
            np.testing.assert_array_equal(stepwise["obs"][:, -1], got["obs"], err_msg=tag)
            # ... and its order books and event windows behind the last step
            want = bo.stack(bo.real_steps(r, real, plans, every=H), H - 1)
            have = obs.call(r.eng)
            bo.same(have, want, "%s: lob_branch_book / _history(K = %d)" % (tag, K))
            branch_steps(r, db, plans, got, tag + ": the branches against the roll-out")
            select_against_the_rollout(r, db, dr, plans, parent, tag + ": select")
            clean(r, tag)
            t = ref["term"]
            ends_at = (t[:, :-1] == 0) & (t[:, 1:] != 0)
            live = t[0, 0] == 0
            seen["dry_inside"] |= bool((ends_at & (t[:, 1:] == 2)).any())
            seen["ends_inside"] |= bool(ends_at[:, 1:-1].any())
            seen["ret_differs"] |= bool((live & (bits(got["ret"]) != bits(got["ret"])[0]).any(0)).any())
            seen["stepped_less"] |= bool((live & (got["stepped"] < H) & (got["stepped"] > 0)).any())
            seen["hist_differs"] |= bool((have["hist.rec"] != have["hist.rec"][:1]).any())
        got1, cur1 = real_step(r, a, cur[s + 1], "D=%d T=%d step %d" % (D, T, s + 1), s in script)
        if s in script:
            cov.step(term[s], cur[s], got1["terminal"].astype(np.int32), cur1)
    np.testing.assert_array_equal(r.eng.get_terminal(), term[-1])
    assert (term[-1] == 2).all() and len(acts) > 150
    assert all(seen.values()), (D, T, seen)
    assert cov.missing(D) == [], (D, T, cov.seen)
    for d in (dr, db, obs, real):
        d.free()
    r.close()


# ---- 3. eight keys ------------------------------------------------------------------------------------------------------------------------

def test_eight_keys():
    """The crafted batch of tests/edge_cases.py: a look-ahead of each kind in front of every step that consumes a merging event, in
    front of the step before it, and in front of every 8th step.  Where a branch stands is read from
    lob_branch_history's rec (the record behind the branch's cursor): every merging event is consumed inside a checked look-ahead by
    its first step, and by a later one."""
    p, rec, runs = lc.eight_keys_case()
    r, acts, ends, cur, term = start(p, rec, lc.SEED_EIGHT)
    B = r.B
    script = lc.eight_script(r.rng, runs, cur, term, B)
    P, H = 3, 4
    dp, dr, db = DevPeek(B, r.V), DevRoll(B, r.V, P, H), DevBranch(B, r.V, P)
    obs = bo.DevObs(B, p.depth, p.max_trades, P, 1)
    seen = peek_seen()
    first, later = set(), set()
    for s in range(len(acts) + 1):
        if s not in script:
            real_step(r, acts[s], cur[s + 1], "eight keys", False)
            continue
        tag = "eight keys before step %d" % (s + 1)
        plans = script[s]
        peek_against_the_step(r, dp, tag, seen)
        got = dr.rollout(r.eng, plans, GAMMA)
        clean(r, tag)
        assert_equal(got, composed(r, plans, GAMMA), tag + ": the roll-out against the composed route")
        stepwise = steps_against_the_real_steps(r, db, plans, tag + ": the branches against the real steps")
        np.testing.assert_array_equal(bits(stepwise["reward"]), bits(got["reward"]), err_msg=tag + ": the real steps against the roll-out")
        # once more, with the branches' cursors read behind every step
        live = r.eng.get_terminal() == 0
        db.fork(r.eng)
        c0 = np.broadcast_to(books(r)["cursor"], (P, B))
        for h in range(H):
            t0 = np.broadcast_to(live, (P, B)) if h == 0 else step["terminal"] == 0
            step = db.step(r.eng, plans[:, h])
            c1 = np.where(step["terminal"] == 2, rec.shape[1], obs.call(r.eng)["hist.rec"] + 1)
            for n in range(P):
                (first if h == 0 else later).update(lc.runs_consumed(runs, c0[n], c1[n], t0[n] & (step["stepped"][n] == 1)))
            c0 = c1
        clean(r, tag)
        if s < len(acts):
            real_step(r, acts[s], cur[s + 1], tag)
    want = {(b, f) for b, f, _ in runs}
    assert first == want and later == want, (sorted(want - first), sorted(want - later))
    assert (r.eng.get_terminal() == 2).all() and len(acts) > 100 and seen["reward_differs"] and seen["obs_differs"] and seen["dry"]
    for d in (dp, dr, db, obs):
        d.free()
    r.close()


# ---- 4. the PnL window against the horizon ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lb,H", lc.ROLL_WINDOWS)
def test_window_against_horizon(lb, H):
    """REWARD_NORMED reads the two PnL windows.  roll_rm_prep takes the entry a push replaces from the engine's ring while the plan has
    pushed fewer than lb_pnl times, and from the plan's own pushes -- a workspace that exists only when 1 < lb_pnl < H -- afterwards:
    (2, 3) the smallest workspace, (4, 5) one below the horizon, (3, 64) twenty times round; (5, 5) and above have none, and at 63 /
    64 / 256 the ring slot n % w is far from 0 at entry.  The roll-out and a fork plus H branch steps against the composed route."""
    p, rec, counts, rows = lc.window_case(lb)
    r, acts, ends, cur, term = start(p, rec, lc.SEED_WINDOW)
    n = len(acts)
    script = lc.window_script(r.rng, lb, H, n)
    P = lc.WINDOW_P
    dr, db = DevRoll(r.B, r.V, P, H), DevBranch(r.B, r.V, P)
    obs = bo.DevObs(r.B, p.depth, p.max_trades, P, 1)
    cov = lc.Coverage(rows, rec.shape[1])
    seen = {"own_pushes": False, "full_at_entry": False, "nonzero": False}
    for s, a in enumerate(acts):
        if s in script:
            plans = script[s]
            tag = "lb_pnl=%d H=%d before step %d" % (lb, H, s + 1)
            before = everything(r)
            got = dr.rollout(r.eng, plans, GAMMA)
            bt, bc = branch_steps(r, db, plans, got, tag + ": the branches against the roll-out", obs)
            unchanged(r, before, tag)
            clean(r, tag)
            for q in range(P):
                for h in range(H):
                    cov.step(bt[h, q], bc[h, q], bt[h + 1, q], bc[h + 1, q])
            ref = composed(r, plans, GAMMA)
            assert_equal(got, ref, tag + ": the roll-out against the composed route")
            ticks = dumps_to_np(before["books"])["total_ticks"]
            t = ref["term"].astype(np.int32)
            full = (t[0, 0] == 0) & (ticks >= lb)
            assert lb < 63 or full.any(), tag + ": windows full at entry"
            if lb < H:
                seen["own_pushes"] |= bool(((t[:, 0] == 0) & (ticks >= lb)[None] & (got["stepped"] > lb) & (got["reward"][:, lb:] != 0.0).any(1)).any())
            seen["full_at_entry"] |= bool(full.any())
            seen["nonzero"] |= bool((got["reward"][:, :, full] != 0.0).any())
            np.testing.assert_array_equal(bt.transpose(1, 0, 2), t, err_msg=tag + ": the branches' terminal words against the real steps'")
        real_step(r, a, cur[s + 1], "lb_pnl=%d step %d" % (lb, s + 1), s in script)
    np.testing.assert_array_equal(r.eng.get_terminal(), term[-1])
    assert (term[-1] == 2).all() and n > (400 if lb == 256 else 150)
    assert seen["full_at_entry"] and seen["nonzero"] and cov.missing(p.depth) == [], (lb, H, seen, cov.seen)
    assert seen["own_pushes"] == (lb < H), (lb, H, seen)
    for d in (dr, db, obs):
        d.free()
    r.close()


# ---- 5. windows of 2 / 101 / 256 through peek and branch sets ---------------------------------------------------------------------------

@pytest.mark.parametrize("lb", lc.PEEK_WINDOWS)
def test_windows_through_peek(lb):
    p, rec, counts, rows = lc.window_case(lb)
    r, acts, ends, cur, term = start(p, rec, lc.SEED_PEEK_WINDOW)
    n = len(acts)
    sched = set(lc.peek_window_schedule(lb, n))
    dp = DevPeek(r.B, r.V)
    seen, cov = peek_seen(), lc.Coverage(rows, rec.shape[1])
    nonzero_full = False
    for s in range(n + 1):
        if s in sched:
            tag = "lb_pnl=%d before step %d" % (lb, s + 1)
            before = everything(r)
            pk = peek_against_the_step(r, dp, tag, seen)
            unchanged(r, {k: v for k, v in before.items() if k != "counters"}, tag)   # (the yardstick's nine steps are counted)
            clean(r, tag)
            nonzero_full |= bool(s >= lb and (pk["reward"] != 0.0).any())
        if s < n:
            got, cur1 = real_step(r, acts[s], cur[s + 1], "lb_pnl=%d step %d" % (lb, s + 1), s in sched)
            if s in sched:
                cov.step(term[s], cur[s], got["terminal"].astype(np.int32), cur1)
    assert (r.eng.get_terminal() == 2).all() and n > lb + 20
    assert seen["reward_differs"] and seen["obs_differs"] and seen["dry"] and nonzero_full, (lb, seen)
    assert cov.missing(p.depth) == [], (lb, cov.seen)
    dp.free()
    r.close()


@pytest.mark.parametrize("lb", lc.PEEK_WINDOWS)
def test_windows_through_branch_sets(lb):
    """The sessions of lc.branch_script: a fork of 9 (once, at lb_pnl 256 right behind the fill, of 64: 64 x 128 lanes x (416 + 16 x 256)
    bytes), branch steps and, every 5th call, a select by random per-book parents.  Every step's rewards equal the roll-out of each
    branch's ancestry up to that step, obs / terminal behind it too; at the end of the session the ancestry goes through the real
    steps from a snapshot."""
    p, rec, counts, rows = lc.window_case(lb)
    r, acts, ends, cur, term = start(p, rec, lc.SEED_BRANCH_WINDOW)
    n = len(acts)
    script = lc.branch_script(r.rng, lb, n)
    bufs, rolls, obs = {}, {}, {}
    cov = lc.Coverage(rows, rec.shape[1])
    seen = {"nonzero_behind_a_select": False, "wrapped": False, "replaced": False, "select_moves": False, "big": lb != 256,
            "last_slot_behind_a_select": lb == 256,   # (a second time round 256 entries would take 511 steps)
            "reward_differs": False, "obs_differs": False}
    cols = np.arange(r.B)[None, :]
    for s, a in enumerate(acts):
        if s in script:
            Nb, calls = script[s]
            tag = "lb_pnl=%d N=%d before step %d" % (lb, Nb, s + 1)
            if Nb not in bufs:
                bufs[Nb], obs[Nb] = DevBranch(r.B, r.V, Nb), bo.DevObs(r.B, p.depth, p.max_trades, Nb, 1)
            db = bufs[Nb]
            before = everything(r)
            ticks = dumps_to_np(before["books"])["total_ticks"]
            got = db.fork(r.eng)
            check_fork(r, got, tag)
            t0, c0 = got["terminal"].astype(np.int32), obs[Nb].call(r.eng)["hist.rec"] + 1   # (the branches' cursors: the record behind them + 1)
            played = np.zeros((Nb, 0, r.B), np.int32)
            pushes = np.zeros((Nb, r.B), np.int32)
            selected = False
            for i, (kind, words) in enumerate(calls):
                if kind == "select":
                    sel = db.select(r.eng, words)
                    np.testing.assert_array_equal(sel["obs"], got["obs"][words, cols], err_msg="%s call %d: out.obs of select is the gather" % (tag, i))
                    np.testing.assert_array_equal(sel["terminal"], got["terminal"][words, cols], err_msg="%s call %d: out.terminal of select" % (tag, i))
                    played, pushes, selected = lc.ancestry(played, words), pushes[words, cols], True
                    t0, c0 = t0[words, cols], c0[words, cols]
                    seen["select_moves"] |= bool((words != np.arange(Nb)[:, None]).any())
                    continue
                got = db.step(r.eng, words)
                played = np.concatenate([played, words[:, None]], 1)
                h = played.shape[1]
                if (Nb, h) not in rolls:
                    rolls[(Nb, h)] = DevRoll(r.B, r.V, Nb, h)
                ref = rolls[(Nb, h)].rollout(r.eng, played, 1.0)
                np.testing.assert_array_equal(bits(got["reward"]), bits(ref["reward"][:, -1]), err_msg="%s call %d: reward against the ancestry's roll-out" % (tag, i))
                np.testing.assert_array_equal(got["obs"], ref["obs"], err_msg="%s call %d: obs against the ancestry's roll-out" % (tag, i))
                np.testing.assert_array_equal(got["terminal"], ref["terminal"], err_msg="%s call %d: terminal against the ancestry's roll-out" % (tag, i))
                st = got["stepped"] == 1
                pushes += st
                t1, c1 = got["terminal"].astype(np.int32), obs[Nb].call(r.eng)["hist.rec"] + 1
                for k in range(Nb):
                    cov.step(t0[k], c0[k], t1[k], c1[k])
                t0, c0 = t1, c1
                if h == 1:   # branches of one book under different actions from one state
                    seen["reward_differs"] |= bool((st.all(0) & (bits(got["reward"]) != bits(got["reward"])[0]).any(0)).any())
                    seen["obs_differs"] |= bool((st.all(0) & (got["obs"].view(np.uint32) != got["obs"].view(np.uint32)[0]).any((0, 2))).any())
                seen["nonzero_behind_a_select"] |= bool(selected and (st & (got["reward"] != 0.0)).any())
                seen["wrapped"] |= bool((st & ((ticks[None] + pushes) % lb == 0)).any())
                seen["replaced"] |= bool((st & (ticks >= lb)[None]).any())
                # (push number j, from 0, goes to slot j % lb_pnl: the last slot of a full window, copied by a select just before)
                seen["last_slot_behind_a_select"] |= bool(selected and (st & (ticks >= lb)[None] & ((ticks[None] + pushes) % lb == 0)).any())
            unchanged(r, before, tag)
            clean(r, tag)
            # the ancestry through the real steps: the last branch step's outputs
            c = composed(r, played, 1.0)
            np.testing.assert_array_equal(bits(got["reward"]), bits(c["reward"][:, -1]), err_msg=tag + ": reward against the real steps along the ancestry")
            np.testing.assert_array_equal(got["obs"], c["obs"], err_msg=tag + ": obs against the real steps along the ancestry")
            np.testing.assert_array_equal(got["terminal"], c["terminal"], err_msg=tag + ": terminal against the real steps along the ancestry")
            seen["big"] |= Nb == abi.MAX_BRANCHES
        real_step(r, a, cur[s + 1], "lb_pnl=%d step %d" % (lb, s + 1), s in script)
    assert (r.eng.get_terminal() == 2).all() and n > lb + 20
    assert all(seen.values()), (lb, seen)
    assert cov.missing(p.depth) == [], (lb, cov.seen)
    for d in list(bufs.values()) + list(rolls.values()) + list(obs.values()):
        d.free()
    r.close()


# ---- 6. market look-backs of 256 ------------------------------------------------------------------------------------------------------------

def test_market_lookbacks_of_256():
    p, rec, counts, rows = lc.lookback_case()
    r, acts, ends, cur, term = start(p, rec, lc.SEED_LOOKBACKS)
    n = len(acts)
    script = lc.lookback_script(r.rng, n)
    P, H = lc.WINDOW_P, 8
    dp, dr = DevPeek(r.B, r.V), DevRoll(r.B, r.V, P, H)
    seen, cov = peek_seen(), lc.Coverage(rows, rec.shape[1])
    obs_differs = False
    for s in range(n + 1):
        if s in script:
            tag = "look-backs of 256 before step %d" % (s + 1)
            peek_against_the_step(r, dp, tag, seen)
            got = dr.rollout(r.eng, script[s], GAMMA)
            clean(r, tag)
            assert_equal(got, composed(r, script[s], GAMMA), tag + ": the roll-out against the composed route")
            obs_differs |= bool((got["obs"].view(np.uint32)[0] != got["obs"].view(np.uint32)[1]).any())
        if s < n:
            got1, cur1 = real_step(r, acts[s], cur[s + 1], "look-backs of 256 step %d" % (s + 1), s in script)
            if s in script:
                cov.step(term[s], cur[s], got1["terminal"].astype(np.int32), cur1)
    assert (cur[0] >= 256).all() and (r.eng.get_terminal() == 2).all() and n > 400
    assert seen["reward_differs"] and seen["obs_differs"] and seen["dry"] and obs_differs, seen
    assert cov.missing(p.depth) == [], cov.seen
    dp.free()
    dr.free()
    r.close()
