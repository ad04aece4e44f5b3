"""TEST INFRASTRUCTURE: the case generators of tests/test_gpu_lookahead_edges.py -- the look-ahead family (lob_vec_peek, lob_vec_rollout,
the branch calls) at the edges of depth, trade slots and PnL window -- kept apart from the GPU file so that
tests/test_lookahead_edge_cases.py can play the same cases through the oracle on the CPU and show that what the GPU file asserts about
its inputs can be met without the code under test (not collected by pytest).

Every case is a function of its index alone: the records come from tests/edge_cases.py (hardened batches, the crafted eight-key batch)
with the row masks of tests/hard_streams.harden_rows beside them, the actions from the generator tests/test_gpu_snapshot.py Run makes
for (B, seed), drawn from in the same order by both files (scout first, then the plans of the checked look-aheads in step order).
The schedules -- at which steps a look-ahead is checked -- are functions of the scouted episode and live here too."""
import numpy as np

from rl_markets_amd import abi, engine
from tests import edge_cases as ec
from tests import hard_streams as hs
from tests.test_gpu_vec_env import make_params

NA = abi.LOB_N_ACTIONS
B = 65                                   # one lane past a wave
SHAPES = [(1, 1), (1, 8), (2, 2), (4, 3), (6, 2), (7, 5), (9, 8), (10, 1)]   # (depth, trade slots)
HISTORY_K = dict(zip(SHAPES, (128, 3, 1, 128, 3, 1, 128, 3)))                 # K of lob_branch_history, spread over the shapes
ROLL_WINDOWS = [(2, 3), (4, 5), (5, 5), (6, 5), (3, 64), (63, 64), (64, 64), (256, 64)]   # (lb_pnl, H) under REWARD_NORMED
PEEK_WINDOWS = (2, 101, 256)             # lb_pnl through peek and branch sets
WINDOW_D, WINDOW_T = 5, 2
ROLL_P, ROLL_H = 3, 6                    # section 2: plans per book, steps per plan
BRANCH_N, SELECT_EVERY, BIG_FORK = 9, 5, abi.MAX_BRANCHES
SEED_ONE_STEP, SEED_SEVERAL, SEED_EIGHT, SEED_WINDOW, SEED_PEEK_WINDOW, SEED_BRANCH_WINDOW, SEED_LOOKBACKS = 90, 91, 92, 93, 94, 95, 96
_rows = {}


def rng_of(n_books, seed):
    return np.random.default_rng(1000 * n_books + seed)   # (tests/test_gpu_snapshot.py Run's own generator for this seed)


def n_events_of(lb_pnl):
    return 800 if lb_pnl == 256 else 400


def hardened(D, T, n_events=400):
    """-> (records, counts, row masks) of edge_cases.hardened(D, T, B, dry=True, n_events): the same call with the masks kept."""
    key = (D, T, n_events)
    if key not in _rows:
        g = engine.default_gen_params()
        g.n_events = n_events
        g.trade2_prob_q16 = 30000 if T > 1 else 0
        rec, counts, rows = hs.harden_rows(engine.gen_stream_host(g, D, T, 0, B), D, T, hs.SEED + 100 * D + T, dry=True)
        rec.setflags(write=False)
        rows["beyond"] = beyond_rows(rec, rows["deep_trades"] & ~np.roll(rows["crossed"], 1, axis=1), D, T)
        _rows[key] = (rec, counts, rows)
    return _rows[key]


def beyond_rows(rec, deep, D, T):
    """bool [B, n]: the row carries a deep trade (`deep`: of those behind a row that is not crossed) whose price lies beyond the last
    level of the book of the row before it."""
    f = rec.view(np.float32)
    px = f[:, 1:, 2 + 4 * D]
    ask_last, bid_last = f[:, :-1, 2 + D - 1], f[:, :-1, 2 + 2 * D + D - 1]
    out = np.zeros(rec.shape[:2], bool)
    out[:, 1:] = deep[:, 1:] & (rec[:, 1:, 2 + 4 * D + T] > 0) & ((px > ask_last) | (px < bid_last))
    return out


def shape_case(D, T):
    """-> (params, records, counts, row masks): private theta, the PnL reward, 400 hardened events with a dry tail on some books."""
    return (make_params(D, T),) + hardened(D, T)


def window_case(lb_pnl):
    """-> (params, records, counts, row masks): REWARD_NORMED over PnL windows of lb_pnl steps at depth 5 with two trade slots."""
    p = make_params(WINDOW_D, WINDOW_T)
    p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, lb_pnl
    return (p,) + hardened(WINDOW_D, WINDOW_T, n_events_of(lb_pnl))


def lookback_case():
    """-> (params, records, counts, row masks): every market look-back at LOB_MAX_WINDOW = 256 (and lb_pnl with them, under the PnL
    reward) on 1 200 hardened events: Initialise fills the windows and the episode has rows left to step through."""
    p = make_params(WINDOW_D, WINDOW_T)
    for name in ec.LOOKBACKS:
        setattr(p, name, 256)
    return (p,) + hardened(WINDOW_D, WINDOW_T, 1200)


def eight_keys_case():
    """-> (params, records [3, 400, W], runs) of edge_cases.crafted_eight_keys()."""
    rec, runs = ec.crafted_eight_keys()
    return make_params(5, 8), rec, runs


# ---- actions and plans -----------------------------------------------------------------------------------------------------------------

def scout(orc, rng, n_books, cap=900):
    """tests/test_gpu_vec_peek.py scout, restated so that the CPU file imports no look-ahead test: the episode played by the oracle
    alone under random actions -> the action arrays, for every step whether a live book's episode ends in it, and the cursors
    [steps + 1][B] and terminal words [steps + 1][B] in front of every step and behind the last."""
    acts, ends = [], []
    book = orc.recs()["book"]
    cur, term = [book["cursor"].copy()], [book["terminal"].copy()]
    while (term[-1] == 0).any():
        assert len(acts) < cap, "the episode did not end"
        a = rng.integers(0, NA, size=n_books).astype(np.int32)
        orc.env_step(a)
        book = orc.recs()["book"]
        acts.append(a)
        ends.append(bool(((term[-1] == 0) & (book["terminal"] != 0)).any()))
        cur.append(book["cursor"].copy())
        term.append(book["terminal"].copy())
    return acts, ends, np.array(cur), np.array(term)


def padded_plans(rng, P, H, n_books):
    """Per-book plans [P][H][B]: random actions, a tail of -1 pads of random length (0 .. H - 1) in a third of the (plan, book)
    pairs, and one action out of range (9) in front of a pad-free plan."""
    plans = rng.integers(0, NA, size=(P, H, n_books)).astype(np.int32)
    length = np.where(rng.random((P, n_books)) < 1.0 / 3.0, rng.integers(1, H + 1, size=(P, n_books)), H)
    plans[np.arange(H)[None, :, None] >= length[:, None, :]] = -1
    p, b = int(rng.integers(0, P)), int(rng.integers(0, n_books))
    plans[p, int(rng.integers(0, H)), b] = NA
    return plans


def n_bad(plans):
    return int(((plans < 0) | (plans >= NA)).sum())


def random_plans(rng, P, H, n_books):
    return rng.integers(0, NA, size=(P, H, n_books)).astype(np.int32)


def random_parents(rng, N, n_books):
    return rng.integers(0, N, size=(N, n_books)).astype(np.int32)


# ---- schedules: the steps in front of which a look-ahead is checked (len(acts) stands for "behind the last step") ----------------------

def one_step_schedule(ends, k=7):
    """tests/test_gpu_vec_peek.py scouted_actions_to_the_end: before every k-th step, before every step in which a book's episode ends,
    before each of the last three steps and once behind the last."""
    n = len(ends)
    return [s for s in range(n) if s % k == 0 or ends[s] or s >= n - 3] + [n]


# Section 2 runs four yardsticks per checked step (the composed route, the real steps twice, the ancestry's roll-out) and at K = 128
# reads 6 MB of history per call: before every 10th step its slowest shapes took 1.07 s, against 0.39 s for the slowest case of
# tests/test_gpu_vec_rollout.py::test_against_the_real_steps on the same card; before every 15th they take 0.85 s.  The window cases,
# one yardstick per checked step, keep every 10th.
STRIDE, STRIDE_SEVERAL = 10, 15


def several_steps_schedule(n, k=STRIDE, tail=8):
    return [s for s in range(n) if s % k == 0 or s >= n - tail]


def eight_schedule(runs, cur, term, k=8):
    """The crafted batch: in front of every scouted step that consumes the first row of a merging event of `runs` (the look-ahead's
    first step meets it), in front of the step before that one (a later step does), in front of every step in which a book's episode
    ends, every k-th step and once behind the last."""
    n = len(cur) - 1
    hit = {s for s in range(n) if runs_consumed(runs, cur[s], cur[s + 1], term[s] == 0)}
    ends = {s for s in range(n) if ((term[s] == 0) & (term[s + 1] != 0)).any()}
    return sorted(hit | {s - 1 for s in hit if s > 0} | ends | set(range(0, n, k)) | {n})


def window_schedule(lb_pnl, H, n):
    """The roll-out's window cases.  Windows that fill late (lb_pnl >= 63): four entries -- lb_pnl + 2 real steps in (the windows are
    full at entry), twice in the middle, and within H steps of the end.  The long horizon over a short window: every 40th step from
    the 5th and one within H steps of the end.  The short horizons: every 10th step and the last eight."""
    if lb_pnl >= 63:
        first = lb_pnl + 2
        assert n - 40 > first + 2, (lb_pnl, n)
        return sorted({first, first + (n - 40 - first) // 3, first + 2 * (n - 40 - first) // 3, n - 40})
    if H >= 64:
        return sorted(set(range(5, n - 40, 40)) | {n - 40})
    return several_steps_schedule(n)


def peek_window_schedule(lb_pnl, n, k=11):
    """Windows through peek: every k-th step, the first three steps behind the fill (lb_pnl real steps in), the last three steps
    and once behind the last."""
    return sorted({s for s in range(n) if s % k == 0 or lb_pnl <= s < lb_pnl + 3 or s >= n - 3} | {n})


def branch_window_schedule(lb_pnl, n):
    """Windows through branch sets: a session (a fork and the calls of branch_script) in front of every 40th real step, four steps
    in front of the fill -- the windows fill inside the session and the ring slot goes from lb_pnl - 1 back to 0 --, right behind
    it, where every push replaces an entry of the engine's, and five steps in front of the second time round, where the push behind
    the session's first select replaces the ring's last slot (where the episode is that long)."""
    again = {2 * lb_pnl - 5} if 0 <= 2 * lb_pnl - 5 < n - SESSION else set()
    return sorted({s for s in range(n) if s % 40 == 0} | {max(lb_pnl - 4, 0), min(lb_pnl + 1, n - 1)} | again)


# ---- scripts: everything a case draws behind its scouted episode, drawn at once and in one order ------------------------------------------

WINDOW_P = 2
SESSION = 12   # calls of a branch session behind its fork


def several_script(rng, n):
    """{step: (plans [ROLL_P][ROLL_H][B] with pads and an action out of range, parents [ROLL_P][B] of the select)}"""
    return {s: (padded_plans(rng, ROLL_P, ROLL_H, B), random_parents(rng, ROLL_P, B)) for s in several_steps_schedule(n, k=STRIDE_SEVERAL)}


def eight_script(rng, runs, cur, term, n_books, P=3, H=4):
    return {s: random_plans(rng, P, H, n_books) for s in eight_schedule(runs, cur, term)}


def window_script(rng, lb_pnl, H, n):
    return {s: random_plans(rng, WINDOW_P, H, B) for s in window_schedule(lb_pnl, H, n)}


def lookback_script(rng, n, H=8):
    return {s: random_plans(rng, WINDOW_P, H, B) for s in sorted({t for t in range(n) if t % 50 == 0 or t >= n - 3} | {n})}


def branch_script(rng, lb_pnl, n):
    """{step: (N, calls)}: a branch session in front of that real step -- a fork of N, then `calls`, each ("step", actions [N][B]) or,
    every SELECT_EVERY-th, ("select", parents [N][B]).  N = BRANCH_N; at lb_pnl 256 the session right behind the fill forks BIG_FORK
    branches and is half as long."""
    out = {}
    for s in branch_window_schedule(lb_pnl, n):
        big = lb_pnl == 256 and s == lb_pnl + 1
        N = BIG_FORK if big else BRANCH_N
        calls = []
        for i in range(1, (SESSION // 2 if big else SESSION) + 1):
            if i % SELECT_EVERY == 0:
                calls.append(("select", random_parents(rng, N, B)))
            else:
                calls.append(("step", rng.integers(0, NA, size=(N, B)).astype(np.int32)))
        out[s] = (N, calls)
    return out


def ancestry(played, parent):
    """The actions [N][h][B] that branch (n, b) has behind it, rearranged by a select with in-range parents [N][B]."""
    cols = np.arange(parent.shape[1])
    return played[parent[:, None, :], np.arange(played.shape[1])[None, :, None], cols[None, None, :]]


# ---- what a comparison has covered ---------------------------------------------------------------------------------------------------

class Coverage:
    """Conditions on the INPUTS, accumulated over the checked steps from a yardstick's own words (the oracle's on the CPU, the real
    step's on the GPU): `rows` are the masks of hard_streams.harden_rows."""

    def __init__(self, rows, n_events):
        self.rows, self.n = rows, n_events
        self.seen = {"dry": False, "crossed": False, "beyond": False}
        self.books = np.arange(next(iter(rows.values())).shape[0])

    def step(self, term0, cur0, term1, cur1):
        """One checked real step: terminal words and cursors in front of it and behind it."""
        live = term0 == 0
        at = np.minimum(cur0, self.n - 1)
        self.seen["dry"] |= bool((live & (term1 == 2)).any())
        self.seen["crossed"] |= bool((live & self.rows["crossed"][self.books, at]).any())
        if "beyond" in self.rows:
            for b in np.flatnonzero(live & (cur1 > cur0)):
                self.seen["beyond"] |= bool(self.rows["beyond"][b, cur0[b]:cur1[b]].any())

    def missing(self, depth):
        need = ["dry", "crossed"] + (["beyond"] if depth == 1 else [])
        return [k for k in need if not self.seen[k]]


def runs_consumed(runs, cur0, cur1, live):
    """The (book, first row) of `runs` whose first row a step from cursors cur0 to cur1 consumes."""
    return {(b, first) for b, first, _ in runs if live[b] and cur0[b] <= first < cur1[b]}
