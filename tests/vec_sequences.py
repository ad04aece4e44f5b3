"""Seeded call sequences over the vector-env interface, chosen from the state of the model (tests/vec_model.py) alone -- never from an
engine's output -- so that the same sequence can be produced and walked on the CPU without an engine.  Not collected by pytest; used
by tests/test_vec_model.py (coverage of the default seeds) and tests/test_gpu_call_sequences.py.

    for i, kind, args, want in ops(seed):      # `want`: the model's Result for the call, the model already behind it
        ...

A sequence starts on an engine whose stream is loaded and which has seen no lob_reset, runs 60-90 operations over two or three
episodes and usually reaches books that are over.  About one operation in eight is a call the contract refuses in the present state
(only calls the header documents as refused on the host: no invalid pointer, nothing that reaches a kernel with bad arguments).
lob_reset inside a half-done learner step is left out (tests/test_gpu_halfstep.py has it): where the step counter stands behind an
abandoned half is not part of the contract."""
import zlib

import numpy as np

from rl_markets_amd import abi, engine
from tests.test_gpu_vec_env import gen, make_params
from tests.test_oracle_days import make_days
from tests.vec_model import KINDS, NA, Model

N_EVENTS = 160
DAY_LENGTHS = (160, 100, 130)
MEM = 1 << 14   # (private weights of 130 books: the learner is exact at any table size)
# kinds the contract never refuses once a stream is loaded
NEVER_REFUSED = ("reset", "close", "status")
EDGE_SEEDS = tuple(s for s in range(24) if s % 8 in (3, 6))
LONG_FACTOR, LONG_PROLOGUE = 4, 110   # the edge seeds with lb_pnl 101: streams of 400 .. 640 events (225 steps and more), 110 steps in front
EDGE_VISIT = ("vec_step", "fork", "bstep", "select", "bstep", "peek", "rollout")


class Variant:
    """The shapes of one sequence, derived from its seed: each value of each axis occurs in at least four of the 24 default seeds
    (tests/test_vec_model.py asserts it).  A quarter of the seeds (EDGE_SEEDS, seed % 8 in {3, 6}) run an edge shape in place of
    their depth, trade slots and window: depth 1 or 7, one or eight trade slots, and lb_pnl 101 where the seed's reward is NORMED
    -- the edges of tests/test_gpu_lookahead_edges.py under an order nobody chose.  A window of 101 steps never fills in an episode
    of 160 events, so the seeds that have it (`long`) play streams four times as long, and every episode of theirs opens with EDGE_VISIT:
    LONG_PROLOGUE real steps, behind which the windows are full, then a fork, a branch step, a select, a branch step, a peek and a
    roll-out, all with non-zero NORMED rewards to compare (tests/test_vec_model.py asserts that they occur).  Every other seed is
    what it was."""

    def __init__(self, seed):
        self.seed = seed
        self.B = (3, 65, 130)[seed % 3]                      # a partial wave, one lane past a wave, two waves + 2
        self.env16_off = (seed // 3) % 3 == 0                # LOB_ENV16_MAX=0: the real steps run the 64-lane env_kernel
        self.depth = (5, 10)[seed % 2]
        self.trades = (2, 3)[(seed // 2) % 2]                # the <true> and <false> forms of the look-ahead step
        self.normed = (seed // 4) % 2 == 1                   # REWARD_NORMED, lb_pnl 3: the private window ring
        self.edge = seed % 8 in (3, 6)
        self.lb_pnl = 3
        if self.edge:
            self.depth = (1, 7)[seed % 2]                    # rows of 28 and 124 bytes
            self.trades = (1, 8)[(seed // 3) % 2]            # the <true> form with one slot, step_event<LOB_MAX_TRADES>
            self.lb_pnl = 101                                # (read under NORMED only)
        self.long = self.edge and self.normed
        self.n_events = LONG_FACTOR * N_EVENTS if self.long else N_EVENTS
        self.day_lengths = tuple(LONG_FACTOR * n for n in DAY_LENGTHS) if self.long else DAY_LENGTHS
        self.days = seed % 4 in (1, 2)                       # a day library of unequal days
        self.ending = "dry" if self.days else ("session", "dry")[(seed // 3 + seed) % 2]

    def label(self):
        return "B=%d D=%d T=%d %s %s%s%s" % (self.B, self.depth, self.trades, "normed-%d" % self.lb_pnl if self.normed else "pnl", self.ending,
                                             " days" if self.days else "", " env16-off" if self.env16_off else "")

    def params(self):
        p = make_params(self.depth, self.trades, MEM)
        if self.normed:
            p.reward_measure, p.lb_pnl = abi.REWARD_NORMED, self.lb_pnl
        return p

    def data(self):
        """(records [B][n][W] or None, days or None)"""
        p = self.params()
        if self.days:
            return None, make_days(self.day_lengths, first_id=2000 + self.seed, depth=self.depth, trades=self.trades)
        return engine.gen_stream_host(gen(self.n_events, self.ending, p), self.depth, self.trades, 0, self.B), None

    def model(self):
        rec, days = self.data()
        return Model(self.params(), self.B, records=rec, days=days)


def describe(kind, args):
    """One line per operation; a long array as its shape and checksum (ops(seed) makes it again)."""
    parts = []
    for k, v in args.items():
        if isinstance(v, np.ndarray):
            v = v.tolist() if v.size <= 16 else "<%s %s crc %08x>" % (v.dtype, list(v.shape), zlib.crc32(np.ascontiguousarray(v).tobytes()))
        parts.append("%s=%s" % (k, v))
    return "%s(%s)" % (kind, ", ".join(parts))


class Sequence:
    def __init__(self, seed, variant=None, model=None):
        self.seed, self.v = seed, variant or Variant(seed)
        self.m = model or self.v.model()
        self.rng = np.random.default_rng([seed, 20261020])
        self.length = 60 + int(self.rng.integers(0, 31))
        self.done_once = set()          # the rare shapes taken once per sequence
        self.first_fork = None
        self.refuse_turn = seed * 11    # the refused kinds take turns, from a start that moves with the seed
        self.log = []                   # describe() of every operation so far
        self.over_ops = self.ops_since_reset = 0
        self.refusing = False
        self.void_probe = 0
        self.stats = {"all_over_ops": 0}
        self.visit = []                 # what is left of EDGE_VISIT in this episode (Variant.long)

    # ---- arguments ------------------------------------------------------------------------------------------------------------------
    def actions(self, shape, p_hole=0.06):
        a = self.rng.integers(0, NA, size=shape).astype(np.int32)
        holes = self.rng.random(shape) < p_hole
        a[holes] = self.rng.choice(np.array([-1, NA], np.int32), size=int(holes.sum()))   # out of range: the book is skipped
        return a

    def mask(self):
        B, r = self.m.B, self.rng
        which = int(r.integers(0, 7))
        if (self.m.terminal() != 0).any() and r.random() < 0.8:
            which = 6 if r.random() < 0.7 else 0   # books are over: more often than not a restore is there to revive them
        if which == 0:
            return None
        if which == 1:
            return r.integers(0, 2, size=B).astype(np.uint8)
        if which == 2:
            return np.zeros(B, np.uint8)
        if which == 3:
            return (np.arange(B) == 0).astype(np.uint8)
        if which == 4:
            return (np.arange(B) == B - 1).astype(np.uint8)
        if which == 5:
            return np.where(r.integers(0, 2, size=B) == 1, r.integers(2, 256, size=B), 0).astype(np.uint8)   # bytes other than 1
        m = self.m.terminal() != 0                                                                            # the books that are over
        return m.astype(np.uint8) * np.uint8(r.integers(1, 256))

    def parents(self):
        N, B, r = self.m.N, self.m.B, self.rng
        which = int(r.choice([0, 1, 2, 3, 3, 3, 4, 4]))
        ident = np.broadcast_to(np.arange(N, dtype=np.int32)[:, None], (N, B)).copy()
        if which == 0:
            return ident
        if which == 1:
            return np.broadcast_to(r.permutation(N).astype(np.int32)[:, None], (N, B)).copy()
        if which == 2:
            return np.full((N, B), int(r.integers(0, N)), np.int32)
        p = r.integers(0, N, size=(N, B)).astype(np.int32)
        if which == 4:
            odd = r.random((N, B)) < 0.3
            p[odd] = r.choice(np.array([-1, N, N + 7, np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int32), size=int(odd.sum()))
        return p

    def once(self, name, every, phase):
        """True the first time (in a call that is not going to be refused) in a sequence whose seed is `phase` mod `every`."""
        if self.refusing or self.seed % every != phase or name in self.done_once:
            return False
        self.done_once.add(name)
        return True

    def args_of(self, kind):
        m, r = self.m, self.rng
        if kind == "vec_step":   # (a burst of k calls: an episode of 160 events lasts 50-70 steps)
            return {"actions": self.actions((1 if self.refusing else int(r.choice([1, 1, 2, 4, 7, 10])), m.B), 0.06 if r.random() < 0.5 else 0.0)}
        if kind == "history":
            return {"K": abi.MAX_HISTORY if self.once("K", 4, 2) else int(r.choice([1, 2, 7]))}
        if kind == "peek":
            return {"mask": abi.PEEK_ALL if r.random() < 0.5 else int(r.integers(1, abi.PEEK_ALL + 1))}
        if kind == "rollout":
            P, H = int(r.choice([1, 2, 3, 5])), int(r.choice([1, 2, 4, 6]))
            if self.once("P", 4, 3):      # each limit once in a few seeds (both at once: half a million oracle steps at B = 130)
                P, H = abi.MAX_ROLLOUT_PLANS, 2
            elif self.once("H", 4, 0):
                P, H = 2, abi.MAX_ROLLOUT_STEPS
            return {"plans": self.actions((P, H, m.B)), "gamma": float(r.choice([1.0, 0.97, 0.0]))}
        if kind in ("save", "restore"):
            full = [s for s in range(abi.MAX_SNAPSHOTS) if m.slot_state[s] == "full"]
            if kind == "restore" or (full and r.random() < 0.4):
                return {"slot": int(r.choice(full)), "mask": self.mask()}
            return {"slot": int(r.integers(0, abi.MAX_SNAPSHOTS)), "mask": None}
        if kind == "snapshot_free":
            return {"slot": int(r.integers(0, abi.MAX_SNAPSHOTS))}
        if kind == "fork":
            if self.first_fork is None:
                N = int(r.choice([1, 2, 2]))
            else:
                N = abi.MAX_BRANCHES if self.once("N", 4, 1) else int(r.choice([1, 2, 9, 9]))
            return {"N": N}
        if kind == "bstep":
            return {"actions": self.actions((m.N, m.B))}
        if kind == "select":
            return {"parent": self.parents()}
        if kind == "stats":
            return {"by_day": bool(m.lib is not None and r.random() < 0.5)}
        if kind == "log_enable":
            if m.log_n and r.random() < 0.7:
                return {"sel": np.zeros(0, np.int32), "cap": 0}
            if r.random() < 0.4:
                return {"sel": None, "cap": int(r.choice([4, 64]))}
            sel = np.flatnonzero(r.random(m.B) < 0.4).astype(np.int32)
            return {"sel": sel if len(sel) else np.array([m.B - 1], np.int32), "cap": int(r.choice([4, 64]))}
        if kind in ("td_step", "eval_step"):
            return {"n": int(r.choice([1, 1, 2, 5]))}
        if kind == "days_set":
            return {"days": r.integers(0, m.n_days, size=m.B).astype(np.int32)}
        if kind == "days_select":
            first = int(r.integers(0, m.n_days))
            return {"mode": int(r.choice([abi.DAYS_RANDOM, abi.DAYS_IN_ORDER])), "first": first, "n": int(r.integers(1, m.n_days - first + 1))}
        return {}

    # ---- the choice ------------------------------------------------------------------------------------------------------------------
    def legal(self):
        """(kind, weight) of the calls that are legal now."""
        m = self.m
        if m.half_open:
            return [("td_end", 6.0), ("status", 1.0), ("snapshot_free", 0.5), ("close", 0.3)]
        over = float((m.terminal() != 0).mean())
        mixed = 0.0 < over < 1.0
        full = any(s == "full" for s in m.slot_state)
        w = [("vec_step", 26.0), ("observe", 2.5), ("status", 2.0), ("getters", 3.0), ("book", 2.5), ("history", 2.5), ("peek", 3.5),
             ("rollout", 2.5), ("save", 7.0), ("snapshot_free", 2.0), ("fork", 4.0 + 8.0 * mixed), ("close", 2.0),
             ("stats", 3.0 + 4.0 * m.restored), ("log_enable", 3.0 if m.log_n else 1.5), ("clear_inventory", 2.0),
             ("reset", 0.3 + 0.08 * self.ops_since_reset + 6.0 * over * over + (400.0 if self.over_ops >= 3 else 0.0))]
        if full and not m.log_n:
            w.append(("restore", 6.0 + 250.0 * over))
        if m.branch == "live":
            w += [("bstep", 8.0 + 15.0 * mixed), ("select", 8.0)]
        if m.log_n:
            w += [("log_counts", 8.0), ("log_read", 9.0)]
        if not m.restored:   # (learner and greedy steps among the vec steps, whatever those skipped)
            w += [("td_step", 3.5), ("eval_step", 3.0), ("td_begin", 3.5)]
        if m.lib is not None:   # (a selection may come at any time: the next lob_reset plays the latest)
            w += [("days_set", 2.5), ("days_select", 2.5)]
        return w

    def refusable(self):
        """(kind, args) of the calls the contract refuses now."""
        m, r = self.m, self.rng
        out = []
        self.refusing = True
        try:
            return self._refusable(m, r, out)
        finally:
            self.refusing = False

    def _refusable(self, m, r, out):
        if not m.was_reset or m.half_open:
            guarded = ["vec_step", "observe", "book", "history", "peek", "rollout", "save", "restore", "fork", "bstep", "select", "stats",
                       "clear_inventory", "td_step", "eval_step", "td_begin"]
            if not m.was_reset:
                guarded += ["getters", "td_end"]
            else:
                guarded += ["log_enable"] + (["log_counts", "log_read"] if m.log_n else []) + (["days_set", "days_select"] if m.lib is not None else [])
            for k in guarded:
                if k in ("bstep", "select") and m.N == 0:
                    out.append((k, {"actions" if k == "bstep" else "parent": np.zeros((2, m.B), np.int32)}))
                elif k == "restore":
                    out.append((k, {"slot": int(r.integers(0, abi.MAX_SNAPSHOTS)), "mask": None}))
                else:
                    out.append((k, self.args_of(k)))
            out.append(("snapshot_free", {"slot": abi.MAX_SNAPSHOTS}))   # (no guard in front of it: the argument check alone)
            return out
        hollow = [s for s in range(abi.MAX_SNAPSHOTS) if m.slot_state[s] != "full"]
        full = [s for s in range(abi.MAX_SNAPSHOTS) if m.slot_state[s] == "full"]
        if hollow:
            out.append(("restore", {"slot": int(r.choice(hollow)), "mask": self.mask()}))
            out.append(("save", {"slot": int(r.choice(hollow)), "mask": r.integers(0, 2, size=m.B).astype(np.uint8)}))
        if m.branch != "live":
            N = max(m.N, 2)
            out.append(("bstep", {"actions": np.zeros((N, m.B), np.int32)}))
            out.append(("select", {"parent": np.zeros((N, m.B), np.int32)}))
        if m.restored:
            out += [("td_step", {"n": 1}), ("eval_step", {"n": 1}), ("td_begin", {})]
        if m.log_n and full:
            out.append(("restore", {"slot": int(r.choice(full)), "mask": None}))
        if not m.log_n:
            out += [("log_counts", {}), ("log_read", {})]
        if m.lib is None:
            out += [("stats", {"by_day": True}), ("days_set", {"days": np.zeros(m.B, np.int32)}),
                    ("days_select", {"mode": abi.DAYS_IN_ORDER, "first": 0, "n": 1})]
        out += [("td_end", {}), ("fork", {"N": int(r.choice([0, abi.MAX_BRANCHES + 1]))}),
                ("save", {"slot": abi.MAX_SNAPSHOTS, "mask": None}), ("restore", {"slot": abi.MAX_SNAPSHOTS, "mask": None}),
                ("snapshot_free", {"slot": abi.MAX_SNAPSHOTS})]
        return out

    def choose(self, i):
        m, r = self.m, self.rng
        if not m.was_reset:
            if i < 2 + self.seed % 2:
                return self.refused_one()
            if m.lib is not None and m.day_next is None:
                k = "days_set" if r.random() < 0.5 else "days_select"
                return k, self.args_of(k)
            return "reset", {}
        if self.v.long and self.ops_since_reset == 0 and not m.half_open:
            self.visit = list(EDGE_VISIT)
        if self.visit and not m.half_open:
            return self.visit_one(self.visit.pop(0))
        if m.half_open:
            if i >= self.length - 1:
                return "td_end", {}   # (a sequence ends on a whole step: the last sweep compares the books)
            if r.random() < 0.7 and self.half_refusals < 5:
                self.half_refusals += 1
                return self.refused_one()
        elif r.random() < 0.06 and i < self.length - 1:
            return self.refused_one()
        if m.branch == "void" and not m.half_open and self.void_probe != m.episode and r.random() < 0.5:
            self.void_probe = m.episode   # a lob_reset has voided the set: once per episode a step or a select on it, which is refused
            k = "bstep" if r.random() < 0.5 else "select"
            return k, {"actions" if k == "bstep" else "parent": np.zeros((m.N, m.B), np.int32)}
        kinds, weights = zip(*self.legal())
        weights = np.array(weights) / np.sum(weights)
        kind = str(kinds[int(r.choice(len(kinds), p=weights))])
        if kind == "reset" and m.lib is not None and r.random() < 0.8:
            k = "days_set" if r.random() < 0.5 else "days_select"   # another day in front of the reset: the next turn resets
            self.reset_next = True
            return k, self.args_of(k)
        if kind == "td_begin":
            self.half_refusals = 0
        return kind, self.args_of(kind)

    def visit_one(self, kind):
        """The next call of EDGE_VISIT, with arguments that keep every book stepping."""
        m, r = self.m, self.rng
        if kind == "vec_step":
            return kind, {"actions": self.actions((LONG_PROLOGUE, m.B), 0.0)}
        if kind == "fork":
            return kind, {"N": 2}
        if kind == "bstep":
            return kind, {"actions": self.actions((m.N, m.B), 0.0)}
        if kind == "select":
            return kind, {"parent": r.integers(0, m.N, size=(m.N, m.B)).astype(np.int32)}
        if kind == "peek":
            return kind, {"mask": abi.PEEK_ALL}
        return kind, {"plans": self.actions((2, 4, m.B), 0.0), "gamma": 1.0}

    def refused_one(self):
        """The refusable calls take turns by kind, so that every kind is refused across a handful of seeds."""
        cand = self.refusable()
        kinds = sorted({k for k, _ in cand}, key=KINDS.index)
        self.refuse_turn += 5   # (a stride through the kinds that are refusable now: each gets its turn across a handful of seeds)
        options = [c for c in cand if c[0] == kinds[self.refuse_turn % len(kinds)]]
        return options[int(self.rng.integers(0, len(options)))]

    def __iter__(self):
        self.half_refusals, self.reset_next = 0, False
        for i in range(self.length):
            if self.reset_next and not self.m.half_open:
                self.reset_next = False
                kind, args = "reset", {}
            else:
                kind, args = self.choose(i)
            self.log.append(describe(kind, args))
            before = {"restored": self.m.restored, "branch": self.m.branch, "full": any(s == "full" for s in self.m.slot_state)}
            want = self.m.apply(kind, **args)
            if kind == "fork" and want.rc == abi.LOB_OK and self.first_fork is None:
                self.first_fork = args["N"]
            want.before = before
            self.ops_since_reset = 0 if kind == "reset" else self.ops_since_reset + 1
            all_over = self.m.was_reset and bool((self.m.terminal() != 0).all())
            self.over_ops = self.over_ops + 1 if all_over else 0
            self.stats["all_over_ops"] += all_over
            yield i, kind, args, want


def ops(seed, variant=None):
    """The operations of sequence `seed`: (index, kind, args, the model's Result), the model already behind the call."""
    return iter(Sequence(seed, variant))
