"""TEST INFRASTRUCTURE: the oracle-compared cases of tests/test_gpu_exchange_edges.py -- several book shards exchanging their weights
on a schedule -- kept apart from the GPU file so that tests/test_edge_cases.py can run the same schedules on the CPU, oracle shards
against nudged shadow shards: a case whose shadow takes another action says nothing about the engine from that step on, so the
configurations here are the ones the CPU check has seen to stay stable to their end.

A schedule is a list of operations that a ring of shards interprets (OracleRing here, the engines' ring in the GPU file):
    ("step", n)          n learner steps on every shard
    ("begin",) ("end",)  the two halves of one learner step; an exchange fits between them
    ("x",)               one weight exchange
    ("update", rank, k)  an external update (lob_vec_update) of free-standing rows on one shard: update_rows(cfg, k)
    ("episode",)         clear_inventory, handle_terminal, reset on every shard
    ("until_done", period, cap)   steps in periods of `period` with an exchange behind each, until no shard has a live book"""
import numpy as np

from rl_markets_amd import abi, engine
from rl_markets_amd.parallel import shard_books
from tests import exchange_ref as xr
from tests import oracle_lib as ol
from tests.tile_ref import expected_theta, tiles

RL_ALGOS = (abi.ALGO_R_LEARN, abi.ALGO_ONLINE_R_LEARN, abi.ALGO_DOUBLE_R_LEARN)
TWO_VECTORS = (abi.ALGO_DOUBLE_Q, abi.ALGO_DOUBLE_R_LEARN)

# outside, inside, outside, inside the half-open step
FOUR_EXCHANGES = [("step", 8), ("x",), ("step", 7), ("begin",), ("x",), ("end",), ("step", 8), ("x",), ("step", 7), ("begin",), ("x",), ("end",),
                  ("step", 4)]


def case(algo, world, total=12, M=1 << 16, n_events=200, first_book=0, ops=FOUR_EXCHANGES, **params):
    return {"algo": algo, "world": world, "total": total, "M": M, "n_events": n_events, "first_book": first_book, "ops": ops, "params": params}


CASES = {}
for _a, _name in zip(RL_ALGOS, ("r_learn", "online_r_learn", "double_r_learn")):
    for _w in (2, 3):
        CASES["%s-w%d" % (_name, _w)] = case(_a, _w, epsilon=0.4, beta=0.02)
CASES["double_q-inside"] = case(abi.ALGO_DOUBLE_Q, 2)
for _a, _name in ((abi.ALGO_SARSA, "sarsa"), (abi.ALGO_QLAMBDA, "qlambda"), (abi.ALGO_DOUBLE_Q, "double_q")):
    # (c) of the update cases: an update on one rank, learner steps on all, the exchange, four more steps
    CASES["update-%s" % _name] = case(_a, 3, ops=[("step", 6), ("x",), ("update", 1, 0), ("step", 8), ("x",), ("step", 4), ("update", 2, 1),
                                                    ("step", 3), ("begin",), ("x",), ("end",), ("step", 4)])
# one shard's books end several exchange periods before the others'; then the episode boundary
CASES["unequal-ends"] = case(abi.ALGO_QLAMBDA, 3, total=9, n_events=[120, 260, 300],
                             ops=[("until_done", 8, 60), ("episode",), ("x",), ("step", 16), ("x",), ("step", 4)])
CASES["unequal-ends-sarsa"] = case(abi.ALGO_SARSA, 3, total=9, n_events=[120, 260, 300],
                                   ops=[("until_done", 8, 60), ("episode",), ("x",), ("step", 16), ("x",), ("step", 4)])


def tweak_of(cfg):
    def tweak(p):
        p.book_id_offset += cfg["first_book"]
        for k, v in cfg["params"].items():
            setattr(p, k, v)
    return tweak


def shard_inputs(cfg):
    """-> [(params, records)] of the shards, as tests/test_gpu_delta_exchange.py make_shards builds them."""
    out = []
    g = engine.default_gen_params()
    for r in range(cfg["world"]):
        g.n_events = cfg["n_events"][r] if isinstance(cfg["n_events"], (list, tuple)) else cfg["n_events"]
        first, n = shard_books(cfg["total"], cfg["world"], r)
        p = engine.default_params()
        p.memory_size, p.algo, p.book_id_offset = cfg["M"], cfg["algo"], first
        tweak_of(cfg)(p)
        out.append((p, engine.gen_stream_host(g, p.depth, p.max_trades, p.book_id_offset, n)))
    return out


def update_rows(cfg, k, n=48):
    """-> (rows f32 [n][V], actions i32 [n], step f64 [n]) of external update k: random states, small dyadic steps (multiples of
    2^-12 up to 1/64 in size: sums of them are exact in any order, and they nudge the Q values without swamping them)."""
    rng = np.random.default_rng(7700 + k)
    V = engine.default_params().n_vars
    rows = rng.uniform(-3, 3, size=(n, V)).astype(np.float32)
    actions = rng.integers(0, abi.LOB_N_ACTIONS, size=n).astype(np.int32)
    step = rng.integers(-64, 65, size=n).astype(np.float64) * 2.0 ** -12
    return rows, actions, step


def add_update(theta_view, M, rows, actions, step):
    """theta[tile] += step over the 96 tiles of (row, action), in place on a live weight view."""
    expected_theta(M, tiles(M, rows), actions, step, into=theta_view)


class OracleRing:
    """The oracle's schedule of several shards on one common weight vector: the shards step apart, an exchange gives every shard
    theta_sync + the rank-order sum of the shards' theta - theta_sync (written through the oracle's live views), and rho_sync + the
    mean of the shards' rho - rho_sync (oracle_set_rho)."""

    def __init__(self, cfg, inputs=None):
        self.cfg = cfg
        self.M = cfg["M"]
        self.orcs = [ol.Oracle(p, rec) for p, rec in (inputs or shard_inputs(cfg))]
        self.rl = cfg["algo"] in RL_ALGOS
        self.views = [lambda o: o.theta(0)] + ([lambda o: o.theta_b(0)] if cfg["algo"] in TWO_VECTORS else [])
        for o in self.orcs:
            o.reset()
        self.sync = [get(self.orcs[0]).copy() for get in self.views]
        self.rho_sync = self.orcs[0].rho()[0] if self.rl else 0.0
        self.n_exchanges = 0

    def close(self):
        for o in self.orcs:
            o.close()

    def cursors(self):
        return [o.recs()["book"]["cursor"].copy() for o in self.orcs]

    def exchange(self):
        for v, get in enumerate(self.views):
            total = xr.rank_sum([get(o) - self.sync[v] for o in self.orcs])
            for o in self.orcs:
                get(o)[:] = self.sync[v] + total
            self.sync[v] = get(self.orcs[0]).copy()
        if self.rl:
            self.rho_sync = xr.rho_expected([o.rho()[0] for o in self.orcs], self.rho_sync)["rho"]
            for o in self.orcs:
                o.set_rho([self.rho_sync])
        self.n_exchanges += 1

    def update(self, rank, k):
        rows, actions, step = update_rows(self.cfg, k)
        for get in self.views:                      # (double Q: the same increments to both vectors)
            add_update(get(self.orcs[rank]), self.M, rows, actions, step)

    def apply(self, ev):
        """One event of walk() on every shard."""
        if ev[0] == "step":
            for o in self.orcs:
                o.td_step(1)
        elif ev[0] == "begin":
            for o in self.orcs:
                o.td_step_begin()
        elif ev[0] == "end":
            for o in self.orcs:
                o.td_step_end()
        elif ev[0] == "x":
            self.exchange()
        elif ev[0] == "update":
            self.update(ev[1], ev[2])
        elif ev[0] == "episode":
            for o in self.orcs:
                o.clear_inventory(); o.handle_terminal(); o.reset()
        else:
            raise ValueError(ev)

    def run(self, ops):
        """Interprets the schedule.  -> the "until_done" periods (walk)."""
        periods = []
        for ev in walk(ops, self.cursors, periods):
            self.apply(ev)
        return periods


def walk(ops, cursors, periods):
    """The schedule as single events -- ("step",), ("begin",), ("end",), ("x",), ("update", rank, k), ("episode",) -- for whoever
    interprets it (OracleRing.run, shadow_cut, the engines' ring of the GPU file): the one place that unrolls it.  cursors(): the
    books' stream cursors per shard (the oracle's), which decide when "until_done" ends; periods: a list that receives, per period of
    "until_done", which shards still had a book stepping in it."""
    for op in ops:
        if op[0] == "step":
            for _ in range(op[1]):
                yield ("step",)
        elif op[0] == "until_done":
            for _ in range(op[2]):
                before = cursors()
                for _ in range(op[1]):
                    yield ("step",)
                moved = [bool((a != b).any()) for a, b in zip(before, cursors())]
                periods.append(moved)
                yield ("x",)
                if not any(moved):
                    break
            else:
                raise AssertionError("until_done: books still stepping after %d periods" % op[2])
        elif op[0] in ("begin", "end", "x", "update", "episode"):
            yield op
        else:
            raise ValueError(op)


def shadow_cut(cfg):
    """The case's schedule on the oracle shards beside shadow shards whose weights are nudged by 1e-13 (relative) after the fourth
    step -> (None when every shard takes the same actions and draws the same random numbers as its shadow to the end, else the number
    of the first learner step that differs; the "until_done" periods).  (tests/edge_cases.py shadow_cut, for a ring of shards.)"""
    inputs = shard_inputs(cfg)
    ring, shadow = OracleRing(cfg, inputs), OracleRing(cfg, inputs)
    n_step, cut, periods = 0, None, []
    try:   # the two rings run in lock step: one schedule walked over both
        for ev in walk(cfg["ops"], ring.cursors, periods):
            ring.apply(ev)
            shadow.apply(ev)
            if ev[0] not in ("step", "end"):
                continue
            if n_step == 3:
                for get in shadow.views:
                    for o in shadow.orcs:
                        th = get(o)
                        th[th != 0] *= 1.0 + 1e-13
            for a, b in zip(ring.orcs, shadow.orcs):
                ra, rb = a.recs(), b.recs()
                if cut is None and (not np.array_equal(ra["action"], rb["action"]) or not np.array_equal(ra["rng_ctr"], rb["rng_ctr"])):
                    cut = n_step
            n_step += 1
        return cut, periods
    finally:
        ring.close(); shadow.close()
