"""The multi-GPU weight exchange at the edges of world size, table size and algorithm -- several shards on ONE device, the collectives
formed on the host (tests/test_gpu_delta_exchange.py host_allreduce / host_sparse_allreduce), every exchange held BIT FOR BIT against
the numpy restatement tests/exchange_ref.py: each rank's dense delta or packed buffer before it is summed, the count, the zeros behind
the union, theta of every rank after the apply (every weight, so an untouched one that moved shows), the exact map afterwards.  (Of
the two tables above a million weights theta is read back from two ranks; the maps and packed buffers from all.)  The
test tracks theta_sync itself (theta at lob_delta_init, then what the reference says): the engine does not expose it.

The oracle-compared cases (average-reward agents, an external update followed by learner steps, shards that finish at different
times) are the schedules of tests/exchange_cases.py, which tests/test_edge_cases.py has run on the CPU against nudged shadow shards.

No torch in this process; device buffers for lob_vec_update are plain hipMalloc memory (tests/test_gpu_vec_act.py DevArray)."""
import copy
import ctypes as C

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import exchange_cases as xc
from tests import exchange_ref as xr
from tests.exchange_ref import bits
from tests.test_gpu_delta_exchange import d2h_u32, exchange_stats, host_allreduce, host_sparse_allreduce, make_shards
from tests.test_gpu_fold_masks import PAIR, check_invariant
from tests.test_gpu_vec_act import DevArray
from tests.test_gpu_vec_features import dyadic
from tests.tile_ref import tiles

pytestmark = pytest.mark.gpu

SA, QL, DQ = abi.ALGO_SARSA, abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q
NA, NT = abi.LOB_N_ACTIONS, 96
FOLD_MAX = 65537          # up to here Engine.fold_maps() is read back and tests/test_gpu_fold_masks.py check_invariant runs
BIG_TABLE = 1 << 20       # above this theta is read back from two ranks only (128 MiB a vector at 2^24 weights); the maps and the packed
                          # buffers, which are small, from all of them


def rho_of(eng):
    out = np.zeros(1)
    fn = eng.lib.lob_debug_rho
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]
    assert fn(eng.h, out.ctypes.data_as(C.c_void_p), 1) == 0
    return out[0]


class Ring:
    """Shards on one device + the test's own record of theta_sync / rho_sync.  exchange() performs one exchange of the ring's kind and
    asserts everything the reference predicts about it."""

    def __init__(self, algo, world, total, M=1 << 16, n_events=200, kind="dense", tweak=None, fold=False):
        self.engs, orcs = make_shards(algo, total=total, world=world, M=M, n_events=n_events, tweak=tweak)
        for o in orcs:
            o.close()
        self.algo, self.world, self.M, self.kind, self.fold = algo, world, M, kind, fold and M <= FOLD_MAX
        self.nv = 2 if algo in xc.TWO_VECTORS else 1
        self.rl = algo in xc.RL_ALGOS
        self.words = M // 32 + 1
        self.checked = list(range(world)) if M <= BIG_TABLE else [0, 1]     # (a prefix of the ranks: list index = rank)
        th = self.thetas()
        for t in th[1:]:
            np.testing.assert_array_equal(bits(t), bits(th[0]), err_msg="the shards start from one vector")
        self.sync = th[0]
        self.rho_sync = rho_of(self.engs[0]) if self.rl else 0.0
        self.log = []         # one dict per exchange: kind, count, union size, synced or not
        self.rho_moved = False

    def close(self):
        for e in self.engs:
            e.close()

    def thetas(self):
        """theta (double Q: [theta | theta_b]) of the checked ranks -- all of them unless the table is a big one."""
        engs = [self.engs[r] for r in self.checked]
        return [np.concatenate([e.theta(v) for v in range(self.nv)]) if self.nv > 1 else e.theta(0) for e in engs]

    def own_maps(self):
        return [d2h_u32(e.delta_sparse_maps(self.world)[0], self.words) for e in self.engs]

    # ---- the schedule's operations ----
    def step(self, n=1):
        for e in self.engs:
            e.td_step(n)

    def begin(self):
        for e in self.engs:
            e.td_step_begin()

    def end(self):
        for e in self.engs:
            e.td_step_end()

    def episode(self):
        for e in self.engs:
            e.clear_inventory(); e.handle_terminal(); e.reset()

    def update(self, rank, rows, actions, step, second=False):
        n = len(rows)
        dv, da, ds = DevArray((n, rows.shape[1]), np.float32), DevArray(n, np.int32), DevArray(n, np.float64)
        dv.upload(rows); da.upload(actions); ds.upload(step)
        self.engs[rank].vec_update(dv.ptr, n, da.ptr, ds.ptr, second=second)
        self.engs[rank].sync()
        for d in (dv, da, ds):
            d.free()

    # ---- one exchange, checked ----
    def exchange(self, tag, kind=None):
        kind = kind or self.kind
        before = self.thetas()
        info = self._dense(tag, before) if kind == "dense" else self._sparse(tag, before)
        if self.fold:   # (inside the half-open step as well: every writer of the exact map keeps the masks with it)
            for r, e in enumerate(self.engs):
                check_invariant(e, "%s: rank %d after the exchange" % (tag, r))
        info.update(kind=kind, before=before)
        self.log.append(info)
        return info

    def _dense(self, tag, before):
        nvM = self.nv * self.M
        rhos = [rho_of(e) for e in self.engs] if self.rl else None
        seen = {}
        host_allreduce(self.engs, seen)
        assert seen["count"] == nvM + (2 if self.rl else 0), (tag, seen["count"])
        exp = xr.dense_expected(before, self.sync)
        for r in self.checked:
            np.testing.assert_array_equal(bits(seen["deltas"][r][:nvM]), bits(exp["deltas"][r]), err_msg="%s: rank %d's delta buffer" % (tag, r))
        if len(self.checked) == self.world:
            np.testing.assert_array_equal(bits(seen["total"][:nvM]), bits(exp["total"]), err_msg=tag + ": the rank-order sum")
        # (what every rank must hold: the base + the sum the ranks were handed -- of all ranks' buffers, also where only some are checked)
        exp["total"] = seen["total"][:nvM]
        exp["theta"] = self.sync + exp["total"]
        after = self.thetas()
        for r in self.checked:
            np.testing.assert_array_equal(bits(after[r]), bits(exp["theta"]), err_msg="%s: theta of rank %d after the apply" % (tag, r))
        if self.rl:
            rexp = xr.rho_expected(rhos, self.rho_sync)
            for r in range(self.world):
                slots = seen["deltas"][r][nvM:]
                assert bits(slots[1:])[0] == bits([1.0])[0], "%s: rank %d: slot count - 1 is exactly 1.0 (rho_delta_begin_kernel ran)" % (tag, r)
                np.testing.assert_array_equal(bits(slots), bits(rexp["slots"][r]), err_msg="%s: rank %d's rho slots" % (tag, r))
            for r, e in enumerate(self.engs):
                assert bits([rho_of(e)])[0] == bits([rexp["rho"]])[0], "%s: rho of rank %d after the apply: %r, expected %r" % (tag, r, rho_of(e), rexp["rho"])
            self.rho_moved = self.rho_moved or rexp["rho"] != self.rho_sync or any(x != self.rho_sync for x in rhos)
            self.rho_sync = rexp["rho"]
        if self.algo in (SA, QL):   # the exact map afterwards holds every weight some rank has changed
            changed = np.flatnonzero(exp["total"] != 0.0)
            for r, m in enumerate(self.own_maps()):
                assert ((m[changed >> 5] >> (changed & 31).astype(np.uint32)) & 1).all(), "%s: rank %d's exact map misses exchanged weights" % (tag, r)
        self.sync = exp["theta"]
        return {"count": seen["count"], "union": None, "synced": True, "exp": exp}

    def _sparse(self, tag, before):
        st0 = exchange_stats(self.engs[0])
        seen = {}
        n = host_sparse_allreduce(self.engs, seen)
        st1 = exchange_stats(self.engs[0])
        synced = st1["synced"] == st0["synced"] + 1
        assert synced != (st1["no_sync"] == st0["no_sync"] + 1), (tag, st0, st1)
        exp = xr.sparse_expected(before, self.sync, seen["maps"], n)      # (the maps of all ranks; theta of the checked ones)
        nu = exp["idx"].size
        if len(self.checked) == self.world:
            np.testing.assert_array_equal(bits(seen["total"]), bits(exp["total"]), err_msg=tag + ": the rank-order sum")
        else:   # the sum the ranks were handed is of all ranks' packed buffers: the expectation goes by it
            moved, total = exp["moved"], seen["total"]
            for t, sy, b in zip(exp["theta"], exp["sync"], before):
                t[moved] = sy[moved] = self.sync[moved] + total[:moved.size]
                rest = np.ones(t.size, bool)
                rest[moved] = False
                assert np.array_equal(bits(t[rest]), bits(b[rest]))
            exp["total"] = total
        if synced:
            assert n == nu, "%s: a synchronised exchange carries the union: count %d, |union| %d" % (tag, n, nu)
        else:
            assert n == st1["fixed_count"], (tag, n, st1)
        for r in range(self.world):
            assert seen["packed"][r].size == n
            if r in self.checked:
                np.testing.assert_array_equal(bits(seen["packed"][r]), bits(exp["packed"][r]), err_msg="%s: rank %d's packed buffer" % (tag, r))
            if nu < n:
                assert (bits(seen["packed"][r][nu:]) == 0).all(), "%s: rank %d: +0.0 behind the union up to the count" % (tag, r)
        after = self.thetas()
        for r in self.checked:
            np.testing.assert_array_equal(bits(after[r]), bits(exp["theta"][r]), err_msg="%s: theta of rank %d after the apply" % (tag, r))
        for r, m in enumerate(self.own_maps()):
            assert ((m & exp["union"]) == exp["union"]).all(), "%s: rank %d's exact map does not hold the union" % (tag, r)
        for s in exp["sync"][1:]:
            assert np.array_equal(bits(s), bits(exp["sync"][0]))
        sync_before, self.sync = self.sync, exp["sync"][0]
        return {"count": n, "union": nu, "synced": synced, "exp": exp, "maps": seen["maps"], "stats": st1, "sync_before": sync_before}


def pair_env(monkeypatch):
    for k, v in PAIR.items():
        monkeypatch.setenv(k, v)


def four_exchanges(ring, tag, steps=(8, 12, 9, 16)):
    """Four exchanges 8-16 learner steps apart; the second and the fourth sit inside lob_td_step_begin / _end."""
    for k, n in enumerate(steps):
        mid = k % 2 == 1
        ring.step(n - 1 if mid else n)
        if mid:
            ring.begin()
        ring.exchange("%s exchange %d%s" % (tag, k, " (inside the step)" if mid else ""))
        if mid:
            ring.end()
    ring.step(2)      # ... and the shards go on from the exchanged weights
    assert any((t != 0).any() for t in ring.thetas()), tag + ": nothing was learned"


KINDS = ["dense", "sparse"]
ALGOS2 = [(SA, "sarsa"), (QL, "qlambda")]


# ---- 1. world sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,total", [(1, 13), (2, 13), (3, 13), (5, 13), (8, 13), (8, 8)], ids=lambda v: str(v))
@pytest.mark.parametrize("algo,name", ALGOS2, ids=[a[1] for a in ALGOS2])
@pytest.mark.parametrize("kind", KINDS)
def test_world_sizes_bit_for_bit(kind, algo, name, world, total):
    ring = Ring(algo, world, total, kind=kind)
    if kind == "sparse":
        assert all(e.delta_sparse_supported() for e in ring.engs)
    four_exchanges(ring, "%s %s world %d / %d books" % (kind, name, world, total))
    if kind == "sparse":
        assert all(i["union"] > 0 for i in ring.log)
    ring.close()


def test_the_gather_buffer_grows_with_the_world():
    """lob_delta_sparse_maps with world 2, then with world 5, on the same engines: the gather buffer of two slots is replaced by one
    of five (packing for five is refused until then), four exchanges of all five shards follow; at the end two of the shards
    exchange as a pair in the grown buffer.  (Every rank takes part in every exchange up to that last one: the ranks agree on the
    exchange's length from their common history of union sizes.)"""
    ring = Ring(QL, 5, 13, kind="sparse")
    lib = ring.engs[0].lib
    for e in ring.engs:
        own, gather, words = e.delta_sparse_maps(2)
        assert own and gather and words == ring.words
        p, cnt = C.c_void_p(), C.c_int64()
        assert lib.lob_delta_sparse_pack(e.h, 5, C.byref(p), C.byref(cnt)) == abi.LOB_EINVAL
        assert b"lob_delta_sparse_pack" in lib.lob_last_error()
    four_exchanges(ring, "world 2 -> 5")
    grown = [e.delta_sparse_maps(5)[1] for e in ring.engs]
    assert [e.delta_sparse_maps(2)[1] for e in ring.engs] == grown, "a smaller world goes into the grown buffer"
    pair = copy.copy(ring)
    pair.engs, pair.world, pair.checked, pair.log = ring.engs[:2], 2, [0, 1], []
    pair.step(3)
    info = pair.exchange("a pair in the buffer of five")
    assert info["union"] > 0
    ring.close()


# ---- 2. table sizes -------------------------------------------------------------------------------------------------------------------
SMALL_M = [1, 2, 31, 32, 33, 8191, 8192, 8193, 65537]
BIG_M = [8396863, (1 << 24) + 31]      # 1 026 map blocks (two per scan thread, the upper half of the threads idle) / 2 049 (three)


@pytest.mark.parametrize("M", SMALL_M)
@pytest.mark.parametrize("algo,name", ALGOS2, ids=[a[1] for a in ALGOS2])
@pytest.mark.parametrize("kind", KINDS)
def test_table_sizes_bit_for_bit(monkeypatch, kind, algo, name, M):
    """words = M / 32 + 1: an empty last word (M % 32 == 0), a single weight in it, a last word that starts a block of its own
    (M = 8 192 / 8 193: word 256), one map word in all.  On the forced pair path, so that the action masks are kept and read back."""
    pair_env(monkeypatch)
    ring = Ring(algo, 3, 6, M=M, kind=kind, fold=True)
    four_exchanges(ring, "%s %s M = %d" % (kind, name, M))
    if kind == "sparse":
        assert all(i["union"] > 0 for i in ring.log), [i["union"] for i in ring.log]
        assert all(i["union"] <= M for i in ring.log)
    ring.close()


def planted_rows(M, words):
    """Free-standing (row, action) pairs whose tiles set map bits where sparse_scan_kernel's multi-block path can go wrong, found on
    the CPU with oracle_tiles: in the table's last word, in the first and in the last word of one block, in a block >= 1 024."""
    rng = np.random.default_rng(99)
    rows = rng.uniform(-12, 12, size=(8192, engine.default_params().n_vars)).astype(np.float32)
    w = tiles(M, rows) >> 5                      # [n][9][96] map words
    picks = []

    def pick(mask, what):
        hit = np.argwhere(mask.any(axis=2))
        assert len(hit), "no candidate row has a tile " + what
        picks.append((int(hit[0][0]), int(hit[0][1])))
        return w[hit[0][0], hit[0][1]][mask[hit[0][0], hit[0][1]]][0]

    pick(w == words - 1, "in the table's last word")
    first = int(pick(((w & 255) == 0) & (w >= 1024 * 256) & (w + 255 < words), "in the first word of a whole block >= 1 024"))
    pick(w == first + 255, "in the last word of block %d" % (first >> 8))
    sel = np.array([p[0] for p in picks])
    return rows[sel], np.array([p[1] for p in picks], np.int32), np.array([0.5, -0.25, 0.125]), first >> 8


@pytest.mark.parametrize("M", BIG_M)
@pytest.mark.parametrize("algo,name", ALGOS2, ids=[a[1] for a in ALGOS2])
@pytest.mark.parametrize("kind", KINDS)
def test_tables_of_more_than_1024_map_blocks(kind, algo, name, M):
    """sparse_scan_kernel with several blocks per thread (per = 2 with trailing threads whose range starts behind the last block, per
    = 3) and a partial last block.  One shard receives an external update whose tiles lie in the table's last word, in the first and
    last word of one block and in blocks >= 1 024, so that the union has bits there by construction."""
    ring = Ring(algo, 3, 6, M=M, kind=kind)
    words = ring.words
    nb = (words + 255) // 256
    assert nb > 1024 and words % 256 != 0 and (nb + 1023) // 1024 == (2 if M < (1 << 24) else 3)
    rows, actions, step, block = planted_rows(M, words)
    ring.engs[0].kernel_timing(True)
    ring.update(1, rows, actions, step)
    four_exchanges(ring, "%s %s M = %d" % (kind, name, M), steps=(8, 8, 8, 8))
    if kind == "sparse":
        u = ring.log[0]["exp"]["union"]
        assert u[words - 1] != 0, "the union has no bit in the table's last word: nothing was checked"
        assert u[block * 256] != 0 and u[block * 256 + 255] != 0 and block >= 1024, "first / last word of block %d" % block
        assert (u[1024 * 256:] != 0).any()
        assert ring.engs[0].kernel_time_ms("delta_begin_kernel")[1] >= 8 and ring.engs[0].kernel_time_ms("delta_apply_kernel")[1] >= 4, \
            "the sparse kernels' launches under the exchange's two timer names (dense: 4 and 4); %d blocks is this test's arithmetic" % nb
    ring.close()


def test_zeros_behind_the_union_over_a_dense_exchanges_leftovers():
    """The packed vector lives in the dense exchange's scratch buffer.  A dense exchange fills all of it; the sparse exchanges that
    follow on the same engines must hand over +0.0 in [|union|, count) whenever they go by the fixed count."""
    ring = Ring(QL, 3, 12, kind="sparse")
    ring.step(12)
    ring.exchange("dense first", kind="dense")
    assert np.count_nonzero(ring.log[0]["exp"]["total"]) > 100
    for k in range(10):
        ring.step(2)
        ring.exchange("sparse %d behind the dense one" % k)
        if sum(1 for i in ring.log if not i["synced"] and i["union"] < i["count"]) >= 2:
            break
    loose = [i for i in ring.log if not i["synced"]]
    assert len(loose) >= 2 and all(i["union"] < i["count"] for i in loose), [(i["synced"], i["union"], i["count"]) for i in ring.log]
    ring.close()


# ---- 3. the cut of a short exchange -------------------------------------------------------------------------------------------------
def settle_fixed_count(ring):
    """One-step exchanges until the NEXT exchange will go by the fixed count too (lob_delta_sparse_pack: the last union size + twice
    its last increase fits): the engine's rule restated over the union sizes the test has seen."""
    prev = last = -1
    for k in range(14):
        ring.step(1)
        info = ring.exchange("settling %d" % k)
        if info["union"] != last:
            prev, last = last, info["union"]
        fixed = info["stats"]["fixed_count"]
        if info["stats"]["no_sync"] >= 1 and prev >= 0 and last + 2 * max(last - prev, 0) <= fixed:
            return fixed, last
    raise AssertionError("the fixed count did not settle: %r" % [(i["synced"], i["union"], i["count"]) for i in ring.log])


def rows_that_split_a_word(ring, fixed):
    """Rows for two ranks (dyadic steps) whose tiles, with the maps as they stand, make a union several times the fixed count in which
    entry `fixed` lies inside a word that has further bits behind it.  Chosen on the CPU: rows are added one by one until it holds."""
    M = ring.M
    rng = np.random.default_rng(4242)
    n_max = 8 * fixed // NT + 64
    rows = rng.uniform(-12, 12, size=(n_max, engine.default_params().n_vars)).astype(np.float32)
    actions = rng.integers(0, NA, size=n_max).astype(np.int32)
    step = dyadic(rng, n_max)
    step[step == 0.0] = 2.0 ** -20
    F = tiles(M, rows)[np.arange(n_max), actions]          # [n][96]
    have = np.unpackbits(xr.union_layout(ring.own_maps())[0].view(np.uint8), bitorder="little").astype(bool)
    for n in range(5 * fixed // NT, n_max):
        m = have.copy()
        m[F[:n].ravel()] = True
        idx = np.flatnonzero(m)
        if idx.size >= 4 * fixed and idx[fixed - 1] >> 5 == idx[fixed] >> 5:
            half = n // 2 + 8                                  # rank 0: rows [0, half), rank 2: rows [half - 16, n): sixteen on both
            return (rows[:half], actions[:half], step[:half]), (rows[half - 16:n], actions[half - 16:n], step[half - 16:n])
    raise AssertionError("no row count puts the cut inside a word")


def short_exchange(ring):
    """-> the info of an exchange whose union outgrew the fixed count several-fold, checked: which weights moved, which kept theta."""
    fixed, _ = settle_fixed_count(ring)
    st0 = exchange_stats(ring.engs[0])
    a, b = rows_that_split_a_word(ring, fixed)
    ring.update(0, *a)
    ring.update(2, *b)
    info = ring.exchange("the short exchange")
    idx = info["exp"]["idx"]
    assert not info["synced"] and info["count"] == fixed and info["union"] >= 4 * fixed, (info["synced"], info["count"], info["union"], fixed)
    assert idx[fixed - 1] >> 5 == idx[fixed] >> 5, "the cut falls between two words: entries %d | %d" % (idx[fixed - 1], idx[fixed])
    after = ring.thetas()
    late = idx[fixed:]
    for r in range(ring.world):   # (ring.exchange has compared every weight with the reference; here the two halves by name)
        np.testing.assert_array_equal(bits(after[r][late]), bits(info["before"][r][late]), err_msg="rank %d: a late entry keeps its theta" % r)
    moved = idx[:fixed]
    assert all(np.array_equal(bits(after[0][moved]), bits(t[moved])) for t in after), "the entries that travelled agree on every rank"
    assert any(not np.array_equal(bits(after[0][late]), bits(t[late])) for t in after), "the surplus has not travelled yet"
    assert exchange_stats(ring.engs[0])["overflows"] == st0["overflows"]
    info["st0"] = st0
    return info


def whole_exchange(short):
    """What ONE exchange of the whole union would have left, from the state before the short one."""
    return xr.sparse_expected(short["before"], short["sync_before"], short["maps"], short["union"])["theta"][0]


def test_the_cut_of_a_short_exchange(monkeypatch):
    monkeypatch.setenv("LOB_SPX_COUNT", "64")
    ring = Ring(QL, 3, 12, kind="sparse")
    short = short_exchange(ring)
    nxt = ring.exchange("the exchange behind the short one")
    st = exchange_stats(ring.engs[0])
    assert nxt["synced"] and nxt["count"] == nxt["union"] >= short["union"], (nxt["synced"], nxt["count"], nxt["union"])
    assert st["overflows"] == short["st0"]["overflows"] + 1, (short["st0"], st)
    after = ring.thetas()
    for t in after[1:]:
        np.testing.assert_array_equal(bits(t), bits(after[0]))
    np.testing.assert_array_equal(bits(after[0]), bits(whole_exchange(short)), err_msg="as if nothing had been late")
    ring.close()


def test_the_surplus_of_a_short_exchange_crosses_a_reset(monkeypatch):
    """Short exchange, end of the episode, lob_reset, exchange: the late entries' theta - theta_sync outlives the reset."""
    monkeypatch.setenv("LOB_SPX_COUNT", "64")
    ring = Ring(QL, 3, 12, kind="sparse")
    short = short_exchange(ring)
    kept = ring.thetas()
    ring.episode()
    for r, t in enumerate(ring.thetas()):
        np.testing.assert_array_equal(bits(t), bits(kept[r]), err_msg="the weights outlive the episode")
    nxt = ring.exchange("the first exchange of episode 2")
    assert nxt["synced"] and nxt["count"] == nxt["union"] >= short["union"]
    assert exchange_stats(ring.engs[0])["overflows"] == short["st0"]["overflows"] + 1
    after = ring.thetas()
    for t in after[1:]:
        np.testing.assert_array_equal(bits(t), bits(after[0]))
    np.testing.assert_array_equal(bits(after[0]), bits(whole_exchange(short)), err_msg="nothing was lost across the reset")
    ring.step(4)
    ring.exchange("four steps into episode 2")
    ring.close()


# ---- 4. the oracle's schedule of the same shards ------------------------------------------------------------------------------------
def compare_with_oracle(ring, oring, tag, weights=False):
    """Tolerances: the ones the project uses for shared weights (theta 1e-9 / 1e-15, TD errors 1e-9 / 1e-12, rho 1e-9 / 1e-12)."""
    stepped_any = False
    for r, (e, o) in enumerate(zip(ring.engs, oring.orcs)):
        recs = o.recs()
        stepped = e.stepped().astype(bool)
        stepped_any = stepped_any or bool(stepped.any())
        np.testing.assert_array_equal(e.rng_counters(), recs["rng_ctr"], err_msg="%s: rank %d rng counters" % (tag, r))
        if stepped.any():
            np.testing.assert_array_equal(e.last_actions()[stepped], recs["action"][stepped], err_msg="%s: rank %d actions" % (tag, r))
            np.testing.assert_allclose(e.last_td()[stepped], recs["td"][stepped], rtol=1e-9, atol=1e-12, err_msg="%s: rank %d TD errors" % (tag, r))
        if weights:
            for v, get in enumerate(oring.views):
                np.testing.assert_allclose(e.theta(v), get(o), rtol=1e-9, atol=1e-15, err_msg="%s: rank %d weight vector %d" % (tag, r, v))
            if ring.rl:
                np.testing.assert_allclose(rho_of(e), o.rho()[0], rtol=1e-9, atol=1e-12, err_msg="%s: rank %d rho" % (tag, r))
    return stepped_any


def run_schedule(ring, cfg, tag):
    """The case's schedule (tests/exchange_cases.py walk) on the engines and on the oracle shards, side by side.
    -> the "until_done" periods, decided by the oracle's cursors."""
    oring = xc.OracleRing(cfg)
    n_step, periods, mid = 0, [], False
    for ev in xc.walk(cfg["ops"], oring.cursors, periods):
        if ev[0] == "update":
            rows, actions, step = xc.update_rows(cfg, ev[2])
            for second in ((False, True) if ring.nv == 2 else (False,)):
                ring.update(ev[1], rows, actions, step, second=second)
        elif ev[0] == "x":
            ring.exchange("%s exchange %d%s" % (tag, len(ring.log), " (inside the step)" if mid else ""))
        else:
            {"step": ring.step, "begin": ring.begin, "end": ring.end, "episode": ring.episode}[ev[0]]()
        oring.apply(ev)
        if ev[0] == "begin":
            mid = True
        elif ev[0] in ("step", "end"):
            mid = False
            compare_with_oracle(ring, oring, "%s step %d" % (tag, n_step), weights=ev[0] == "end")
            n_step += 1
        elif ev[0] == "x" and not mid:
            compare_with_oracle(ring, oring, "%s behind exchange %d" % (tag, len(ring.log) - 1), weights=True)
    compare_with_oracle(ring, oring, tag + " at the end", weights=True)
    assert any((get(oring.orcs[0]) != 0).any() for get in oring.views)
    oring.close()
    return periods


def ring_of(cfg, kind, **kw):
    return Ring(cfg["algo"], cfg["world"], cfg["total"], M=cfg["M"], n_events=cfg["n_events"], kind=kind, tweak=xc.tweak_of(cfg), **kw)


def sparse_is_refused(ring):
    lib = ring.engs[0].lib
    for e in ring.engs:
        assert not e.delta_sparse_supported()
        own, gather, words = C.c_void_p(), C.c_void_p(), C.c_int64()
        assert lib.lob_delta_sparse_maps(e.h, ring.world, C.byref(own), C.byref(gather), C.byref(words)) == abi.LOB_ESTATE
        assert b"lob_delta_sparse" in lib.lob_last_error()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["r_learn", "online_r_learn", "double_r_learn"])
def test_average_reward_agents(name, world):
    """rho_delta_begin_kernel / rho_delta_apply_kernel: the two slots behind the weights, [rho - rho_sync, 1.0]; the sum's second slot is
    the number of ranks and rho <- rho_sync + the mean change.  Bit for bit against rho_expected (and the weights, theta_b included,
    against dense_expected) at every exchange, outside and inside the half-open step; the trajectory against the oracle shards."""
    cfg = xc.CASES["%s-w%d" % (name, world)]
    ring = ring_of(cfg, "dense")
    sparse_is_refused(ring)
    assert ring.engs[0].delta_begin()[1] == ring.nv * ring.M + 2
    run_schedule(ring, cfg, "%s world %d" % (name, world))
    assert len(ring.log) == 4 and ring.rho_moved, "rho never moved: the test exercises nothing"
    ring.close()


def test_double_q_exchanged_inside_the_half_open_step():
    cfg = xc.CASES["double_q-inside"]
    ring = ring_of(cfg, "dense")
    sparse_is_refused(ring)
    assert ring.engs[0].delta_begin()[1] == 2 * ring.M
    run_schedule(ring, cfg, "double Q")
    assert len(ring.log) == 4
    for v in (0, 1):
        assert np.count_nonzero(ring.engs[0].theta(v)) > 100
    ring.close()


# ---- 5. lob_vec_update and the exchange ---------------------------------------------------------------------------------------------
UPDATE_FORMS = [("dense", QL, False), ("sparse", QL, False), ("dense", SA, False), ("sparse", SA, False), ("dense", DQ, True)]
UPDATE_IDS = ["dense-qlambda", "sparse-qlambda", "dense-sarsa", "sparse-sarsa", "dense-double_q-second"]


def update_case(M, seed, n=64):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-12, 12, size=(n, engine.default_params().n_vars)).astype(np.float32)
    actions = rng.integers(0, NA, size=n).astype(np.int32)
    step = dyadic(rng, n)
    step[step == 0.0] = 2.0 ** -20
    inc = np.zeros(M)
    np.add.at(inc, tiles(M, rows)[np.arange(n), actions].ravel(), np.repeat(step, NT))
    return rows, actions, step, inc


@pytest.mark.parametrize("ranks", [(0,), (0, 2)], ids=["one-rank", "two-ranks"])
@pytest.mark.parametrize("kind,algo,second", UPDATE_FORMS, ids=UPDATE_IDS)
def test_an_external_update_travels_with_the_next_exchange(kind, algo, second, ranks):
    """lob_vec_update does NOT move the multi-GPU base: the update is a local change and the next exchange carries it (on the sparse
    path through the exact-map bit vec_feat_mark sets).  Fresh shards (every weight +0.0, so base + update is the update, exactly:
    dyadic steps), an update of free-standing rows on one rank, or the same rows on two; one exchange; every rank holds the sum.
    A second exchange with nobody stepping changes nothing: the base moved with the first."""
    ring = Ring(algo, 3, 6, kind=kind)
    M = ring.M
    rows, actions, step, inc = update_case(M, 61)
    assert (bits(ring.sync) == 0).all() and np.count_nonzero(inc) > 3000
    for r in ranks:
        ring.update(r, rows, actions, step, second=second)
    want = np.zeros(ring.nv * M)
    want[M if second else 0:][:M] = len(ranks) * inc          # (exact: dyadic)
    mine = ring.thetas()
    for r in range(3):
        np.testing.assert_array_equal(bits(mine[r]), bits(want / len(ranks) if r in ranks else np.zeros(ring.nv * M)), err_msg="before the exchange: rank %d" % r)
    info = ring.exchange("behind the update")
    if kind == "sparse":
        assert info["union"] >= np.count_nonzero(inc)
    for r, t in enumerate(ring.thetas()):
        np.testing.assert_array_equal(bits(t), bits(want), err_msg="rank %d holds base + update" % r)
    ring.exchange("nobody stepped")
    for r, t in enumerate(ring.thetas()):
        np.testing.assert_array_equal(bits(t), bits(want), err_msg="rank %d after the second exchange: the base moved with the first" % r)
    ring.step(4)
    ring.exchange("four learner steps on the updated weights")
    ring.close()


@pytest.mark.parametrize("kind,name", [("dense", "qlambda"), ("sparse", "qlambda"), ("dense", "sarsa"), ("sparse", "sarsa"), ("dense", "double_q")])
def test_an_update_then_learner_steps_then_the_exchange(kind, name):
    """An update on one rank, learner steps on all, the exchange, more steps: against the oracle shards, where the increment is
    added to that shard's weight view (tests/test_gpu_vec_features.py external_update is the model)."""
    cfg = xc.CASES["update-" + name]
    ring = ring_of(cfg, kind)
    run_schedule(ring, cfg, "update %s %s" % (kind, name))
    assert len(ring.log) == 3
    ring.close()


# ---- 6. ranks that finish at different times, and the episode boundary --------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("sparse", "unequal-ends"), ("dense", "unequal-ends"), ("sparse", "unequal-ends-sarsa"), ("dense", "unequal-ends-sarsa")])
def test_ranks_that_finish_at_different_times(kind, name):
    """One shard's books have all ended several exchange periods before the others': it goes on exchanging (zero deltas) until the
    last book stops.  Then the episode ends on every rank, and an exchange comes BEFORE the first step of episode 2: nobody has
    learned, the sum is zero and theta is bit-identical.  Then 16 steps and an exchange, against the oracle."""
    cfg = xc.CASES[name]
    ring = ring_of(cfg, kind)
    periods = run_schedule(ring, cfg, "%s %s" % (name, kind))
    first_idle = [min(k for k, m in enumerate(periods) if not m[r]) for r in range(3)]
    assert max(first_idle) - min(first_idle) >= 3, "no shard ended several periods before the others: %r" % (first_idle,)
    k = len(periods)          # the exchange behind the reset: log entry k
    boundary = ring.log[k]
    exp = boundary["exp"]
    assert not np.asarray(exp["total"]).any(), "nobody learned between the last exchange and the reset: the sum is zero"
    theta_after = exp["theta"] if boundary["kind"] == "dense" else exp["theta"][0]
    np.testing.assert_array_equal(bits(theta_after), bits(boundary["before"][0]), err_msg="theta across the exchange before episode 2's first step")
    assert len(ring.log) == k + 2
    ring.close()


@pytest.mark.parametrize("kind", KINDS)
def test_an_exchange_right_after_the_first_reset(kind):
    """lob_delta_init and an exchange on a freshly reset engine, no step made: lob_reset has emptied both memo lists (mk_count), so
    the memo launch behind the apply walks an empty list under the new weight version -- the call sequence lob_theta_set takes.  Every
    delta is +0.0; sixteen learner steps behind it follow the oracle."""
    cfg = xc.case(QL, 3, ops=[("x",), ("step", 16), ("x",), ("step", 4)])
    ring = ring_of(cfg, kind)
    run_schedule(ring, cfg, "fresh " + kind)
    first = ring.log[0]["exp"]
    assert not np.asarray(first["total"]).any()
    ring.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = abi.load()
    p = engine.default_params()
    p.memory_size = 1 << 12
    g = engine.default_gen_params()
    g.n_events = 100
    ptr, n = C.c_void_p(), C.c_int64()
    # private theta: no common vector to exchange
    p.theta_mode = abi.THETA_PRIVATE
    e = engine.Engine(p, 2)
    assert lib.lob_delta_init(e.h) == abi.LOB_EINVAL and b"shared theta" in lib.lob_last_error()
    e.close()
    p.theta_mode = abi.THETA_SHARED
    e = engine.Engine(p, 2)
    e.load_events(engine.gen_stream_host(g, p.depth, p.max_trades, 0, 2))
    e.reset()
    # before lob_delta_init
    assert lib.lob_delta_begin(e.h, C.byref(ptr), C.byref(n)) == abi.LOB_ESTATE and b"lob_delta_init" in lib.lob_last_error()
    assert lib.lob_delta_apply(e.h) == abi.LOB_ESTATE and b"lob_delta_init" in lib.lob_last_error()
    assert lib.lob_delta_sparse_apply(e.h) == abi.LOB_EINVAL and b"no packed exchange" in lib.lob_last_error()
    e.delta_init()
    assert lib.lob_delta_sparse_apply(e.h) == abi.LOB_EINVAL, "no pack yet"
    assert lib.lob_delta_sparse_pack(e.h, 1, C.byref(ptr), C.byref(n)) == abi.LOB_EINVAL, "no lob_delta_sparse_maps yet"
    e.delta_sparse_maps(2)
    assert lib.lob_delta_sparse_pack(e.h, 3, C.byref(ptr), C.byref(n)) == abi.LOB_EINVAL and b"world size" in lib.lob_last_error()
    e.td_step(3)      # the refused calls left the engine usable
    e.sync()
    e.close()
