"""tests/exchange_ref.py on the CPU: the numpy restatement of the weight exchange against a per-bit Python loop, and
oracle_set_rho (the oracle's half of the shared-rho exchange) against the plain oracle."""
import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import exchange_ref as xr
from tests import oracle_lib as ol

WORDS = [1, 2, 256, 257, 2049]


def naive_union(maps):
    words = len(maps[0])
    u, idx = [0] * words, []
    for w in range(words):
        for b in range(32):
            if any((int(m[w]) >> b) & 1 for m in maps):
                u[w] |= 1 << b
                idx.append(32 * w + b)
    return np.array(u, np.uint32), np.array(idx, np.int64)


def special_maps(words, M):
    """An all-zero map, a full one (the table's valid bits), only bit 0, only the last valid bit."""
    zero = np.zeros(words, np.uint32)
    full = np.full(words, 0xFFFFFFFF, np.uint32)
    full[-1] = (1 << (M & 31)) - 1          # (words = M / 32 + 1: the last word holds M % 32 weights, none when M % 32 == 0)
    first, last = zero.copy(), zero.copy()
    first[0] = 1
    last[(M - 1) >> 5] = np.uint32(1) << np.uint32((M - 1) & 31)
    return {"zero": zero, "full": full, "first": first, "last": last}


def table_sizes(words):
    """The three kinds of table with this many map words: an empty last word, one weight in it, 31 weights in it."""
    return [M for M in (32 * (words - 1), 32 * (words - 1) + 1, 32 * words - 1) if M >= 1]


@pytest.mark.parametrize("words", WORDS)
def test_union_layout_against_the_per_bit_loop(words):
    rng = np.random.default_rng(100 + words)
    for M in table_sizes(words):
        assert M // 32 + 1 == words
        sp = special_maps(words, M)
        valid = sp["full"]
        rnd = [rng.integers(0, 1 << 32, size=words, dtype=np.uint64).astype(np.uint32) & valid for _ in range(3)]
        thin = [m & rng.integers(0, 1 << 32, size=words, dtype=np.uint64).astype(np.uint32) & rnd[0] for m in rnd]
        cases = [[sp["zero"]], [sp["full"]], [sp["first"]], [sp["last"]], [sp["zero"], sp["first"], sp["last"]], rnd, thin,
                 [sp["zero"]] * 8, thin + [sp["last"]], [sp["full"], rnd[0]]]
        for maps in cases:
            u, idx = xr.union_layout(maps)
            nu, nidx = naive_union(maps)
            np.testing.assert_array_equal(u, nu)
            np.testing.assert_array_equal(idx, nidx)
            assert idx.dtype == np.int64 and (idx.size == 0 or idx.max() < M)
        assert xr.union_layout([sp["zero"]])[1].size == 0
        assert xr.union_layout([sp["full"]])[1].size == M
        np.testing.assert_array_equal(xr.union_layout([sp["first"], sp["last"]])[1], np.unique([0, M - 1]))


def naive_sparse(thetas, syncs, maps, count):
    _, idx = naive_union(maps)
    packed = [[0.0] * count for _ in thetas]
    for r, (t, s) in enumerate(zip(thetas, syncs)):
        for p, f in enumerate(idx):
            if p < count:
                packed[r][p] = t[f] - s[f]
    total = [0.0] * count
    for p in range(count):
        acc = packed[0][p]
        for r in range(1, len(thetas)):
            acc = acc + packed[r][p]
        total[p] = acc
    after = [np.array(t, copy=True) for t in thetas]
    sync_after = [np.array(s, copy=True) for s in syncs]
    for r in range(len(thetas)):
        for p, f in enumerate(idx):
            if p < count:
                after[r][f] = syncs[r][f] + total[p]
                sync_after[r][f] = after[r][f]
    return idx, np.array(packed).reshape(len(thetas), count), np.array(total), after, sync_after


@pytest.mark.parametrize("words", WORDS)
def test_sparse_expected_against_the_per_entry_loop(words):
    M = 32 * words - 1 if words < 2049 else 65537
    rng = np.random.default_rng(200 + words)
    world = 3
    sync = rng.standard_normal(M)
    sync[rng.random(M) < 0.5] = 0.0
    maps, thetas = [], []
    for r in range(world):
        t = sync.copy()
        w = rng.random(M) < 0.15
        t[w] += rng.standard_normal(int(w.sum()))
        t[min(3, M - 1)] = -0.0                      # (a sign the sum must keep)
        m = np.zeros(words * 32, np.uint8)
        m[:M][w] = 1
        m[min(3, M - 1)] = 1
        if M > 40:
            m[40] = 1                                # marked, never written: its delta is +0.0
        maps.append(np.packbits(m, bitorder="little").view("<u4").astype(np.uint32))
        thetas.append(t)
    n = xr.union_layout(maps)[1].size
    for count in sorted({0, 1, n // 2, max(n - 1, 0), n, n + 5}):
        got = xr.sparse_expected(thetas, sync, maps, count)
        idx, packed, total, after, sync_after = naive_sparse(thetas, [sync] * world, maps, count)
        np.testing.assert_array_equal(got["idx"], idx)
        np.testing.assert_array_equal(got["moved"], idx[:count])
        np.testing.assert_array_equal(xr.bits(got["total"]), xr.bits(total))
        for r in range(world):
            np.testing.assert_array_equal(xr.bits(got["packed"][r]), xr.bits(packed[r]))
            np.testing.assert_array_equal(xr.bits(got["theta"][r]), xr.bits(after[r]))
            np.testing.assert_array_equal(xr.bits(got["sync"][r]), xr.bits(sync_after[r]))
            assert (xr.bits(got["packed"][r][min(count, n):]) == 0).all(), "behind the union: +0.0"
            rest = np.setdiff1d(np.arange(M), idx[:count])
            np.testing.assert_array_equal(xr.bits(got["theta"][r][rest]), xr.bits(thetas[r][rest]), err_msg="every other weight as before")
    # one base per rank is accepted as well
    a = xr.sparse_expected(thetas, [sync] * world, maps, n)
    b = xr.sparse_expected(thetas, sync, maps, n)
    for r in range(world):
        np.testing.assert_array_equal(xr.bits(a["theta"][r]), xr.bits(b["theta"][r]))


def test_a_count_that_cuts_inside_a_word_keeps_exactly_the_first_indices():
    words, M = 257, 8193
    m0, m1 = np.zeros(words, np.uint32), np.zeros(words, np.uint32)
    m0[0], m0[3], m1[3], m1[255], m1[256] = 0x80000001, 0x0000F0F0, 0x00000F00, 0xFFFFFFFF, 1
    want = [0, 31] + [96 + b for b in (4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)] + [255 * 32 + b for b in range(32)] + [8192]
    _, idx = xr.union_layout([m0, m1])
    assert idx.tolist() == want
    sync = np.arange(M, dtype=np.float64)
    thetas = [sync + 1.0, sync + 0.5]
    for count in (5, 14, 15, 30, 45):     # inside word 3, its last set bit, the first bit of word 255, inside it, one short of its end
        e = xr.sparse_expected(thetas, sync, [m0, m1], count)
        assert e["moved"].tolist() == want[:count]
        word = want[count - 1] >> 5
        assert count in (14,) or any(f >> 5 == word for f in want[count:]), "the cut leaves bits of the same word behind"
        for r in range(2):
            moved = np.zeros(M, bool)
            moved[want[:count]] = True
            np.testing.assert_array_equal(e["theta"][r][moved], sync[moved] + 1.5)
            np.testing.assert_array_equal(xr.bits(e["theta"][r][~moved]), xr.bits(thetas[r][~moved]))
            np.testing.assert_array_equal(xr.bits(e["sync"][r][~moved]), xr.bits(sync[~moved]))
            assert e["packed"][r].size == count and (e["packed"][r] == (1.0, 0.5)[r]).all()


def test_dense_and_rho_expected():
    rng = np.random.default_rng(7)
    sync = rng.standard_normal(1000)
    thetas = [sync + rng.standard_normal(1000) * (rng.random(1000) < 0.3) for _ in range(5)]
    thetas[0][0], sync[0] = -0.0, 0.0
    d = xr.dense_expected(thetas, sync)
    for i in range(0, 1000, 7):
        acc = thetas[0][i] - sync[i]
        for r in range(1, 5):
            acc = acc + (thetas[r][i] - sync[i])
        assert xr.bits(d["total"][i:i + 1])[0] == xr.bits(np.array([acc]))[0]
        assert xr.bits(d["theta"][i:i + 1])[0] == xr.bits(np.array([sync[i] + acc]))[0]
    assert len(d["deltas"]) == 5 and all((x == t - sync).all() for x, t in zip(d["deltas"], thetas))
    one = xr.dense_expected([thetas[0]], sync)      # one rank: its own delta, -0.0 kept
    assert xr.bits(one["total"][:1])[0] == xr.bits(np.array([-0.0]))[0]
    r = xr.rho_expected([0.25, 0.5, 1.0], 0.125)
    assert all(s[1] == 1.0 for s in r["slots"]) and r["total"].tolist() == [0.125 + 0.375 + 0.875, 3.0]
    assert r["rho"] == 0.125 + (0.125 + 0.375 + 0.875) / 3.0
    assert xr.rho_expected([0.3], 0.1)["rho"] == 0.1 + (0.3 - 0.1) / 1.0


@pytest.mark.parametrize("algo", [abi.ALGO_R_LEARN, abi.ALGO_ONLINE_R_LEARN, abi.ALGO_DOUBLE_R_LEARN])
def test_oracle_set_rho_one_shard_schedule_is_the_plain_oracle(algo):
    """One shard that `exchanges` every 8 steps -- rho <- rho_sync + (rho - rho_sync) / 1 (rho_expected), written back with
    oracle_set_rho -- walks the plain oracle's trajectory bit for bit: one rank's exchange hands back the rho it read (asserted
    here for every exchange of the schedule), and get-then-set leaves the learner where it was."""
    p = engine.default_params()
    p.algo, p.theta_mode, p.memory_size, p.beta, p.epsilon = algo, abi.THETA_SHARED, 1 << 16, 0.02, 0.4
    g = engine.default_gen_params()
    g.n_events = 300
    rec = engine.gen_stream_host(g, p.depth, p.max_trades, 0, 12)
    plain, shard = ol.Oracle(p, rec), ol.Oracle(p, rec)
    plain.reset(); shard.reset()
    moved, rho_sync = False, 0.0
    for k in range(6):
        plain.td_step(8); shard.td_step(8)
        rho = shard.rho()[0]
        np.testing.assert_array_equal(xr.bits(shard.rho()), xr.bits(plain.rho()))
        moved = moved or rho != 0.0
        new = xr.rho_expected([rho], rho_sync)["rho"]
        np.testing.assert_array_equal(xr.bits([new]), xr.bits([rho]), err_msg="one rank: the exchanged rho is the rho it read")
        shard.set_rho([new])
        np.testing.assert_array_equal(xr.bits(shard.rho()), xr.bits([new]))
        rho_sync = new
        a, b = plain.recs(), shard.recs()
        np.testing.assert_array_equal(a["action"], b["action"])
        np.testing.assert_array_equal(xr.bits(a["td"]), xr.bits(b["td"]))
        np.testing.assert_array_equal(xr.bits(plain.theta(0)), xr.bits(shard.theta(0)))
    assert moved, "rho never moved: the test exercises nothing"
    # ... and a value that was not read is the one returned; one entry too many is refused
    shard.set_rho([0.625])
    assert shard.rho()[0] == 0.625
    two = np.zeros(2)
    assert shard.lib.oracle_set_rho(shard.h, ol.ptr(two), 2) == -1 and shard.rho()[0] == 0.625
    plain.close(); shard.close()
