"""The per-sum action masks of the pair learn kernel (DevState::theta_nzm) against the maps they summarise.

learn_q_pair_kernel resolves a tiling that passed the folded map with ONE 16-bit mask per hash sum instead of nine exact-map
words.  That is only right while, for every tile group g, hash sum s and action a,

    mask[g][s] bit a   ==  exact bit (s + term[g][a]) mod M          folded[g] bit s  ==  (mask[g][s] != 0)

hold at every point a learn kernel can run -- the masks are kept by the sites that keep the folded map: nzd_mark (every first
write of a weight: the act / env / trace kernels, both weight-exchange kernels) and rebuild_nzd_kernel (lob_theta_set).  Here the
three tables are read back through lob_debug_fold_maps (Engine.fold_maps, after a stream synchronisation) and compared entry for
entry after each of those: learner steps on the forced pair path -- a dense small table (lists past the kernel's capacity, books
handed back) and a sparse one, a full and a partial block and a single book --, a reset into a second episode, a weight load,
and one weight exchange of each kind between two shards on one device."""
import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests.test_gpu_delta_exchange import host_allreduce, host_sparse_allreduce, make_shards

pytestmark = pytest.mark.gpu

PAIR = {"LOB_Q_LANES": "1", "LOB_Q_PAIR": "1", "LOB_FUSE_ACT": "1"}
ALGOS = [abi.ALGO_QLAMBDA, abi.ALGO_SARSA, abi.ALGO_DOUBLE_Q]
IDS = ["qlambda", "sarsa", "double_q"]


def check_invariant(eng, tag, min_written=1):
    m = eng.fold_maps()
    M = int(eng.M)
    s = np.arange(M, dtype=np.int64)
    exact, written = m["exact"], 0
    assert not (m["masks"] >> 9).any(), tag + ": mask bits beyond the nine actions"
    for g in range(2):
        masks = m["masks"][g].astype(np.uint32)
        for a in range(9):
            f = (s + int(m["terms"][g][a])) % M
            want = (exact[f >> 5] >> (f & 31).astype(np.uint32)) & 1
            have = (masks >> a) & 1
            bad = np.flatnonzero(want != have)
            assert bad.size == 0, "%s: group %d action %d: mask bit != exact bit at %d sums, first s = %d (exact %d, mask %d)" % (
                tag, g + 1, a, bad.size, bad[0], want[bad[0]], have[bad[0]])
            written = max(written, int(want.sum()))
        folded = (m["folded"][g][s >> 5] >> (s & 31).astype(np.uint32)) & 1
        bad = np.flatnonzero(folded != (masks != 0))
        assert bad.size == 0, "%s: group %d: folded bit != (mask != 0) at %d sums, first s = %d" % (tag, g + 1, bad.size, bad[0])
    assert written >= min_written, tag + ": the maps are empty -- nothing was checked"
    return written


def make_engine(B, algo, M, n_events=400):
    p = engine.default_params()
    p.depth, p.max_trades = 10, 2
    p.algo, p.theta_mode, p.memory_size = algo, abi.THETA_SHARED, M
    g = engine.default_gen_params()
    g.n_events = n_events
    eng = engine.Engine(p, B)
    eng.load_events(engine.gen_stream_host(g, p.depth, 2, 0, B))
    return p, eng


@pytest.mark.parametrize("M", [4099, 65536])
@pytest.mark.parametrize("B", [192, 1])
@pytest.mark.parametrize("algo", ALGOS, ids=IDS)
def test_masks_after_learner_steps_and_across_a_reset(monkeypatch, algo, B, M):
    for k, v in PAIR.items():
        monkeypatch.setenv(k, v)
    p, eng = make_engine(B, algo, M)
    eng.reset()
    check_invariant(eng, "after the reset", min_written=0)
    eng.td_step(30)
    w1 = check_invariant(eng, "after 30 steps")
    # the weights (and with them the maps) outlive the episode
    eng.clear_inventory()
    eng.handle_terminal()
    eng.reset()
    w2 = check_invariant(eng, "after the reset into episode 2")
    assert w2 >= w1    # (monotone; the first action's tiles may be marked already)
    eng.td_step(10)
    assert check_invariant(eng, "10 steps into episode 2") >= w2
    eng.close()


@pytest.mark.parametrize("M", [4099, 65536])
@pytest.mark.parametrize("algo", [abi.ALGO_QLAMBDA, abi.ALGO_DOUBLE_Q], ids=["qlambda", "double_q"])
def test_masks_after_a_weight_load(monkeypatch, algo, M):
    """lob_theta_set: rebuild_nzx_kernel + rebuild_nzd_kernel (gather form), on top of the bits the maps already hold."""
    for k, v in PAIR.items():
        monkeypatch.setenv(k, v)
    p, eng = make_engine(192, algo, M)
    eng.reset()
    eng.td_step(5)
    w0 = check_invariant(eng, "before the load")
    rng = np.random.default_rng(31)
    th = np.zeros(M)
    idx = rng.choice(M, size=M // 50, replace=False)
    th[idx] = rng.normal(0.0, 0.01, size=idx.size)
    th[[0, M - 1]] = 0.5   # (the table's first and last weight: the wrap-around of (s + term) mod M on both sides)
    eng.set_theta(th)
    w1 = check_invariant(eng, "after the load")
    assert w1 >= max(w0, idx.size // 9)
    if algo == abi.ALGO_DOUBLE_Q:
        thb = np.zeros(M)
        thb[rng.choice(M, size=M // 50, replace=False)] = 0.01
        eng.set_theta(thb, 1)   # (one pair of maps for both vectors)
        assert check_invariant(eng, "after the load of theta_b") >= w1
    eng.td_step(5)
    check_invariant(eng, "5 steps after the load")
    eng.close()


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_masks_after_a_weight_exchange(monkeypatch, kind):
    """delta_apply_kernel / sparse_apply_kernel set exact bits for the weights other ranks have written: two shards on one
    device, as tests/test_gpu_delta_exchange.py runs them."""
    for k, v in PAIR.items():
        monkeypatch.setenv(k, v)
    engs, orcs = make_shards(abi.ALGO_QLAMBDA, M=1 << 16)
    for o in orcs:
        o.close()
    for e in engs:
        e.td_step(16)
    before = [check_invariant(e, "shard %d before the exchange" % r) for r, e in enumerate(engs)]
    if kind == "dense":
        host_allreduce(engs)
    else:
        assert all(e.delta_sparse_supported() for e in engs)
        host_sparse_allreduce(engs)
    after = [check_invariant(e, "shard %d after the %s exchange" % (r, kind)) for r, e in enumerate(engs)]
    assert all(a >= b for a, b in zip(after, before)) and any(a > b for a, b in zip(after, before)), (before, after)
    for e in engs:
        e.td_step(4)
    for r, e in enumerate(engs):
        check_invariant(e, "shard %d, 4 steps after the %s exchange" % (r, kind))
        e.close()
