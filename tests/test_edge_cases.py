"""tests/edge_cases.py on the CPU: what tests/test_gpu_edges.py takes for granted about its inputs.

* The shared-theta sweeps there (look-backs, policy / reward) compare TD errors and weights beside a shadow oracle whose weights
  are nudged by 1e-13, and a case whose shadow takes another action proves nothing from that step on.  At most one case in ten
  of a sweep may end that way (the cap of tests/test_gpu_steady.py).  That is a property of the cases, not of the engine: here the
  oracle runs against its shadow alone, over the same cases and the same schedule.
* The crafted batch fills all eight trade slots of a merged list: lob_validate_stream passes it and refuses a ninth key, and the
  oracle's books consume the events that carry the lists.
* tests/hard_streams.harden makes valid streams at the depths and trade-slot counts that file runs."""
import ctypes as C

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import edge_cases as ec
from tests import exchange_cases as xc
from tests import hard_streams as hs
from tests import oracle_lib as ol

EPISODES, STEPS = 2, 60      # the schedule of tests/test_gpu_edges.py


def validate(rec, D, T):
    return abi.load().lob_validate_stream(rec.ctypes.data_as(C.c_void_p), D, T, rec.shape[0], rec.shape[1])


def test_lookback_sweep_is_not_chaotic():
    cut = []
    for i in ec.shared_lookback_cases():
        p, g, B, kernel = ec.lookback_case(i)
        where = ec.shadow_cut(p, ec.stream(p, g, B), EPISODES, STEPS)
        if where is not None:
            cut.append("case %d at episode %d step %d" % ((i,) + where))
    n = len(ec.shared_lookback_cases())     # (the private-theta half of the sweep is compared for equality: no shadow there)
    print("look-back sweep: %d of its %d shared-theta cases cut short by the shadow oracle %s" % (len(cut), n, cut))
    assert len(cut) <= n // 10, cut


def test_policy_sweep_is_not_chaotic():
    """The fast-kernel leg (one shared vector, 64 / 130 / 300 books; "pair" and "pair_env64" run the same case) and the shared-theta
    cases of the general leg."""
    cut_fast, cut_general, n_general = [], [], 0
    for i in range(ec.N_POLICY):
        p, g, B = ec.policy_case_fast(i, ec.fast_variants(i)[0])
        where = ec.shadow_cut(p, ec.stream(p, g, B), EPISODES, STEPS)
        if where is not None:
            cut_fast.append("case %d at episode %d step %d" % ((i,) + where))
        p, g, B = ec.policy_case(i)
        if p.theta_mode == abi.THETA_SHARED and B > 1:
            n_general += 1
            where = ec.shadow_cut(p, ec.stream(p, g, B), EPISODES, STEPS)
            if where is not None:
                cut_general.append("case %d at episode %d step %d" % ((i,) + where))
    print("policy sweep: fast kernels %d of %d cases cut short %s; general kernels %d of %d shared-theta cases %s" %
          (len(cut_fast), ec.N_POLICY, cut_fast, len(cut_general), n_general, cut_general))
    assert len(cut_fast) <= ec.N_POLICY // 10, cut_fast
    assert len(cut_general) <= n_general // 10, cut_general
    # ... and the one case that takes the fused action selection by its size, which the GPU test requires to run to its end
    p, rec = ec.policy_size_case()
    assert ec.shadow_cut(p, rec, EPISODES, STEPS) is None


@pytest.mark.parametrize("algo", ec.BIG_ALGOS)
@pytest.mark.parametrize("M", ec.BIG_TABLES)
def test_tables_around_the_pair_kernel_threshold_are_not_chaotic(M, algo):
    """The six cases of one GiB of weights: the GPU test compares all of it, so none of them may end early.  (From an all-zero
    vector four of the six did, at steps 7-9, with any stream tried: tests/edge_cases.py big_table_case.)"""
    p, rec = ec.big_table_case(M, algo)
    assert ec.shadow_cut(p, rec, 1, 40) is None


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_exchange_schedules_are_not_chaotic(name):
    """The oracle-compared cases of tests/test_gpu_exchange_edges.py (several shards exchanging their weights and rho, external updates,
    shards that end at different times): the GPU test runs every one of them to its end, so none may leave its shadow."""
    cut, periods = xc.shadow_cut(xc.CASES[name])
    assert cut is None, "%s: the shadow shards take another action at step %d" % (name, cut)
    if name.startswith("unequal-ends"):
        first_idle = [min(k for k, m in enumerate(periods) if not m[r]) for r in range(3)]
        assert max(first_idle) - min(first_idle) >= 3 and not any(periods[-1]), first_idle


def test_an_exchange_right_after_the_first_reset_is_not_chaotic():
    cut, _ = xc.shadow_cut(xc.case(abi.ALGO_QLAMBDA, 3, ops=[("x",), ("step", 16), ("x",), ("step", 4)]))
    assert cut is None


def test_policy_sweep_holds_every_algorithm_and_measure():
    algos, rewards, taus, mm_exp = set(), {}, set(), []
    for i in range(ec.N_POLICY):
        p, g, B = ec.policy_case(i)
        assert p.policy == abi.POLICY_BOLTZMANN and p.tau in ec.TAUS and p.beta in ec.BETAS
        algos.add(p.algo); taus.add(p.tau)
        rewards[p.reward_measure] = rewards.get(p.reward_measure, 0) + 1
        if p.reward_measure == abi.REWARD_MM_EXP:
            assert 0.0 <= p.pos_weight <= 0.2
            mm_exp.append(ec.fast_variants(i))
    assert algos == set(range(6)) and taus == set(ec.TAUS)
    assert set(rewards) == set(ec.ALL_REWARDS) and min(rewards.values()) >= 2, rewards
    # MM_EXP reaches both env-step forms of the fast kernels three times: its cases' algorithms go with "pair" and "pair_env64"
    assert len(mm_exp) >= 3 and all(v == ("pair", "pair_env64") for v in mm_exp), mm_exp


def test_eight_keys_fill_a_merged_trade_list_and_a_ninth_is_refused():
    D, T, B = 5, 8, 3
    rec, runs = ec.crafted_eight_keys(D=D, B=B)
    assert validate(rec, D, T) == 0
    bad, _ = ec.crafted_eight_keys(D=D, B=B, ninth=True)
    assert validate(bad, D, T) == abi.LOB_EDATA
    assert b"max_trades = 8" in abi.load().lob_last_error()
    # from the records: the rows behind each merging event's predecessor, up to its own first row, hold eight distinct keys
    f = rec.view(np.float32)
    otp, otv = 2 + 4 * D, 2 + 4 * D + T
    for b, first, _ in runs:
        firsts = np.flatnonzero(hs.event_firsts(rec[b], D))
        k = int(np.searchsorted(firsts, first))
        assert firsts[k] == first and firsts[k - 1] == first - 5, (b, first, firsts[k - 2:k + 1])
        rows = slice(firsts[k - 1] + 1, first + 1)
        live = rec[b, rows, otv:otv + T] > 0
        keys = np.rint(f[b, rows, otp:otp + T][live].astype(np.float64) * 10000.0).astype(np.int64)
        assert len(set(keys.tolist())) == 8 and live.sum() == 8, (b, first, keys)
    # the oracle consumes them: over the GPU test's schedule every book's cursor passes two of its three merging events
    p = engine.default_params()
    p.depth, p.max_trades, p.theta_mode, p.memory_size = D, T, abi.THETA_PRIVATE, 1 << 16
    o = ol.Oracle(p, rec)
    o.reset()
    o.td_step(70)
    cursor = o.recs()["book"]["cursor"]
    o.close()
    passed = [int(sum(cursor[b] > first for bb, first, _ in runs if bb == b)) for b in range(B)]
    assert min(passed) >= 2, (passed, cursor)


@pytest.mark.parametrize("D,T", [(D, T) for D in (1, 2, 4, 6, 7, 8, 9) for T in (1, 2)] + [(D, T) for D in (5, 7, 10) for T in (3, 5, 6, 7, 8)])
def test_harden_is_valid_at_the_edge_shapes(D, T):
    g = engine.default_gen_params()
    g.n_events = 200
    g.trade2_prob_q16 = 30000 if T > 1 else 0
    rec, counts = hs.harden(engine.gen_stream_host(g, D, T, 0, 16), D, T, hs.SEED + 100 * D + T, dry=True)
    assert validate(rec, D, T) == 0
    for k in hs.KINDS:
        assert counts[k] > 0, (D, T, k, counts)
    o = ol.Oracle(_params(D, T), rec)      # ... and the oracle plays them (the reference throws on a malformed stream)
    o.reset()
    o.td_step(60)
    assert o.counters()[0] > 0
    o.close()


def _params(D, T):
    p = engine.default_params()
    p.depth, p.max_trades, p.memory_size = D, T, 1 << 16
    return p
