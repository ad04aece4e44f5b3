"""The oracle against the UNMODIFIED reference at the edges tests/test_gpu_edges.py holds the engine to: look-backs of 101 .. 256
events, tables of 1 .. 4 098 weights (and one of 2^27), with Boltzmann, every reward measure but `none`, beta and random_init as
tests/test_oracle_ref_sweep.py::random_case already draws them.  That file's case generator, wrapped and not edited; its
comparison, statement for statement: the reset state, every step of the trajectory, the final step count, the weights.  This
is what gives tests/oracle_lib its authority where the GPU file uses it as the yardstick (D = 5: the reference reads
five-level depth files only)."""
import os
import tempfile

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests import edge_cases as ec
from tests import oracle_lib as ol
from tests.test_oracle_golden import compare_traj
from tests.test_oracle_ref_sweep import check_sparse, off_grid, random_case, ref_or_failed_init, sparse

pytestmark = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref/ref_harness not built (needs the reference checkout)")

N_CASES = 24
TABLES = (1, 2, 31, 32, 33, 64, 4098)
PAST_INITIALISE = []     # the cases whose reference run got past Initialise


def edge_case(seed):
    p, g, algo, x = random_case(91000 + seed)
    r = np.random.default_rng(91500 + seed)
    for name in ec.LOOKBACKS:
        if r.integers(0, 2):
            w = int(r.choice(ec.LB_EDGES))
            setattr(p, name, w)
            x[name] = w
    p.memory_size = x["mem"] = int(TABLES[seed % len(TABLES)])
    g.n_events = 1200       # Initialise fills a window of 256 and steps follow
    return p, g, algo, x


def against_the_reference(p, g, algo, x, seed, tag):
    """-> True when the reference got past Initialise and the trajectories were compared."""
    rec = engine.gen_stream_host(g, 5, p.max_trades, p.book_id_offset, 1)
    if seed % 3 == 2:
        rec = off_grid(rec, p.max_trades, seed)
    with tempfile.TemporaryDirectory() as td:
        tb = os.path.join(td, "theta_b.bin")
        if "double" in algo:
            x["theta_b_out"] = tb
        if seed % 8 == 5:
            # learning.random_init: the reference's own constructors fill the (tiny) vectors, one agent per book
            x["random_init"] = 1
            p.random_init = 1
            p.theta_mode = abi.THETA_PRIVATE
        out = ref_or_failed_init(p, rec, tag, trades=p.max_trades, algo=algo, mem=p.memory_size, seed=p.seed,
                                 rng_stream=p.book_id_offset, eps=p.epsilon, extra=x)
        if out is None:
            return False
        traj, info, theta = out
        theta_b = sparse(tb) if "double" in algo else None
    o = ol.Oracle(p, rec)
    o.reset()
    r0 = o.rec(0)
    for n in r0["book"].dtype.names:
        if n != "cursor":
            assert np.array_equal(r0["book"][n], traj[0]["book"][n]), "%s reset book.%s" % (tag, n)
    np.testing.assert_array_equal(r0["vars"], traj[0]["vars"], err_msg=tag)
    compare_traj(lambda: o.td_step(1), lambda: o.rec(0), traj, tag)
    o.td_step(1)    # the reference ended on out-of-data / the close
    assert o.counters()[0] == int(info["steps"]), tag
    check_sparse(o.theta(0), theta[0], theta[1], tag)
    if theta_b is not None:
        check_sparse(o.theta_b(0), theta_b[0], theta_b[1], tag + " theta_b")
    o.close()
    return True


@pytest.mark.parametrize("seed", range(N_CASES))
def test_edge_configuration_against_the_reference(seed):
    p, g, algo, x = edge_case(seed)
    tag = "edge seed %d (%s, %s, M = %d, look-backs %s)" % (seed, algo, x["reward"], p.memory_size, [getattr(p, n) for n in ec.LOOKBACKS])
    if against_the_reference(p, g, algo, x, seed, tag):
        PAST_INITIALISE.append(seed)


def test_a_table_of_2_to_the_27_against_the_reference():
    """The size from which the engine's learn kernel changes (plan_paths): one GiB of weights in the reference harness and in the
    oracle, the weights compared through the harness's sparse dump."""
    p, g, algo, x = edge_case(3)
    p.memory_size = x["mem"] = 1 << 27
    g.n_events = 400
    for name in ec.LOOKBACKS:
        w = min(getattr(p, name), 100)
        setattr(p, name, w)
        x[name] = w
    assert against_the_reference(p, g, algo, x, 3, "M = 2^27 (%s, %s)" % (algo, x["reward"])), "a condition on the case: Initialise succeeds"


def test_zz_most_edge_cases_get_past_initialise():
    """(after the sweep: file order)  A case whose stream ends before the windows are full only checks that both sides refuse it."""
    if os.environ.get("PYTEST_XDIST_WORKER"):
        pytest.skip("under pytest-xdist this process has seen only its share of the sweep")
    print("edge cases past Initialise: %d of %d %s" % (len(PAST_INITIALISE), N_CASES, PAST_INITIALISE))
    assert len(PAST_INITIALISE) >= 16, PAST_INITIALISE
