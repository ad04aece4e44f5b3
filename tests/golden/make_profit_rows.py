"""Writes tests/golden/step_log/profit_rows_b0.npz: the rows the reference's OWN experiment::serial::Backtester handed to its profit_log
logger (Intraday::LogProfit, src/environment/intraday.cpp:438-451) for one backtest -- one training episode, GoGreedy, one
Backtester episode -- through oracle/_ref/ref_harness --profit_out, the way tests/test_oracle_ref_sweep.py
test_random_backtest_against_the_reference drives it.  The fixture holds data only: the engine parameters and the generator
parameters as the bytes of their C structs (include/lob_engine.h, ABI version 6), the number of training steps and the
12-column rows (episode, time, action, position, midprice, spread, quoted_ask, quoted_bid, ask_level, bid_level, pnl_step,
bandh_step).  tests/test_gpu_step_log.py replays the case on the engine.  (A directory of its own: tests/golden/*.npz are
make_golden.py's, and tests/test_oracle_golden.py holds that list to what that script writes.)

Needs the reference checkout at build time (oracle/_ref/ref_harness).  Run from the repository root:
    python tests/golden/make_profit_rows.py
The case: the first seed from 64000 on (test_oracle_ref_sweep.random_case) whose backtest logs at least 80 rows, trades, and
uses one of the three agents the step log's oracle test covers."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from rl_markets_amd import abi, engine  # noqa: E402
from tests import oracle_lib as ol  # noqa: E402
from tests.test_oracle_ref_sweep import random_case, ref_or_failed_init  # noqa: E402


def case(seed):
    p, g, algo, x = random_case(seed)
    x["backtest"] = 1
    x["clear_inventory"] = 1
    rec = engine.gen_stream_host(g, 5, p.max_trades, p.book_id_offset, 1)
    with tempfile.TemporaryDirectory() as td:
        x["profit_out"] = os.path.join(td, "profit.bin")
        out = ref_or_failed_init(p, rec, "seed %d" % seed, trades=p.max_trades, algo=algo, mem=p.memory_size, seed=p.seed,
                                 rng_stream=p.book_id_offset, eps=p.epsilon, extra=x)
        if out is None:
            return None
        traj, info, _ = out
        raw = open(x["profit_out"], "rb").read()
    n = int(np.frombuffer(raw[:8], dtype=np.int64)[0])
    rows = np.frombuffer(raw[8:8 + 96 * n], dtype=np.float64).reshape(n, 12).copy()
    return p, g, algo, len(traj), rows


def main():
    for seed in range(64000, 64400):
        c = case(seed)
        if c is None:
            continue
        p, g, algo, train_steps, rows = c
        if algo not in ("sarsa", "q_learn", "double_q_learn") or len(rows) < 80 or len(set(rows[:, 3])) < 3:
            continue
        path = os.path.join(ROOT, "tests", "golden", "step_log", "profit_rows_b0.npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, abi_version=np.int32(abi.load().lob_abi_version()), seed=np.int32(seed),
                            params=np.frombuffer(bytes(p), dtype=np.uint8), gen=np.frombuffer(bytes(g), dtype=np.uint8),
                            train_steps=np.int32(train_steps), rows=rows)
        print("seed %d (%s): %d training steps, %d rows -> %s (%d bytes)" % (seed, algo, train_steps, len(rows), path, os.path.getsize(path)))
        return 0
    print("no case found")
    return 1


if __name__ == "__main__":
    sys.exit(main())
