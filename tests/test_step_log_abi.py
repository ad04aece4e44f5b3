"""lob_step_log_* (include/lob_engine.h): the ABI mirrors of lob_step_row.  CPU only -- the log itself is tested on the GPU
(tests/test_gpu_step_log.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from rl_markets_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the header's order and offsets, written out: 2 x int64, 8 x double, 4 x int32
FIELDS = [("time_ms", 0), ("position", 8), ("midprice", 16), ("spread", 24), ("ask_quote", 32), ("bid_quote", 40), ("pnl_step", 48),
          ("episode_pnl", 56), ("episode_bandh", 64), ("episode_reward", 72), ("step", 80), ("action", 84), ("ask_level", 88),
          ("bid_level", 92)]


def test_row_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\nint main(){printf("%zu", sizeof(lob_step_row));\n'
                   + "".join('printf(" %%zu", offsetof(lob_step_row, %s));\n' % n for n, _ in FIELDS)
                   + 'printf(" %d\\n", LOB_ABI_VERSION);return 0;}')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[0] == 96 == C.sizeof(abi.StepRow) == engine.STEP_ROW_DTYPE.itemsize
    assert got[1:-1] == [off for _, off in FIELDS]
    assert got[-1] == 6, "additions only: the ABI version stays"
    assert [n for n, _ in abi.StepRow._fields_] == [n for n, _ in FIELDS] == list(engine.STEP_ROW_DTYPE.names)
    for name, off in FIELDS:
        assert getattr(abi.StepRow, name).offset == off == engine.STEP_ROW_DTYPE.fields[name][1], name
        ct = dict(abi.StepRow._fields_)[name]
        assert np.dtype(ct) == engine.STEP_ROW_DTYPE.fields[name][0], name
    assert len(FIELDS) == 14


def test_symbols_and_null_engine():
    lib = abi.load()
    for name in ("lob_step_log_enable", "lob_step_log_counts", "lob_step_log_read"):
        assert hasattr(lib, name), name
    books = np.zeros(1, np.int32)
    n = np.zeros(1, np.int32)
    rows = np.zeros(1, dtype=engine.STEP_ROW_DTYPE)
    vp = C.c_void_p
    assert lib.lob_step_log_enable(None, books.ctypes.data_as(vp), 1, 16) == abi.LOB_EINVAL
    assert lib.lob_last_error()
    assert lib.lob_step_log_counts(None, n.ctypes.data_as(vp), None) == abi.LOB_EINVAL
    assert lib.lob_step_log_read(None, 0, 1, 0, 1, rows.ctypes.data_as(vp)) == abi.LOB_EINVAL
