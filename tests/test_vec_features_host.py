"""The arithmetic of lob_vec_features' contract on the CPU: tests/host_env/feat_diff.cpp compiles the engine's DEVICE header
(rl_markets_amd/csrc/lob_tiles.h) as host code through tests/host_env/shim and holds tile_index(tile_base_m(...), term) over the
three tile groups -- the action-independent hash sum reduced on its own, then the action's term -- against the oracle's
oracle_tiles, which sums in 64 bits and reduces once: a few thousand random rows per setting, exact tile boundaries and their
neighbours, NaN, +-inf, +-1e30 and negative values, for V in {4, 8, 16} and M in {1, 65, 2^16, 2^27 + 1, 2^31 - 1}.  The GPU suite
(tests/test_gpu_vec_features.py) then compares what the kernel stores; this test needs no GPU."""
import os
import re
import subprocess

from tests import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_sum_plus_action_term_equals_oracle_tiles(tmp_path):
    ol.load()   # (builds the oracle library when it is not there yet)
    exe = str(tmp_path / "feat_diff")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "tests", "host_env", "shim"),
                           "-o", exe, os.path.join(ROOT, "tests", "host_env", "feat_diff.cpp"), "-ldl"])
    out = subprocess.run([exe, ol.ORACLE_SO, os.environ.get("LOB_FEAT_DIFF_ROWS", "3000")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "feat_diff OK" in out.stdout
    m = re.search(r"checked (\d+) indices, (\d+) NaN variables, (\d+) boundary rows", out.stdout)
    assert m and int(m.group(1)) > 15 * 3000 * 864 and int(m.group(2)) > 0 and int(m.group(3)) > 0, out.stdout
