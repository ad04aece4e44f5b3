"""The index arithmetic of the per-sum action masks (theta_nzm, rl_markets_amd/csrc/lob_tiles.h) on the CPU.

tests/host_env/fold_mask.cpp compiles the engine's device header as host code (tests/host_env/shim) and checks, for table sizes
61, 4 099, 65 536 and 20 000 000 and random action terms below them: the hash sum the mark computes for a weight f and a term t
satisfies (s + t) mod M == f (every f of the small tables, a seeded sample of the large ones, f < t -- the wrap-around -- and the
edges included), and a mask written through its word and shift is the 16-bit mask the kernel reads at [s], for even and odd s
and the last s of a table of odd length.  The GPU suite (test_gpu_fold_masks.py) then checks the tables the kernels keep."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_sum_and_mask_position(tmp_path):
    exe = str(tmp_path / "fold_mask")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "tests", "host_env", "shim"),
                           "-o", exe, os.path.join(ROOT, "tests", "host_env", "fold_mask.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "fold_mask OK" in out.stdout
