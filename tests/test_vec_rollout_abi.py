"""lob_vec_rollout on the host side: the header as C99, the struct and the two limits against the ctypes mirror, the export, the
refusal of a NULL engine, and the raw wrapper's independence of torch.  CPU only -- no compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")
FIELDS = ["obs", "reward", "terminal", "stepped", "ret"]


def probe(tmp_path):
    """The header compiled as C99 with every warning an error, the prototype declared once more (a second declaration that differs
    from the header's in any type is an error in C)."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\n'
                   'int lob_vec_rollout(lob_engine* e, const int32_t* dev_actions, int n_plans, int horizon, double gamma, const lob_vec_rollout_out* out);\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n",sizeof(lob_vec_rollout_out),offsetof(lob_vec_rollout_out,obs),'
                   'offsetof(lob_vec_rollout_out,reward),offsetof(lob_vec_rollout_out,terminal),offsetof(lob_vec_rollout_out,stepped),'
                   'offsetof(lob_vec_rollout_out,ret),LOB_MAX_ROLLOUT_PLANS,LOB_MAX_ROLLOUT_STEPS,LOB_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return list(map(int, subprocess.check_output([str(exe)]).split()))


def test_header_compiles_as_c99_and_matches_the_ctypes_mirror(tmp_path):
    got = probe(tmp_path)
    assert got == [40, 0, 8, 16, 24, 32, 64, 64, 6], "sizeof, the five offsets, the two limits, LOB_ABI_VERSION"
    V = abi.VecRolloutOut
    assert C.sizeof(V) == 40 and [getattr(V, f).offset for f in FIELDS] == [0, 8, 16, 24, 32]
    assert [f[0] for f in V._fields_] == FIELDS and all(f[1] is C.c_void_p for f in V._fields_)
    assert abi.MAX_ROLLOUT_PLANS == 64 and abi.MAX_ROLLOUT_STEPS == 64
    assert abi.load().lob_abi_version() == 6


def test_symbol_is_exported_declared_and_in_the_header():
    lib = abi.load()
    assert hasattr(lib, "lob_vec_rollout") and "lob_vec_rollout" in lib._declared
    assert lib.lob_vec_rollout.restype is C.c_int
    assert lib.lob_vec_rollout.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(abi.VecRolloutOut)]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+lob_vec_rollout\s*\(\s*lob_engine\s*\*\s*e\s*,\s*const\s+int32_t\s*\*\s*dev_actions\s*,\s*int\s+n_plans\s*,\s*int\s+horizon\s*,"
                     r"\s*double\s+gamma\s*,\s*const\s+lob_vec_rollout_out\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"#define\s+LOB_MAX_ROLLOUT_PLANS\s+64\b", src) and re.search(r"#define\s+LOB_MAX_ROLLOUT_STEPS\s+64\b", src)


def test_null_engine_is_refused_with_a_message():
    lib = abi.load()
    out = abi.VecRolloutOut(None, None, None, None, None)
    lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))   # (a call that succeeds: the message below is this refusal's)
    assert lib.lob_vec_rollout(None, None, 1, 1, 1.0, C.byref(out)) == abi.LOB_EINVAL
    msg = lib.lob_last_error()
    assert msg and b"lob_vec_rollout" in msg


def test_engine_wrapper_exists_without_torch():
    code = ("import sys\nfrom rl_markets_amd import engine, abi\nassert callable(engine.Engine.vec_rollout)\n"
            "assert abi.VecRolloutOut is not None and abi.MAX_ROLLOUT_PLANS == 64 and abi.MAX_ROLLOUT_STEPS == 64\n"
            "assert 'torch' not in sys.modules, 'rl_markets_amd.engine imported torch'\nprint('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
