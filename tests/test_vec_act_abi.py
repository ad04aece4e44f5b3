"""lob_vec_act / lob_vec_q on the host side: the header as C99, the struct and the mode constants against the ctypes mirror, the
exports, the refusal of a NULL engine, and the raw wrappers' independence of torch.  CPU only -- no compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")


def probe(tmp_path):
    """The header compiled as C99 with every warning an error, the two prototypes declared once more (a second declaration that
    differs from the header's in any type is an error in C)."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\n'
                   'int lob_vec_act(lob_engine* e, int32_t mode, const lob_vec_act_out* out);\n'
                   'int lob_vec_q(lob_engine* e, const float* dev_vars, int32_t n, double* dev_q);\n'
                   'int main(void){printf("%zu %zu %zu %d %d %d %d %d\\n",sizeof(lob_vec_act_out),offsetof(lob_vec_act_out,action),'
                   'offsetof(lob_vec_act_out,q),LOB_ACT_GREEDY,LOB_ACT_BEHAVIOUR,LOB_ACT_ARGMAX,LOB_ABI_VERSION,LOB_N_ACTIONS);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return list(map(int, subprocess.check_output([str(exe)]).split()))


def test_header_compiles_as_c99_and_matches_the_ctypes_mirror(tmp_path):
    got = probe(tmp_path)
    assert got == [16, 0, 8, 0, 1, 2, 6, 9], "sizeof, the two offsets, the three modes, LOB_ABI_VERSION, LOB_N_ACTIONS"
    V = abi.VecActOut
    assert C.sizeof(V) == 16 and (V.action.offset, V.q.offset) == (0, 8)
    assert [f[0] for f in V._fields_] == ["action", "q"] and all(f[1] is C.c_void_p for f in V._fields_)
    assert (abi.ACT_GREEDY, abi.ACT_BEHAVIOUR, abi.ACT_ARGMAX) == (0, 1, 2)
    assert abi.load().lob_abi_version() == 6 and abi.LOB_N_ACTIONS == 9


def test_symbols_are_exported_declared_and_in_the_header():
    lib = abi.load()
    for name in ("lob_vec_act", "lob_vec_q"):
        assert hasattr(lib, name) and name in lib._declared
        assert getattr(lib, name).restype is C.c_int
    assert lib.lob_vec_act.argtypes == [C.c_void_p, C.c_int32, C.POINTER(abi.VecActOut)]
    assert lib.lob_vec_q.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+lob_vec_act\s*\(\s*lob_engine\s*\*\s*e\s*,\s*int32_t\s+mode\s*,\s*const\s+lob_vec_act_out\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"\bint\s+lob_vec_q\s*\(\s*lob_engine\s*\*\s*e\s*,\s*const\s+float\s*\*\s*dev_vars\s*,\s*int32_t\s+n\s*,\s*double\s*\*\s*dev_q\s*\)\s*;", src)


def test_null_engine_is_refused_with_a_message():
    lib = abi.load()
    out = abi.VecActOut(None, None)
    lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))   # (a call that succeeds: the message below is this refusal's)
    assert lib.lob_vec_act(None, abi.ACT_GREEDY, C.byref(out)) == abi.LOB_EINVAL
    msg = lib.lob_last_error()
    assert msg and b"lob_vec_act" in msg
    lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))
    assert lib.lob_vec_q(None, None, 1, None) == abi.LOB_EINVAL
    msg = lib.lob_last_error()
    assert msg and b"lob_vec_q" in msg


def test_engine_wrappers_exist_without_torch():
    code = ("import sys\nfrom rl_markets_amd import engine, abi\nassert callable(engine.Engine.vec_act) and callable(engine.Engine.vec_q)\n"
            "assert abi.VecActOut is not None\nassert 'torch' not in sys.modules, 'rl_markets_amd.engine imported torch'\nprint('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
