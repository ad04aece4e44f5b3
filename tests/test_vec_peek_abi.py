"""lob_vec_peek on the host side: the header as C99, the struct and the mask constant against the ctypes mirror, the export, the
refusal of a NULL engine, and the raw wrapper's independence of torch.  CPU only -- no compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")


def probe(tmp_path):
    """The header compiled as C99 with every warning an error, the prototype declared once more (a second declaration that differs
    from the header's in any type is an error in C)."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\n'
                   'int lob_vec_peek(lob_engine* e, uint32_t action_mask, const lob_vec_peek_out* out);\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %u %d %d\\n",sizeof(lob_vec_peek_out),offsetof(lob_vec_peek_out,obs),'
                   'offsetof(lob_vec_peek_out,reward),offsetof(lob_vec_peek_out,terminal),offsetof(lob_vec_peek_out,stepped),'
                   'LOB_PEEK_ALL,LOB_ABI_VERSION,LOB_N_ACTIONS);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return list(map(int, subprocess.check_output([str(exe)]).split()))


def test_header_compiles_as_c99_and_matches_the_ctypes_mirror(tmp_path):
    got = probe(tmp_path)
    assert got == [32, 0, 8, 16, 24, 0x1FF, 6, 9], "sizeof, the four offsets, LOB_PEEK_ALL, LOB_ABI_VERSION, LOB_N_ACTIONS"
    V = abi.VecPeekOut
    assert C.sizeof(V) == 32 and (V.obs.offset, V.reward.offset, V.terminal.offset, V.stepped.offset) == (0, 8, 16, 24)
    assert [f[0] for f in V._fields_] == ["obs", "reward", "terminal", "stepped"] and all(f[1] is C.c_void_p for f in V._fields_)
    assert abi.PEEK_ALL == 0x1FF == (1 << abi.LOB_N_ACTIONS) - 1
    assert abi.load().lob_abi_version() == 6 and abi.LOB_N_ACTIONS == 9


def test_symbol_is_exported_declared_and_in_the_header():
    lib = abi.load()
    assert hasattr(lib, "lob_vec_peek") and "lob_vec_peek" in lib._declared
    assert lib.lob_vec_peek.restype is C.c_int
    assert lib.lob_vec_peek.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(abi.VecPeekOut)]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+lob_vec_peek\s*\(\s*lob_engine\s*\*\s*e\s*,\s*uint32_t\s+action_mask\s*,\s*const\s+lob_vec_peek_out\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"#define\s+LOB_PEEK_ALL\s+0x1FFu\b", src)


def test_null_engine_is_refused_with_a_message():
    lib = abi.load()
    out = abi.VecPeekOut(None, None, None, None)
    lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))   # (a call that succeeds: the message below is this refusal's)
    assert lib.lob_vec_peek(None, abi.PEEK_ALL, C.byref(out)) == abi.LOB_EINVAL
    msg = lib.lob_last_error()
    assert msg and b"lob_vec_peek" in msg


def test_engine_wrapper_exists_without_torch():
    code = ("import sys\nfrom rl_markets_amd import engine, abi\nassert callable(engine.Engine.vec_peek)\n"
            "assert abi.VecPeekOut is not None and abi.PEEK_ALL == 511\nassert 'torch' not in sys.modules, 'rl_markets_amd.engine imported torch'\nprint('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
