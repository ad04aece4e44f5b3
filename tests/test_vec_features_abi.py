"""lob_vec_terms / lob_vec_features / lob_vec_update on the host side: the header as C99, the struct and LOB_N_TILES against the ctypes
mirror, the exports, the refusal of a NULL engine, and the raw wrappers' independence of torch.  CPU only -- no compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")


def probe(tmp_path):
    """The header compiled as C99 with every warning an error, the three prototypes declared once more (a second declaration that
    differs from the header's in any type is an error in C)."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\n'
                   'int lob_vec_terms(lob_engine* e, int32_t host_out[27]);\n'
                   'int lob_vec_features(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const lob_vec_feat_out* out);\n'
                   'int lob_vec_update(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const double* dev_step, int32_t second);\n'
                   'int main(void){printf("%zu %zu %zu %d %d %d\\n",sizeof(lob_vec_feat_out),offsetof(lob_vec_feat_out,sums),'
                   'offsetof(lob_vec_feat_out,idx),LOB_N_TILES,LOB_ABI_VERSION,LOB_N_ACTIONS);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return list(map(int, subprocess.check_output([str(exe)]).split()))


def test_header_compiles_as_c99_and_matches_the_ctypes_mirror(tmp_path):
    got = probe(tmp_path)
    assert got == [16, 0, 8, 96, 6, 9], "sizeof, the two offsets, LOB_N_TILES, LOB_ABI_VERSION, LOB_N_ACTIONS"
    V = abi.VecFeatOut
    assert C.sizeof(V) == 16 and (V.sums.offset, V.idx.offset) == (0, 8)
    assert [f[0] for f in V._fields_] == ["sums", "idx"] and all(f[1] is C.c_void_p for f in V._fields_)
    assert abi.N_TILES == 96
    assert abi.load().lob_abi_version() == 6 and abi.LOB_N_ACTIONS == 9


def test_symbols_are_exported_declared_and_in_the_header():
    lib = abi.load()
    for name in ("lob_vec_terms", "lob_vec_features", "lob_vec_update"):
        assert hasattr(lib, name) and name in lib._declared
        assert getattr(lib, name).restype is C.c_int
    assert lib.lob_vec_terms.argtypes == [C.c_void_p, C.POINTER(C.c_int32)]
    assert lib.lob_vec_features.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(abi.VecFeatOut)]
    assert lib.lob_vec_update.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ws = lambda s: re.sub(r"\s+", " ", s)
    flat = ws(src)
    assert "int lob_vec_terms(lob_engine* e, int32_t host_out[27]);" in flat
    assert "int lob_vec_features(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const lob_vec_feat_out* out);" in flat
    assert "int lob_vec_update(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const double* dev_step, int32_t second);" in flat


def test_null_engine_is_refused_with_a_message():
    lib = abi.load()
    out = abi.VecFeatOut(None, None)
    buf = (C.c_int32 * 27)()
    calls = {"lob_vec_terms": lambda: lib.lob_vec_terms(None, buf),
             "lob_vec_features": lambda: lib.lob_vec_features(None, None, 1, None, C.byref(out)),
             "lob_vec_update": lambda: lib.lob_vec_update(None, None, 1, None, None, 0)}
    for name, call in calls.items():
        lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))   # (a call that succeeds: the message below is this refusal's)
        assert call() == abi.LOB_EINVAL, name
        msg = lib.lob_last_error()
        assert msg and name.encode() in msg, (name, msg)


def test_engine_wrappers_exist_without_torch():
    code = ("import sys\nfrom rl_markets_amd import engine, abi\n"
            "assert callable(engine.Engine.vec_terms) and callable(engine.Engine.vec_features) and callable(engine.Engine.vec_update)\n"
            "assert abi.VecFeatOut is not None and abi.N_TILES == 96\nassert 'torch' not in sys.modules, 'rl_markets_amd.engine imported torch'\nprint('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
