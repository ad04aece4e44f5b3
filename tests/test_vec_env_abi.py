"""lob_vec_* (include/lob_engine.h): the ABI mirror of lob_vec_out and the three entry points.  CPU only -- the interface itself is
tested on the GPU (tests/test_gpu_vec_env.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the header's order and offsets, written out: five device pointers
FIELDS = [("obs", 0), ("reward", 8), ("terminal", 16), ("stepped", 24), ("n_live", 32)]
SYMBOLS = ("lob_vec_step", "lob_vec_observe", "lob_vec_status")


def test_vec_out_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\nint main(){printf("%zu", sizeof(lob_vec_out));\n'
                   + "".join('printf(" %%zu", offsetof(lob_vec_out, %s));\n' % n for n, _ in FIELDS)
                   + 'printf(" %d\\n", LOB_ABI_VERSION);return 0;}')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[0] == 40 == C.sizeof(abi.VecOut)
    assert got[1:-1] == [off for _, off in FIELDS]
    assert got[-1] == 6, "additions only: the ABI version stays"
    assert [n for n, _ in abi.VecOut._fields_] == [n for n, _ in FIELDS]
    for name, off in FIELDS:
        assert getattr(abi.VecOut, name).offset == off, name
        assert C.sizeof(dict(abi.VecOut._fields_)[name]) == 8, name


def test_abi_version_stays():
    assert abi.load().lob_abi_version() == 6


def test_symbols_exported_and_declared():
    lib = abi.load()
    header = open(os.path.join(ROOT, "include", "lob_engine.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in lib._declared, name
        assert re.search(r"^int %s\(lob_engine\* e" % name, header, re.M), name
    assert re.search(r"typedef struct lob_vec_out \{", header)


def test_null_engine_is_einval_with_a_message():
    lib = abi.load()
    out = abi.VecOut()
    n = C.c_int64(-7)
    for call in (lambda: lib.lob_vec_step(None, None, C.byref(out)), lambda: lib.lob_vec_observe(None, C.byref(out)),
                 lambda: lib.lob_vec_status(None, C.byref(n))):
        assert call() == abi.LOB_EINVAL
        assert lib.lob_last_error()
    assert n.value == -7, "nothing is written for a NULL engine"


def test_engine_module_does_not_import_torch():
    code = ("import sys; import rl_markets_amd.engine as e, rl_markets_amd.abi as a; "
            "assert 'torch' not in sys.modules, 'rl_markets_amd.engine pulled torch in'; "
            "assert hasattr(e.Engine, 'vec_step') and hasattr(e.Engine, 'vec_observe') and hasattr(e.Engine, 'vec_status'); print('ok')")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr
