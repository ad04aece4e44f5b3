"""lob_vec_book on the host side: the header's struct and constants against the ctypes mirror, the export, the refusal of a NULL
engine, and the raw wrapper's independence of torch.  CPU only -- no compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")
OWN_NAMES = ("POSITION", "ASK_HAS_ORDER", "ASK_ORDER_PX", "ASK_ORDER_REM", "ASK_Q_HEAD", "BID_HAS_ORDER", "BID_ORDER_PX", "BID_ORDER_REM",
             "BID_Q_HEAD", "ASK_QUOTE", "BID_QUOTE", "LAST_ACTION", "PNL_STEP", "EPISODE_PNL", "EPISODE_REWARD", "TOTAL_TICKS")


def probe(tmp_path):
    src = tmp_path / "probe.c"
    own = "".join(',LOB_OWN_%s' % n for n in OWN_NAMES)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\n'
                   'int main(){int own[]={0%s};int i;'
                   'printf("%%zu %%zu %%zu %%zu %%d %%d",sizeof(lob_vec_book_out),offsetof(lob_vec_book_out,levels),'
                   'offsetof(lob_vec_book_out,own),offsetof(lob_vec_book_out,time_ms),LOB_VEC_OWN_WORDS,LOB_ABI_VERSION);'
                   'for(i=1;i<=16;i++)printf(" %%d",own[i]);printf("\\n");return 0;}' % own)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return list(map(int, subprocess.check_output([str(exe)]).split()))


def test_header_layout_and_its_ctypes_mirror(tmp_path):
    got = probe(tmp_path)
    assert got[:6] == [24, 0, 8, 16, 16, 6], "sizeof, the three offsets, LOB_VEC_OWN_WORDS, LOB_ABI_VERSION"
    assert got[6:] == list(range(16)), "LOB_OWN_* name the sixteen words in the documented order"
    V = abi.VecBookOut
    assert C.sizeof(V) == got[0] and (V.levels.offset, V.own.offset, V.time_ms.offset) == tuple(got[1:4])
    assert [f[0] for f in V._fields_] == ["levels", "own", "time_ms"] and all(f[1] is C.c_void_p for f in V._fields_)
    assert abi.VEC_OWN_WORDS == got[4] and abi.load().lob_abi_version() == got[5]
    assert [getattr(abi, "OWN_" + n) for n in OWN_NAMES] == got[6:]
    dump_fields = {f[0] for f in abi.BookDump._fields_}
    assert len(abi.OWN_FIELDS) == 16 and set(abi.OWN_FIELDS) <= dump_fields
    assert [f.upper() for f in abi.OWN_FIELDS] == list(OWN_NAMES), "word k of own is the dump field of the same name"


def test_symbol_is_exported_declared_and_in_the_header():
    lib = abi.load()
    assert hasattr(lib, "lob_vec_book") and "lob_vec_book" in lib._declared
    assert lib.lob_vec_book.argtypes[1] is C.POINTER(abi.VecBookOut) and lib.lob_vec_book.restype is C.c_int
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+lob_vec_book\s*\(\s*lob_engine\s*\*\s*e\s*,\s*const\s+lob_vec_book_out\s*\*\s*out\s*\)\s*;", src)


def test_null_engine_is_refused_with_a_message():
    lib = abi.load()
    lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))   # (a call that succeeds: the message below is this refusal's)
    out = abi.VecBookOut(None, None, None)
    assert lib.lob_vec_book(None, C.byref(out)) == abi.LOB_EINVAL
    msg = lib.lob_last_error()
    assert msg and b"lob_vec_book" in msg


def test_engine_wrapper_exists_without_torch():
    code = ("import sys\nfrom rl_markets_amd import engine, abi\nassert callable(engine.Engine.vec_book)\n"
            "assert abi.VecBookOut is not None\nassert 'torch' not in sys.modules, 'rl_markets_amd.engine imported torch'\nprint('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
