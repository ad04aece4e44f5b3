"""lob_branch_book / lob_branch_history on the host side: the header as C99, LOB_ABI_VERSION, the exports against the header and the
ctypes mirror, the refusal of a NULL engine by each call, and the raw wrappers' independence of torch.  CPU only -- no compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")
PROTOS = ["int lob_branch_book(lob_engine* e, const lob_vec_book_out* out);",
          "int lob_branch_history(lob_engine* e, int32_t K, const lob_vec_hist_out* out);"]


def test_header_compiles_as_c99_and_the_structs_are_the_ones_reused(tmp_path):
    """The header with every warning an error, the two prototypes declared once more (a second declaration that differs from the
    header's in any type is an error in C); the two out-structs and lob_branch_out keep their sizes, the ABI its version."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lob_engine.h"\n' + "\n".join(PROTOS) + "\n"
                   'int main(void){printf("%zu %zu %zu %d %d\\n",sizeof(lob_vec_book_out),sizeof(lob_vec_hist_out),sizeof(lob_branch_out),'
                   'LOB_MAX_HISTORY,LOB_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert got == [24, 40, 32, 128, 6], "sizeof the three structs, LOB_MAX_HISTORY, LOB_ABI_VERSION"
    assert C.sizeof(abi.VecBookOut) == 24 and C.sizeof(abi.VecHistOut) == 40 and C.sizeof(abi.BranchOut) == 32
    assert abi.MAX_HISTORY == 128
    assert abi.load().lob_abi_version() == 6


def test_symbols_are_exported_declared_and_in_the_header():
    lib = abi.load()
    vp = C.c_void_p
    want = {"lob_branch_book": [vp, C.POINTER(abi.VecBookOut)], "lob_branch_history": [vp, C.c_int32, C.POINTER(abi.VecHistOut)]}
    for name, args in want.items():
        assert hasattr(lib, name) and name in lib._declared, name
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes == args, name
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for proto in PROTOS:
        pat = r"\s*".join(re.escape(tok) for tok in re.findall(r"\w+|[^\w\s]", proto))
        assert re.search(pat, src), proto
    assert re.search(r"#define\s+LOB_ABI_VERSION\s+6\b", src)


def test_null_engine_is_refused_by_each_call_with_its_name():
    lib = abi.load()
    book, hist = abi.VecBookOut(None, None, None), abi.VecHistOut(None, None, None, None, None)
    calls = {"lob_branch_book": lambda: lib.lob_branch_book(None, C.byref(book)),
             "lob_branch_history": lambda: lib.lob_branch_history(None, 1, C.byref(hist))}
    for name, call in calls.items():
        lib.lob_market_preset(b"HSBA.L", C.byref(abi.Market()))   # (a call that succeeds: the message below is this refusal's)
        assert call() == abi.LOB_EINVAL, name
        msg = lib.lob_last_error()
        assert msg and name.encode() in msg, (name, msg)


def test_engine_wrappers_exist_without_torch():
    code = ("import sys\nfrom rl_markets_amd import engine, abi\n"
            "assert all(callable(getattr(engine.Engine, n)) for n in ('branch_book', 'branch_history'))\n"
            "assert 'lob_branch_book' in abi.load()._declared and 'lob_branch_history' in abi.load()._declared\n"
            "assert 'torch' not in sys.modules, 'rl_markets_amd.engine imported torch'\nprint('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
