"""The C ABI of the look-aheads on a ring-mode stream (include/lob_engine.h lob_look_ring, lob_track_window, lob_look_counts): the
symbols, the constants, the NULL checks that need no device, and the header's statement of the window rule against the constants the
kernels are compiled with.  CPU only."""
import os
import re

from rl_markets_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "lob_engine.h")).read()
CSRC = os.path.join(ROOT, "rl_markets_amd", "csrc")


def define(text, name):
    m = re.search(r"^#define\s+%s\s+(\S+)" % name, text, re.M)
    assert m, name
    return m.group(1)


def test_symbols_and_constants():
    lib = abi.load()
    for n in ("lob_look_ring", "lob_track_window", "lob_look_counts"):
        assert hasattr(lib, n) and n in lib._declared and re.search(r"^int %s\s*\(" % n, HEADER, re.M), n
    assert int(define(HEADER, "LOB_TERMINAL_AHEAD")) == abi.TERMINAL_AHEAD == 3
    assert int(define(HEADER, "LOB_TERMINAL_BEHIND")) == abi.TERMINAL_BEHIND == 4
    assert int(define(HEADER, "LOB_TRACK_WINDOW_MARGIN")) == abi.TRACK_WINDOW_MARGIN
    # the two codes continue lob_get_terminal's 0 / 1 / 2 and fit the uint8 planes
    assert {abi.TERMINAL_AHEAD, abi.TERMINAL_BEHIND}.isdisjoint({0, 1, 2}) and abi.TERMINAL_BEHIND < 256


def test_null_arguments():
    lib = abi.load()
    assert lib.lob_look_ring(None, 1) == abi.LOB_EINVAL and b"lob_look_ring" in lib.lob_last_error()
    assert lib.lob_track_window(None, None, None, None) == abi.LOB_EINVAL and b"lob_track_window" in lib.lob_last_error()
    assert lib.lob_look_counts(None, None, None) == abi.LOB_EINVAL and b"lob_look_counts" in lib.lob_last_error()


def test_the_header_states_the_margin_of_the_pre_pass():
    """lo = max(0, n_track - ring length + margin), the margin being the one prepass_extend_kernel grants the real cursor."""
    kernels = open(os.path.join(CSRC, "lob_kernels.h")).read()
    margin = int(define(kernels, "LOB_TRACK_MARGIN"))
    assert margin == abi.TRACK_WINDOW_MARGIN
    assert "k_stop = S.k[b] + S.track_len - LOB_TRACK_MARGIN" in kernels
    flat = re.sub(r"\s*\n \*\s*", " ", HEADER)
    assert "lo = max(0, n_track - ring length + LOB_TRACK_WINDOW_MARGIN)" in flat
    assert "a private state at cursor k can be served while lo <= k; a private step is served when it never needs an entry >= hi while complete == 0" in flat
    assert "LOB_TRACK_WINDOW_MARGIN (%d)" % margin in flat
    # ... and the kernels' window is that very expression
    peek = open(os.path.join(CSRC, "lob_peek.h")).read()
    assert "lo = hi - S.track_len + LOB_TRACK_MARGIN" in peek
    assert "static_assert(LOB_TRACK_WINDOW_MARGIN == LOB_TRACK_MARGIN" in open(os.path.join(CSRC, "lob_tu_host_vec.hip")).read()
