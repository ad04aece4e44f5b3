"""The day library's C ABI (lob_load_days, lob_days_select, lob_days_set, lob_get_days) and the sampler it restates.
CPU only: the symbols and constants against include/lob_engine.h, and tests/days_ref.py (what the GPU tests hold
days_draw_kernel to) against libstdc++'s own std::default_random_engine + std::uniform_int_distribution<size_t>."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rl_markets_amd import abi
from tests import days_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lob_engine.h")
DAY_FUNCS = ["lob_load_days", "lob_days_select", "lob_days_set", "lob_get_days"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_day_symbols_are_exported_and_declared():
    lib = abi.load()
    src = _header()
    for n in DAY_FUNCS:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), "liblob_engine.so does not export %s" % n
        assert n in lib._declared


def test_day_prototypes_match_header():
    src = _header()
    want = {
        "lob_load_days": ["lob_engine*", "const uint32_t*", "const int64_t*", "int32_t"],
        "lob_days_select": ["lob_engine*", "int32_t", "int32_t", "int32_t"],
        "lob_days_set": ["lob_engine*", "const int32_t*"],
        "lob_get_days": ["lob_engine*", "int32_t*"],
    }
    ctype = {"lob_engine*": C.c_void_p, "const uint32_t*": C.c_void_p, "const int64_t*": C.c_void_p,
             "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "int32_t": C.c_int32}
    lib = abi.load()
    for n, types in want.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        args = [re.sub(r"\s+\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]
        assert args == types, (n, args)
        fn = getattr(lib, n)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [ctype[t] for t in types], n


def test_day_mode_constants_match_header():
    src = _header()
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(LOB_DAYS_\w+)\s+(\d+)", src))
    assert consts == {"LOB_DAYS_RANDOM": abi.DAYS_RANDOM, "LOB_DAYS_IN_ORDER": abi.DAYS_IN_ORDER}
    assert abi.DAYS_RANDOM != abi.DAYS_IN_ORDER


SAMPLER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
int main(int argc, char** argv) {
    unsigned seed = (unsigned)strtoul(argv[1], 0, 10);
    size_t n = strtoul(argv[2], 0, 10), k = strtoul(argv[3], 0, 10);
    std::default_random_engine rng(seed);
    for (size_t i = 0; i < k; i++) printf("%zu\n", std::uniform_int_distribution<size_t>{0, n - 1}(rng));
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ (libstdc++)")
def test_sampler_restatement_equals_libstdcxx(tmp_path):
    src = tmp_path / "sampler.cpp"
    src.write_text(SAMPLER_CPP)
    exe = tmp_path / "sampler"
    subprocess.check_call(["g++", "-O1", "-std=c++17", str(src), "-o", str(exe)])
    # small and large libraries, a power of two, seeds 0 and 2^31 - 1 (both seed the engine's state with 1)
    for seed in (0, 1, 42, 2147483647, 4294967295, 123456789):
        for n in (1, 2, 3, 7, 20, 64, 1000, 1 << 20):
            out = subprocess.check_output([str(exe), str(seed), str(n), "10000"]).split()
            ref = [int(v) for v in out]
            x = days_ref.seed_state(seed)
            mine = []
            for _ in range(10000):
                x, v = days_ref.draw(x, n)
                mine.append(v)
            assert mine == ref, (seed, n)
    assert days_ref.book_days(40, 2, 20, 5) == days_ref.book_days(41, 1, 20, 5)   # seeded with seed + global id


def test_dry_padding_is_not_the_same_day():
    """Why the GPU tests of unequal days use one-book oracles (private theta) and no batched oracle over days padded to one
    length: a day padded with rows flagged LOB_EVT_FLAG_TAS_DRY plays exactly like the day itself until the day's data
    runs out, and the step at which it runs out is not the same -- past the day's last row the depth stream still has a
    row to load (Streamer::LoadNext succeeds) where the unpadded day ends.  CPU oracle only."""
    from rl_markets_amd import engine
    from tests import oracle_lib as ol
    p = engine.default_params()
    p.algo, p.theta_mode, p.memory_size = abi.ALGO_QLAMBDA, abi.THETA_PRIVATE, 1 << 16
    g = engine.default_gen_params()
    g.n_events = 300
    day = engine.gen_stream_host(g, 5, 2, 0, 1)
    pad = np.concatenate([day[0], np.repeat(day[0, -1:], 300, axis=0)])[None].copy()
    pad[0, 300:, 1] |= abi.EVT_FLAG_TAS_DRY
    o1, o2 = ol.Oracle(p, day), ol.Oracle(p, pad)
    o1.reset()
    o2.reset()
    parted = None
    for s in range(400):
        o1.td_step(1)
        o2.td_step(1)
        r1, r2 = o1.recs(), o2.recs()
        if r1.tobytes() != r2.tobytes():
            parted = s
            break
    assert parted is not None, "a dry-padded day played like the day itself: a batched oracle over padded days would do"
    assert r1["book"]["terminal"][0] == 2 or r2["book"]["terminal"][0] == 2, "they part where the day's data runs out"
