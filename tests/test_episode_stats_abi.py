"""lob_episode_stats / lob_episode_stats_merge (include/lob_engine.h): the ABI mirrors and the host-side merge.  CPU only --
the merge needs no device; the reduction itself is tested on the GPU (tests/test_gpu_episode_stats.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from rl_markets_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
EPS = 2.0 ** -53


def identity(group=-1):
    r = np.zeros((), dtype=engine.EPISODE_STATS_DTYPE)
    r["group"] = group
    r["f"]["min"], r["f"]["max"] = np.inf, -np.inf
    r["i"]["min"], r["i"]["max"] = I64_MAX, I64_MIN
    r["f"]["argmin"] = r["f"]["argmax"] = r["i"]["argmin"] = r["i"]["argmax"] = -1
    return r


def single(book_id, fvals, ivals, group=-1, terminal=1):
    """The record of one book: what the reduction makes of a book with these four f64 and four integer values."""
    r = identity(group)
    r["n_books"] = 1
    r[("n_live", "n_terminal", "n_out_of_data")[terminal]] = 1
    r["n_rho"] = 1
    for k in range(4):
        for name, v in (("f", float(fvals[k])), ("i", int(ivals[k]))):
            s = r[name][k]
            s["sum"], s["sumsq"], s["min"], s["max"], s["argmin"], s["argmax"] = v, v * v, v, v, book_id, book_id
    return r


def test_struct_sizes_match_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "lob_engine.h"\nint main(){printf("%zu %zu %zu\\n",'
                   'sizeof(lob_stat_f64),sizeof(lob_stat_i64),sizeof(lob_episode_record));return 0;}')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    sizes = list(map(int, subprocess.check_output([exe]).split()))
    assert sizes == [C.sizeof(abi.StatF64), C.sizeof(abi.StatI64), C.sizeof(abi.EpisodeStats)]
    assert engine.EPISODE_STATS_DTYPE.itemsize == sizes[2] == 408
    # field by field: the numpy dtype the Engine returns lies over the ctypes mirror
    for name in ("group", "n_books", "n_live", "n_terminal", "n_out_of_data", "n_rho", "f", "i"):
        assert engine.EPISODE_STATS_DTYPE.fields[name][1] == getattr(abi.EpisodeStats, name).offset, name
    assert (abi.STATF_REWARD, abi.STATF_RHO, abi.STATF_PNL, abi.STATF_BANDH) == (0, 1, 2, 3)
    assert (abi.STATI_STEPS, abi.STATI_TRANSACTIONS, abi.STATI_MARKET_ORDERS, abi.STATI_TICKS_POSITION) == (0, 1, 2, 3)


def test_symbols_and_null_engine():
    lib = abi.load()
    assert hasattr(lib, "lob_episode_stats") and hasattr(lib, "lob_episode_stats_merge")
    out = np.zeros(1, dtype=engine.EPISODE_STATS_DTYPE)
    n = C.c_int32(0)
    assert lib.lob_episode_stats(None, 0, out.ctypes.data_as(C.c_void_p), 1, C.byref(n)) == abi.LOB_EINVAL
    assert lib.lob_last_error()


def test_merge_identity():
    e = identity()
    a = single(7, [1.5, -2.0, 0.25, 3.0], [10, 4, 1, 6], group=-1)
    for m in (engine.merge_episode_stats(a, e), engine.merge_episode_stats(e, a)):
        assert m.tobytes() == a.tobytes()
    ee = engine.merge_episode_stats(e, e)
    assert ee.tobytes() == e.tobytes()
    assert ee["n_books"] == 0 and (ee["f"]["sum"] == 0).all() and (ee["i"]["sum"] == 0).all()
    assert (ee["f"]["min"] == np.inf).all() and (ee["f"]["max"] == -np.inf).all()
    assert (ee["i"]["min"] == I64_MAX).all() and (ee["i"]["max"] == I64_MIN).all()
    assert (ee["f"]["argmin"] == -1).all() and (ee["i"]["argmax"] == -1).all()
    # the inputs are not touched
    assert a.tobytes() == single(7, [1.5, -2.0, 0.25, 3.0], [10, 4, 1, 6]).tobytes()


def test_merge_group_kept_or_dropped():
    a, b = single(1, [0] * 4, [0] * 4, group=3), single(2, [0] * 4, [0] * 4, group=3)
    assert engine.merge_episode_stats(a, b)["group"] == 3
    b["group"] = 4
    assert engine.merge_episode_stats(a, b)["group"] == -1
    assert engine.merge_episode_stats(a, identity(-1))["group"] == -1
    assert engine.merge_episode_stats(a, identity(3))["group"] == 3


def test_merge_exact_fields_and_ties():
    a = single(12, [1.0, 5.0, -3.0, 2.0], [7, 9, 0, 3], terminal=1)
    b = single(5, [1.0, 6.0, -4.0, 2.0], [7, 8, 0, 5], terminal=2)
    c = single(30, [0.5, 6.0, -3.0, 9.0], [2, 9, 0, 5], terminal=0)
    m = engine.merge_episode_stats(engine.merge_episode_stats(a, b), c)
    assert (m["n_books"], m["n_live"], m["n_terminal"], m["n_out_of_data"], m["n_rho"]) == (3, 1, 1, 1, 3)
    f, i = m["f"], m["i"]
    assert list(f["sum"]) == [2.5, 17.0, -10.0, 13.0] and list(f["sumsq"]) == [2.25, 97.0, 34.0, 89.0]
    assert list(f["min"]) == [0.5, 5.0, -4.0, 2.0] and list(f["argmin"]) == [30, 12, 5, 5]      # 2.0 twice: books 12 and 5
    assert list(f["max"]) == [1.0, 6.0, -3.0, 9.0] and list(f["argmax"]) == [5, 5, 12, 30]       # 1.0: 12 and 5; 6.0: 5 and 30; -3.0: 12 and 30
    assert list(i["sum"]) == [16, 26, 0, 13] and list(i["sumsq"]) == [102, 226, 0, 59]
    assert list(i["min"]) == [2, 8, 0, 3] and list(i["argmin"]) == [30, 5, 5, 12]
    assert list(i["max"]) == [7, 9, 0, 5] and list(i["argmax"]) == [5, 12, 5, 5]
    # ties go to the lower id whatever the order of the operands
    for x, y in ((a, b), (b, a)):
        t = engine.merge_episode_stats(x, y)
        assert t["f"]["argmax"][0] == 5 and t["f"]["argmin"][3] == 5 and t["i"]["argmin"][0] == 5 and t["i"]["argmin"][2] == 5


def test_merge_commutes_bitwise():
    rng = np.random.default_rng(3)
    for trial in range(50):
        recs = []
        for side in range(2):
            r = identity(int(rng.integers(-1, 3)))
            for book in rng.integers(0, 1000, size=int(rng.integers(0, 5))):
                r = engine.merge_episode_stats(r, single(int(book), rng.integers(-3, 4, size=4) * 0.1, rng.integers(-3, 4, size=4),
                                                         group=int(r["group"]), terminal=int(rng.integers(0, 3))))
            recs.append(r)
        assert engine.merge_episode_stats(recs[0], recs[1]).tobytes() == engine.merge_episode_stats(recs[1], recs[0]).tobytes()


def test_merge_of_single_books_is_numpy():
    """k one-book records merged in id order against the numpy figures of those k books: integers, counts and extremes exact;
    the f64 sums within the worst-case bound of any summation order, n * 2^-53 * sum|x| (2n * 2^-53 * sum x^2 for the
    squares: one rounding per square as well)."""
    rng = np.random.default_rng(5)
    k = 500
    fv = rng.normal(size=(k, 4)) * np.array([1e3, 1e-2, 50.0, 1.0])
    fv[17] = fv[400]            # a tie in every quantity: the lower id
    iv = rng.integers(0, 3000, size=(k, 4))
    ids = 1000 + np.arange(k)
    m = identity()
    for b in range(k):
        m = engine.merge_episode_stats(m, single(int(ids[b]), fv[b], iv[b]))
    assert m["n_books"] == k and m["n_terminal"] == k and m["n_rho"] == k
    for q in range(4):
        x = fv[:, q]
        s = m["f"][q]
        assert abs(s["sum"] - math.fsum(x)) <= k * EPS * math.fsum(np.abs(x))
        assert abs(s["sumsq"] - math.fsum(x * x)) <= 2 * k * EPS * math.fsum(x * x)
        assert s["min"] == x.min() and s["argmin"] == ids[np.argmin(x)]      # numpy's argmin / argmax: the first = the lowest id
        assert s["max"] == x.max() and s["argmax"] == ids[np.argmax(x)]
        y = iv[:, q].astype(np.int64)
        t = m["i"][q]
        assert t["sum"] == y.sum() and t["sumsq"] == (y * y).sum()
        assert t["min"] == y.min() and t["argmin"] == ids[np.argmin(y)] and t["max"] == y.max() and t["argmax"] == ids[np.argmax(y)]
