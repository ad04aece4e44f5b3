"""What lob_vec_history must write (include/lob_engine.h), in numpy, from the HOST records in the ABI layout (lob_stream.h: time,
flags, ask_px[D], ask_vol[D], bid_px[D], bid_vol[D], trade_px[T], trade_vol[T], padded to a multiple of four words).  Not collected by pytest; used by
tests/test_vec_history_abi.py (which tests it on hand-made records), tests/test_gpu_vec_history.py and
tests/vec_history_torch_child.py."""
import numpy as np

NAMES = ("levels", "trades", "time_ms", "n_valid", "rec")


def record_levels(rows, D):
    """rows: uint32 [..., W] -> (prices f32 [..., 2, D] (ask, bid), volumes i32 [..., 2, D]) of the records' level arrays."""
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    px = np.stack([rows[..., 2:2 + D], rows[..., 2 + 2 * D:2 + 3 * D]], axis=-2).view(np.float32)
    vol = np.stack([rows[..., 2 + D:2 + 2 * D], rows[..., 2 + 3 * D:2 + 4 * D]], axis=-2).view(np.int32)
    return px, vol


def expected_history(records, start, length, rec, K, D, T):
    """records: uint32 [n][W], every stream the engine holds, flat; start[b]: the first record of book b's stream in it; length:
    the records of book b's stream (an int, or one per book); rec[b]: the record of book b's current snapshot within its stream
    (-1: none); K: the window.  -> dict of the five arrays of lob_vec_hist_out."""
    records = np.ascontiguousarray(records, dtype=np.uint32)
    assert records.ndim == 2 and records.shape[1] == (2 + 4 * D + 2 * T + 3) // 4 * 4, "lob_record_words: padded to whole 16 bytes"
    rec = np.asarray(rec, dtype=np.int64)
    B = rec.shape[0]
    start = np.asarray(start, dtype=np.int64)
    length = np.broadcast_to(np.asarray(length, dtype=np.int64), (B,))
    assert start.shape == (B,) and (rec >= -1).all() and (rec < length).all(), "rec lies within the book's own stream"
    idx = rec[:, None] - (K - 1 - np.arange(K, dtype=np.int64))[None, :]        # [B, K]: the record of slot k within the stream
    have = (idx >= 0) & (rec[:, None] >= 0)
    flat = np.where(have, start[:, None] + idx, 0)
    assert (flat >= 0).all() and (flat < records.shape[0]).all()
    rows = records[flat]                                                        # [B, K, W]
    rows = np.where(have[:, :, None], rows, np.uint32(0))
    px, vol = record_levels(rows, D)
    levels = np.stack([px[:, :, 0], vol[:, :, 0].astype(np.float32), px[:, :, 1], vol[:, :, 1].astype(np.float32)], axis=2)
    o = 2 + 4 * D
    trades = np.stack([np.ascontiguousarray(rows[:, :, o:o + T]).view(np.float32),
                       np.ascontiguousarray(rows[:, :, o + T:o + 2 * T]).view(np.int32).astype(np.float32)], axis=2)
    return {"levels": np.ascontiguousarray(levels, dtype=np.float32), "trades": np.ascontiguousarray(trades, dtype=np.float32),
            "time_ms": np.ascontiguousarray(rows[:, :, 0]).view(np.int32),
            "n_valid": np.where(rec >= 0, np.minimum(K, rec + 1), 0).astype(np.int32), "rec": rec.astype(np.int32)}


def assert_record_has_dump_levels(records, start, rec, dump, D, tag, books=None):
    """For the books of the mask (default: every book with rec >= 0): record rec[b] of book b's stream holds exactly the level
    prices and volumes lob_get_books reports (`dump`: tests/parity.py dumps_to_np, or the oracle's)."""
    rec = np.asarray(rec, dtype=np.int64)
    m = (rec >= 0) if books is None else (np.asarray(books, bool) & (rec >= 0))
    rows = np.ascontiguousarray(records, dtype=np.uint32)[(np.asarray(start, dtype=np.int64) + np.maximum(rec, 0))[m]]
    px, vol = record_levels(rows, D)
    for side, name in enumerate(("ask", "bid")):
        np.testing.assert_array_equal(dump[name + "_px"][m][:, :D], px[:, side].astype(np.float64), err_msg="%s: %s_px of the record" % (tag, name))
        np.testing.assert_array_equal(dump[name + "_vol"][m][:, :D], vol[:, side].astype(np.int64), err_msg="%s: %s_vol of the record" % (tag, name))
    return int(m.sum())
