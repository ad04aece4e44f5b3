"""TEST INFRASTRUCTURE: the multi-GPU weight exchange restated in numpy -- no engine, no HIP.

What the exchange kernels compute is three IEEE operations and a prefix sum (theta - theta_sync, the packed layout in index order,
theta_sync + sum), so it can be held bit for bit: tests/test_gpu_exchange_edges.py compares the bit patterns of what the device
wrote with what these functions return, and tests/test_exchange_ref.py holds the functions themselves against a per-bit Python loop.

Conventions: a map is uint32[words]; weight i is bit i & 31 of word i >> 5.  Sums over ranks are formed IN RANK ORDER (rank 0's term
first), the order the tests' host all-reduce uses (rank_sum below)."""
import numpy as np


def bits(a):
    """The f64 bit patterns: -0.0 and NaN cannot hide behind ==."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def rank_sum(terms):
    """terms[0] + terms[1] + ... in that order (no 0 in front: -0.0 stays -0.0)."""
    tot = np.array(terms[0], np.float64, copy=True)
    for t in terms[1:]:
        tot = tot + t
    return tot


def union_layout(maps):
    """-> (the OR of the maps, the ascending weight indices of its set bits as int64)."""
    u = np.zeros_like(np.asarray(maps[0], np.uint32))
    for m in maps:
        m = np.asarray(m, np.uint32)
        assert m.shape == u.shape
        u = u | m
    by_bit = np.unpackbits(np.ascontiguousarray(u).astype("<u4").view(np.uint8), bitorder="little")
    return u, np.flatnonzero(by_bit).astype(np.int64)


def dense_expected(thetas, sync):
    """-> dict: "deltas" theta_r - sync per rank, "total" their rank-order sum, "theta" sync + total (every rank's weights and base
    after the apply)."""
    deltas = [np.asarray(t, np.float64) - sync for t in thetas]
    total = rank_sum(deltas)
    return {"deltas": deltas, "total": total, "theta": sync + total}


def sparse_expected(thetas, sync, maps, count):
    """The sparse exchange of `count` doubles.  sync: one vector common to the ranks, or one per rank.
    -> dict: "union", "idx" (union_layout), "moved" = idx[:count] (the weights this exchange carries), "packed" per rank
    (theta_r[f_p] - sync_r[f_p] for p < min(count, |union|), 0.0 behind the union up to count), "total" their rank-order sum,
    "theta" / "sync" per rank after the apply: sync_r[f_p] + total[p] at the moved weights, every other weight -- the surplus
    p >= count included -- as before."""
    world = len(thetas)
    syncs = list(sync) if isinstance(sync, (list, tuple)) else [sync] * world
    union, idx = union_layout(maps)
    moved = idx[:max(int(count), 0)]
    packed = []
    for t, s in zip(thetas, syncs):
        buf = np.zeros(int(count), np.float64)
        buf[:moved.size] = np.asarray(t, np.float64)[moved] - s[moved]
        packed.append(buf)
    total = rank_sum(packed)
    theta_after, sync_after = [], []
    for t, s in zip(thetas, syncs):
        t2, s2 = np.array(t, np.float64, copy=True), np.array(s, np.float64, copy=True)
        new = s[moved] + total[:moved.size]
        t2[moved] = new
        s2[moved] = new
        theta_after.append(t2)
        sync_after.append(s2)
    return {"union": union, "idx": idx, "moved": moved, "packed": packed, "total": total, "theta": theta_after, "sync": sync_after}


def rho_expected(rhos, rho_sync):
    """The two slots behind the weights of the average-reward agents.
    -> dict: "slots" [rho_r - rho_sync, 1.0] per rank, "total" their rank-order sum, "rho" = rho_sync + total[0] / total[1]
    (the second slot sums to the number of ranks)."""
    slots = [np.array([np.float64(r) - np.float64(rho_sync), 1.0]) for r in rhos]
    total = rank_sum(slots)
    return {"slots": slots, "total": total, "rho": np.float64(rho_sync) + total[0] / total[1]}
