"""TEST INFRASTRUCTURE: the tile indices of states (oracle_tiles) and numpy sums over them, shared by the CPU and the GPU tests."""
import numpy as np

from rl_markets_amd import abi
from tests import oracle_lib as ol

NA, NT = abi.LOB_N_ACTIONS, 96


def tiles(M, rows):
    rows = np.ascontiguousarray(rows, np.float32)
    f = np.zeros((rows.shape[0], NA, NT), np.int32)
    ol.load().oracle_tiles(M, ol.ptr(rows), rows.shape[1], rows.shape[0], ol.ptr(f))
    return f


def expected_theta(M, F, actions, step, into=None):
    th = np.zeros(M, np.float64) if into is None else into
    ok = (actions >= 0) & (actions < NA)
    idx = F[np.nonzero(ok)[0], actions[ok]]                      # [n_ok][96]
    np.add.at(th, idx.ravel(), np.repeat(step[ok], NT))
    return th
