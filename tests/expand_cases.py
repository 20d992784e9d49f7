"""Shapes and the oracle side of the tmg_expand tests (tests/test_expand_emulated.py
on the host wave emulator, tests/test_gpu_expand.py on the device).

The expected children come from the oracle only: the child list is built with
numpy (counts, np.repeat, the action list from the mask bits) and the copies
are stepped by OracleBatch.step(actions, autoreset=False).  Nothing here has a
tolerance: every array is compared with np.array_equal."""
import numpy as np

import edge_cases
from oracle import oracle as orc

# (R, C, k, smask): 3x5 (N = 15) and 7x9 (N = 63) have child rows that start on
# 2-byte boundaries; 4x4 is 8 dwords a board, 10x10 is 50
EMULATED_SHAPES = [(3, 5, 2, 0), (4, 4, 2, 0), (7, 9, 10, 15), (10, 10, 4, 0), (10, 10, 4, 14), (8, 8, 3, 15)]
# on the device also C = 64 (no bitboards) and the 512-cell family (W = 12)
DEVICE_SHAPES = EMULATED_SHAPES + [(2, 64, 4, 0), (20, 20, 6, 15), (20, 20, 6, 0)]
# the limits of the accepted domain (tests/edge_cases.py): 63 actions all horizontal, all
# vertical, 64 rows of 8 (W = 15), W = 16.  On the device all four; on the emulator (8.7 s at
# most, measured) all but 1x64, one of whose envs has a single child, which that test excludes
LIMIT_SHAPES = list(edge_cases.LOOKAHEAD_DEVICE)
DEVICE_SHAPES = DEVICE_SHAPES + LIMIT_SHAPES
EMULATED_LIMIT_SHAPES = [s for s in LIMIT_SHAPES if s != (1, 64, 5, 15)]

STATE = ("board", "rng", "timer", "eff")
OUTPUTS = ("reward", "n_new", "n_act", "flags")
FIELDS = ("first_child", "parent", "action") + STATE + OUTPUTS

FLAG_DONE, FLAG_ERROR = 1, 0x80


def case_id(s):
    return "{}x{}k{}s{}".format(*s)


def envs_of(shape):
    """Envs per parity case: 5, or 3 for the 512-cell family."""
    return 3 if shape[0] * shape[1] > 128 else 5


def unpack_mask(words, A):
    """(n, W) uint64 mask words -> (n, A) bool."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    by = w.view(np.uint8).reshape(w.shape[0], 8 * w.shape[1])
    return np.unpackbits(by, axis=1, bitorder="little")[:, :A].astype(bool)


def pack_mask(mask):
    """(n, A) bool -> (n, W) uint64 mask words, bit a of word a // 64."""
    mask = np.asarray(mask, dtype=bool)
    n, A = mask.shape
    W = (A + 63) // 64
    bits = np.zeros((n, W * 64), np.uint8)
    bits[:, :A] = mask
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n, W).copy()


def oracle_expand(board, rng, timer, eff, select, k, smask, num_moves, threads=1):
    """board (n, 2, R, C) int8, rng (n, 5) uint64, timer (n,) int32, eff (n, W)
    uint64, select (n, A) bool or None -> dict of first_child (n + 1,) int64,
    parent (m,) int64, action (m,) int32, the four state arrays of the m
    children after the move and its four outputs.  The inputs are not changed."""
    n, _, R, C = board.shape
    A = orc.num_actions(R, C)
    mask = unpack_mask(eff, A)
    if select is not None:
        mask = mask & np.asarray(select, dtype=bool)
    mask = mask & (np.asarray(timer) < num_moves)[:, None]
    counts = mask.sum(axis=1).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    parent = np.repeat(np.arange(n, dtype=np.int64), counts)
    action = np.nonzero(mask)[1].astype(np.int32)              # row-major: env-major, ascending action
    m = int(first[n])
    o = orc.OracleBatch(R, C, k, smask, num_moves, np.ascontiguousarray(rng, dtype=np.uint64)[parent].reshape(m, 5),
                        threads=threads)
    o.board[:], o.timer[:], o.eff[:] = board[parent], timer[parent], eff[parent]
    if m:
        o.step(action, autoreset=False)
    out = {"first_child": first, "parent": parent, "action": action}
    out.update({f: getattr(o, f) for f in STATE + OUTPUTS})
    return out


def assert_expand_equal(got, want, what="", fields=FIELDS):
    for f in fields:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, f"{what}: {f} has shape {g.shape}, want {w.shape}"
        if not np.array_equal(g, w):
            rows = np.nonzero((g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(axis=1))[0][:5]
            raise AssertionError(f"{what}: {f} differs in rows {rows.tolist()}: "
                                 f"got {g[rows].tolist()}, want {w[rows].tolist()}")
