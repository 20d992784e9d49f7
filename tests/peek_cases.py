"""Shapes and the oracle side of the tmg_peek tests (tests/test_peek_emulated.py
on the host wave emulator, tests/test_gpu_peek.py on the device).

The expected values come from the oracle only: oracle.move per (env, action),
which runs Board.move (board.py:330-395) on a copy of the board with a copy of
the RNG words and reports zeros for an ineffective action."""
import numpy as np

import dispatch_cases
import edge_cases
from oracle import oracle as orc

# (R, C, k, smask)
EXTRA = [(10, 10, 4, 0), (10, 10, 4, 14), (8, 8, 3, 15), (20, 20, 6, 15), (20, 20, 6, 0)]
# lean, 1 colour plane, even C: peek<128,0,1,0>, which no shape above reaches
ONE_PLANE_EVEN = (4, 4, 2, 0)
SHAPES = list(dispatch_cases.CASES) + [dispatch_cases.ROW_PLANE_CONTROL] + EXTRA + [ONE_PLANE_EVEN]
# the limits of the accepted domain (tests/edge_cases.py): 63 actions all horizontal, all
# vertical, 64 rows of 8, 16 mask words.  Only the *_vs_oracle tests take them, on the device
# and, each running in under 3 s there, on the emulator (measured: peek 1.4 s, rollout 2.9 s)
LIMIT_SHAPES = list(edge_cases.LOOKAHEAD_DEVICE)
# the adversarial boards of the untrusted / spill tests (tests/adversarial.py)
ADVERSARIAL_SHAPES = [(20, 20, 6, 15), (10, 10, 4, 14), (8, 8, 3, 15)]

# laser_sea boards, every one of which spills, more of them than a spill launch
# has waves (kSpillWaves, csrc/tmg_board.hip): a wave of the drain then takes a
# second env and reuses its workspace.  shape -> envs for peek, for rollout (at
# 2 samples, depth 2); the 512-cell family on the device only (the emulator
# needs about a minute for it)
SPILL_WAVES = 16          # kSpillWaves: raise both together, and the env counts below past it
MANY_SPILLS = {(10, 10, 4, 14): (24, 12), (20, 20, 6, 15): (20, 10)}

FLAG_COMBO, FLAG_SHUFFLED, FLAG_ERROR = 2, 4, 0x80
FIELDS = ("reward", "n_new", "n_act", "flags", "best_action", "best_reward")

case_id = dispatch_cases.case_id


def spill_params(device):
    """(shape, mode, many) of the untrusted / spill tests: every mode on every
    adversarial shape with envs_of(shape) envs, then MANY_SPILLS."""
    import pytest
    from adversarial import MODES
    ps = [pytest.param(s, m, False, id=f"{case_id(s)}-{m}") for m in MODES for s in ADVERSARIAL_SHAPES]
    return ps + [pytest.param(s, "laser_sea", True, id=f"{case_id(s)}-laser_sea-many") for s in MANY_SPILLS
                 if device or s[0] * s[1] <= 128]


def envs_of(shape):
    """Envs per case: 4, or 2 for the 512-cell family."""
    return 2 if shape[0] * shape[1] > 128 else 4


def oracle_peek(board, rng, k, smask):
    """board (n, 2, R, C) int8, rng (n, 5) uint64 -> dict of reward / n_new /
    n_act (n, A) int32, flags (n, A) uint8 (combo 2 | shuffled 4), best_action /
    best_reward (n,) int32 (the lowest action of maximal reward; 0, 0 when no
    action is effective).  The inputs are not changed."""
    n, _, R, C = board.shape
    A = orc.num_actions(R, C)
    out = {f: np.zeros((n, A), np.int32) for f in ("reward", "n_new", "n_act")}
    out["flags"] = np.zeros((n, A), np.uint8)
    for i in range(n):
        for a in range(A):
            _, _, res, err = orc.move(board[i], rng[i], a, k, smask)
            assert err == 0, (i, a, err)
            out["reward"][i, a], combo, out["n_new"][i, a], out["n_act"][i, a], shuf = (int(x) for x in res)
            out["flags"][i, a] = (FLAG_COMBO if combo else 0) | (FLAG_SHUFFLED if shuf else 0)
    out["best_action"] = out["reward"].argmax(axis=1).astype(np.int32)         # the first of the maxima
    out["best_reward"] = out["reward"].max(axis=1).astype(np.int32)
    return out


def rolled_batch(shape, seeds, steps=7, num_moves=30):
    """An OracleBatch of the shape after reset() and `steps` uniform-random steps."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k, sm = shape
    o = orc.OracleBatch(R, C, k, sm, num_moves, batch_rng_words(seeds))
    o.reset()
    rs = np.random.default_rng(R * 1000 + C * 10 + k)
    for _ in range(steps):
        o.step(rs.integers(0, o.A, o.n).astype(np.int32))
    return o


def assert_peek_equal(got, want, what=""):
    for f in FIELDS:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(np.asarray(got[f]) != np.asarray(want[f]))[:5]
            raise AssertionError(f"{what}: {f} differs at {bad.tolist()}: "
                                 f"got {[int(got[f][tuple(b)]) for b in bad]}, "
                                 f"want {[int(want[f][tuple(b)]) for b in bad]}")
