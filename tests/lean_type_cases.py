"""The lean step's type check (csrc/tmg_board.hip step_env, "lean variant
precondition"): a trusted tmg_step on a no-specials board that meets a
non-normal tile flags that env with TMG_FLAG_ERROR, leaves its board, RNG words
and timer alone and raises TMG_STATUS_INTERNAL; every other env of the launch
steps as the oracle does.  One case per wave-per-board lean step kernel; the
lane-per-board kernel reads only the colour plane and has no such check
(include/tmg.h, tmg_step).

Shared by tests/test_special_matrix.py (host wave emulator) and
tests/test_gpu_special_matrix.py (device).  `step` is the thing under test:
    step(shape, board, rng, timer, eff, actions, fused) -> dict of board, rng, timer, reward, n_new, n_act, flags,
        status, and terminated ((n, 4) uint8) when fused
one trusted tmg_step with autoreset off on copies, `fused` attaching the
`terminated` output of tmg_plan_config."""
import numpy as np

from oracle import oracle as orc

FLAG_ERROR, STATUS_INTERNAL = 0x80, 1
FIX_C2 = 10 << 24 | 10 << 16 | 4 << 8
N_ENVS, PLANTED, MOVES = 5, 2, 30

# name: (shape, fused, <MAXN, GEN, NB, CODD, FIX> of the trusted step, plain)
CASES = {
    "row planes 10x10 k5": ((10, 10, 5, 0), False, (128, 0, 3, 0, 0), 0),
    "tall sb_move 17x7 k4": ((17, 7, 4, 0), False, (128, 0, 2, 1, 0), 0),
    "fixed c2, fused output": ((10, 10, 4, 0), True, (128, 0, 2, 0, FIX_C2), 0),
    "plain c2": ((10, 10, 4, 0), False, (128, 0, 2, 0, FIX_C2), 1),
    "C = 64": ((2, 64, 4, 0), False, (128, 0, 0, 0, 0), 0),
    "512 cells": ((20, 20, 6, 0), False, (512, 0, 0, 0, 0), 0),
}


def check(step, name):
    from tile_match_gym_amd.seeding import batch_rng_words
    shape, fused, _, _ = CASES[name]
    R, C, k, sm = shape
    ref = orc.OracleBatch(R, C, k, sm, MOVES, batch_rng_words(range(4100, 4100 + N_ENVS)))
    ref.reset()
    actions = np.array([np.nonzero(orc.effective_mask(b)[0])[0][0] for b in ref.board], np.int32)    # an effective move each
    board = ref.board.copy()
    board[PLANTED, 1, R // 2, C // 2] = 2                          # one vertical laser in one env
    before = (board.copy(), ref.rng.copy(), ref.timer.copy())
    got = step(shape, board.copy(), ref.rng.copy(), ref.timer.copy(), ref.eff.copy(), actions, fused)
    ref.step(actions, autoreset=False)
    others = np.arange(N_ENVS) != PLANTED
    assert (ref.reward[others] > 0).all(), "a move that was meant to be effective"
    for f, was in zip(("board", "rng", "timer"), before):
        g = np.asarray(got[f])
        g = g.view(np.uint64) if g.dtype == np.int64 and was.dtype == np.uint64 else g
        assert np.array_equal(g[PLANTED], was[PLANTED]), f"{name}: the planted env's {f} changed"
        assert np.array_equal(g[others], getattr(ref, f)[others]), f"{name}: {f} of the other envs"
    assert got["flags"][PLANTED] == FLAG_ERROR
    assert (got["reward"][PLANTED], got["n_new"][PLANTED], got["n_act"][PLANTED]) == (0, 0, 0)
    for f in ("reward", "n_new", "n_act", "flags"):
        assert np.array_equal(np.asarray(got[f])[others], getattr(ref, f)[others]), f"{name}: {f} of the other envs"
    assert got["status"] == STATUS_INTERNAL
    if fused:
        assert got["terminated"][PLANTED].tolist() == [0, 0, 0, 1]
        assert np.array_equal(got["terminated"][others], np.stack([ref.flags[others] >> i & 1 for i in (0, 1, 2, 7)], 1))
