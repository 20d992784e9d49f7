"""tmg_rollout on the host wave emulator (CPU): the rollout kernels of
csrc/tmg_rollout.hip, picked by peek_ladder (csrc/tmg_dispatch.h) and followed
by the rollout spill pass and the reduce kernel of csrc/tmg_aux.hip, against
the oracle's moves and policy draws of every (sample, env, action)
(tests/rollout_cases.py oracle_rollout).  Everything is compared as integers;
nothing here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dispatch_cases
import peek_cases
import rollout_cases as rc
from adversarial import adversarial_boards
from peek_cases import oracle_peek
from rollout_cases import assert_rollout_equal, oracle_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")
MOVES = 30


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    return emu, emu.load()


def _cover(emu, L):
    from tile_match_gym_amd._native import COVER_NAMES
    return {nm: int(x) for nm, x in zip(COVER_NAMES, emu.cover(L, True))}


def _rollout(emu, L, shape, board, rng, timer, eff, trust_eff, depth, samples, key=rc.KEY, first_env=rc.FIRST_ENV,
             t=rc.T):
    R, C, k, sm = shape
    return emu.rollout(L, R, C, k, sm, MOVES, board, rng, timer, eff, trust_eff, depth, samples, key, first_env, t)


@pytest.mark.parametrize("shape", peek_cases.SHAPES + peek_cases.LIMIT_SHAPES, ids=peek_cases.case_id)
def test_rollout_vs_oracle(emu_lib, shape):
    """After 7 uniform-random steps (boards that hold specials) and after a
    reset; env 0 two moves from the end of its episode and, after the reset,
    the last env at its end; sample 0 with the envs' own RNG words, sample 1
    with words of other seeds."""
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    R, C, k, sm = shape
    n = peek_cases.envs_of(shape)
    other = batch_rng_words(range(7000, 7000 + n))
    depth, samples = 4, 2
    _cover(emu, L)
    for steps in (7, 0):
        o = peek_cases.rolled_batch(shape, range(500, 500 + n), steps=steps, num_moves=MOVES)
        timer = rc.horizon_timers(o, finished=steps == 0)
        rng = np.stack([o.rng, other])
        before = (o.board.copy(), rng.copy(), timer.copy(), o.eff.copy())
        got = _rollout(emu, L, shape, o.board, rng, timer, o.eff, 1, depth, samples)
        want = oracle_rollout(o.board, rng, timer, MOVES, k, sm, depth, samples, rc.KEY, rc.FIRST_ENV, rc.T)
        assert_rollout_equal(got, want, f"{shape} steps={steps}")
        assert (want["plies"][:, 0] <= 2).all() and (want["plies"][:, 0] == 2).any()
        if steps == 0:
            assert not want["plies"][:, -1].any()
        assert all(np.array_equal(x, y) for x, y in zip(before, (o.board, rng, timer, o.eff)))
    c = _cover(emu, L)
    assert c["roll_ply"] > 0 and c["roll_horizon"] > 0, c
    assert L.emu_status() == 0


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)], ids=peek_cases.case_id)
def test_rollout_depth1_is_peek(emu_lib, shape):
    emu, L = emu_lib
    R, C, k, sm = shape
    n = peek_cases.envs_of(shape)
    o = peek_cases.rolled_batch(shape, range(500, 500 + n), steps=7, num_moves=MOVES)
    got = _rollout(emu, L, shape, o.board, o.rng, o.timer, o.eff, 1, 1, 1)
    want = oracle_peek(o.board, o.rng, k, sm)
    assert np.array_equal(got["ret"][0], want["reward"])
    assert np.array_equal(got["flags"][0], want["flags"])
    assert np.array_equal(got["total"], want["reward"])
    assert np.array_equal(got["best_action"], want["best_action"])
    assert np.array_equal(got["best_total"], want["best_reward"])
    assert np.array_equal(got["plies"][0], np.stack([orc_mask(o.board[i]) for i in range(n)]).astype(np.int32))
    assert L.emu_status() == 0


def test_rollout_no_horizon(emu_lib):
    """timer = None: every effective action is played to the full depth, also
    from an env whose timer (not passed) is at the end."""
    emu, L = emu_lib
    shape = (8, 8, 3, 15)
    R, C, k, sm = shape
    n = peek_cases.envs_of(shape)
    depth = 5
    o = peek_cases.rolled_batch(shape, range(500, 500 + n), steps=7, num_moves=MOVES)
    got = _rollout(emu, L, shape, o.board, o.rng, None, o.eff, 1, depth, 1)
    want = oracle_rollout(o.board, o.rng[None], None, MOVES, k, sm, depth, 1, rc.KEY, rc.FIRST_ENV, rc.T)
    assert_rollout_equal(got, want, str(shape))
    mask = np.stack([orc_mask(o.board[i]) for i in range(n)])
    assert np.array_equal(got["plies"][0], np.where(mask, depth, 0))
    assert L.emu_status() == 0


def orc_mask(board):
    from oracle import oracle as orc
    return orc.effective_mask(board)[0]


@pytest.mark.parametrize("shape,mode,many", peek_cases.spill_params(device=False))
def test_rollout_untrusted_and_spill(emu_lib, shape, mode, many):
    """Hand-written boards (they may hold lines and any special), no mask
    given: ply 0 scans its own mask and searches the whole board for lines, the
    general kernels run, and a virtual env one of whose plies outgrows the LDS
    lists is re-run whole by the spill pass.  many: more spilling virtual envs
    than the spill pass has waves."""
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    R, C, k, sm = shape
    n = peek_cases.MANY_SPILLS[shape][1] if many else peek_cases.envs_of(shape)
    depth, samples = 2 if many else 3, 2
    b = adversarial_boards(n, R, C, k, sm, 11, mode)
    words = np.stack([batch_rng_words(range(300, 300 + n)), batch_rng_words(range(340, 340 + n))])
    s0 = L.emu_spills()
    _cover(emu, L)
    got = _rollout(emu, L, shape, b, words, None, None, 0, depth, samples)
    want = oracle_rollout(b, words, None, MOVES, k, sm, depth, samples, rc.KEY, rc.FIRST_ENV, rc.T)
    assert_rollout_equal(got, want, f"{shape} {mode}")
    assert L.emu_status() == 0
    c = _cover(emu, L)
    assert c["roll_spill"] == c["roll_spill_run"], c
    if (R, C) in ((20, 20), (10, 10)) and mode != "stripes":
        assert L.emu_spills() > s0, "the adversarial boards were meant to outgrow the LDS lists"
        assert c["roll_spill"] > 0, c
    if many:
        assert L.emu_spills() - s0 > peek_cases.SPILL_WAVES
    if mode == "combo_grid":
        assert (got["flags"] & rc.FLAG_COMBO).any()


SHUFFLE_ENVS = 16


@pytest.mark.parametrize("shape", dispatch_cases.SHUFFLES, ids=peek_cases.case_id)
def test_rollout_cover(emu_lib, shape):
    """The boards of dispatch_cases.SHUFFLES shuffle inside continuation plies
    (asserted on the oracle first)."""
    emu, L = emu_lib
    R, C, k, sm = shape
    depth = 4
    o = peek_cases.rolled_batch(shape, range(500, 500 + SHUFFLE_ENVS), steps=7, num_moves=MOVES)
    at = []
    want = oracle_rollout(o.board, o.rng[None], o.timer, MOVES, k, sm, depth, 1, rc.KEY, rc.FIRST_ENV, rc.T,
                          shuffled_at=at)
    assert any(d >= 1 for d in at), f"{shape}: no continuation ply shuffles on the oracle"
    _cover(emu, L)
    got = _rollout(emu, L, shape, o.board, o.rng, o.timer, o.eff, 1, depth, 1)
    c = _cover(emu, L)
    assert c["roll_ply"] > 0 and c["shuffle"] > 0, c
    assert np.array_equal(got["flags"], want["flags"])
    assert_rollout_equal(got, want, str(shape))
    assert L.emu_status() == 0
