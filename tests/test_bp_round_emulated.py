"""The redraw round of bp_redraw_pairs (csrc/tmg_board.hip, TMG_BP_ROUND) on the
host wave emulator, against the oracle (oracle/tmg_oracle.c): reads carried
over a rejected round, the ring filled after the round's reads, and rp_move's
closing LDS write left out ahead of an inline regeneration.  Every field;
the accepted and rejected second redraws are those the oracle's trace
predicts (bp_pair_cases.pair_rounds), and every rejected round carries its
reads into the next one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bp_pair_cases import PAIR_SHAPES
from bp_round_cases import REJECTION_SHAPE, ROUND_SHAPE, carried_rejection_words, predicted, round_words
from rowplane_cases import FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


def _load(name):
    subprocess.run(["make", "-C", EMU_DIR, name], check=True, stdout=subprocess.DEVNULL)
    if EMU_DIR not in sys.path:
        sys.path.insert(0, EMU_DIR)
    import emu
    old = os.environ.get("EMU_LIB")
    os.environ["EMU_LIB"] = name
    try:
        return emu, emu.load()
    finally:
        if old is None:
            del os.environ["EMU_LIB"]
        else:
            os.environ["EMU_LIB"] = old


@pytest.fixture(scope="module")
def emu_lib():
    return _load("libwave_emu.so")


def _same(e, o, what):
    for f in FIELDS:
        got, want = getattr(e, f), getattr(o, f)
        if not np.array_equal(got, want):
            n = got.shape[0]
            bad = np.nonzero((got.reshape(n, -1) != want.reshape(n, -1)).any(axis=1))[0]
            raise AssertionError(f"{what}: {f} differs in {bad.size} envs, first {bad[:5]}")


def _hits(emu, L):
    from tile_match_gym_amd._native import COVER_NAMES
    return {nm: int(x) for nm, x in zip(COVER_NAMES, emu.cover(L, True))}


def _regenerate_both_ways(emu, L, shape, w, what):
    """The streams through reset, then through the same-step autoreset after
    an episode's only move, an ineffective one (the regeneration starts from w
    itself).  Returns the cover counts of the two passes."""
    from oracle import oracle as orc
    R, C, k = shape
    e = emu.EmuBatch(L, R, C, k, 0, 1, w)
    o = orc.OracleBatch(R, C, k, 0, 1, w)
    emu.cover(L, True)
    e.reset()
    o.reset()
    _same(e, o, f"{what}: reset")
    h_reset = _hits(emu, L)
    a = np.zeros(o.n, np.int32)
    for i in range(o.n):
        free = np.nonzero(~orc.effective_mask(o.board[i])[0])[0]
        a[i] = free[0] if free.size else 0
    e.rng[:] = w
    o.rng[:] = w
    e.step(a, True)
    o.step(a, True)
    _same(e, o, f"{what}: autoreset")
    assert (o.flags & 1).all()
    h_step = _hits(emu, L)
    assert L.emu_status() == 0
    return h_reset, h_step


def test_round_sequences_emulated(emu_lib):
    """10x10 k4: a board of more than 300 redraws, rounds going reject, reject,
    accept, streams that start with a buffered half-word."""
    from oracle import oracle as orc
    emu, L = emu_lib
    w = round_words(orc)
    assert (w[:, 4] >> np.uint64(32)).any() and not (w[:, 4] >> np.uint64(32)).all()
    acc, rej, longest = predicted(orc, ROUND_SHAPE, w)
    assert longest > 300 and rej >= 2 * 24
    for h in _regenerate_both_ways(emu, L, ROUND_SHAPE, w, "round sequences"):
        assert h["shuffle_gen"] == 0 and h["reject_gen"] == 0, h
        assert (h["bp_pair_acc"], h["bp_pair_rej"]) == (acc, rej), (h, acc, rej)
        assert h["bp_round_carry"] == rej, h


def test_rejected_word_in_carried_redraw_emulated(emu_lib):
    """10x10 k5: a Lemire-rejected word among the colours of a redraw that was
    carried over; the board is redone exactly."""
    from oracle import oracle as orc
    emu, L = emu_lib
    w, _ = carried_rejection_words(orc)
    assert {int(x >> np.uint64(32)) for x in w[:, 4]} == {0, 1}
    for h in _regenerate_both_ways(emu, L, REJECTION_SHAPE, w, "rejection in a carried redraw"):
        assert h["reject_gen"] == w.shape[0], h
        assert h["bp_round_carry"] >= w.shape[0] and h["bp_round_carry"] == h["bp_pair_rej"], h


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=str)
def test_shapes_emulated(emu_lib, shape):
    from oracle import oracle as orc
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    w = batch_rng_words(range(7300, 7364))
    acc, rej, _ = predicted(orc, shape, w)
    for h in _regenerate_both_ways(emu, L, shape, w, str(shape)):
        assert h["bp_round_carry"] == h["bp_pair_rej"], h
        if h["shuffle_gen"] == 0 and h["reject_gen"] == 0:
            assert (h["bp_pair_acc"], h["bp_pair_rej"]) == (acc, rej), (h, acc, rej)


@pytest.mark.parametrize("shape", [(10, 10, 4), (10, 10, 5), (4, 4, 3), (16, 8, 4)], ids=str)
def test_effective_last_move_emulated(emu_lib, shape):
    """Episodes of one move, every move effective, same-step autoreset: the
    row-plane move is followed in the same wave by the regeneration, with and
    without the final board asked for (with it the move still writes LDS)."""
    from oracle import oracle as orc
    from oracle.policy_np import sample_effective_np
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    R, C, k = shape
    n = 32
    for final in (False, True):
        w = batch_rng_words(range(7700, 7700 + n))
        e = emu.EmuBatch(L, R, C, k, 0, 1, w)
        o = orc.OracleBatch(R, C, k, 0, 1, w)
        e.reset()
        o.reset()
        emu.cover(L, True)
        for t in range(4):
            a = sample_effective_np(o.eff, e.A, 9, 0, t)
            last, wprev = o.board.copy(), o.rng.copy()
            out = {"final_board": np.zeros((n, 2, R, C), np.int8)} if final else None
            e.step(a, True, outputs=out)
            o.step(a, True)
            _same(e, o, f"{shape} final={final} step {t}")
            assert (o.flags & 1).all() and (o.reward >= 3).all()
            if final:                                     # the board before its regeneration: the oracle's move
                for i in range(n):
                    mb, _, _, err = orc.move(last[i], wprev[i], int(a[i]), k, 0)
                    assert err == 0 and np.array_equal(out["final_board"][i], mb), (shape, t, i)
        h = _hits(emu, L)
        assert h["sb_lean"] > 0 and (h["rp_nolds"] == 0) == final, (final, h)
        assert L.emu_status() == 0


def test_ab_side_emulated():
    """TMG_BP_ROUND=0: the previous round computes the same and carries nothing."""
    from oracle import oracle as orc
    emu, L = _load("libwave_emu_bpr0.so")
    w = round_words(orc, n_pattern=6, n_buffered=6)[1:]
    acc, rej, _ = predicted(orc, ROUND_SHAPE, w)
    for h in _regenerate_both_ways(emu, L, ROUND_SHAPE, w, "TMG_BP_ROUND=0"):
        assert (h["bp_pair_acc"], h["bp_pair_rej"]) == (acc, rej), (h, acc, rej)
        assert h["bp_round_carry"] == 0 and h["rp_nolds"] == 0, h
