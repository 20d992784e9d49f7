"""bp_generate's paired redraw loop (csrc/tmg_board.hip, bp_redraw_pairs) on
the host wave emulator, against the oracle (oracle/tmg_oracle.c): the
regenerated board, the PCG64 state with its buffered half-word, the effective
mask and the flags, through reset and through a same-step autoreset that
follows an episode's last move.  The emulator counts the second redraws the
loop accepted and rejected; where no shuffle and no Lemire rejection
intervenes the counts are those the oracle's trace of each board predicts
(bp_pair_cases.pair_rounds).  The emulator is built with TMG_BP_PAIR=2: the
paired loop in every kernel whose shape fits, the generic ones included (the
library pairs only in its shape-specialised kernels)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bp_pair_cases import OLD_LOOP_SHAPE, PAIR_SHAPES, long_board_seed, pair_rounds, rejection_cases, trace_generate
from rowplane_cases import FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")
BUF_VALUES = (0x9ABCDEF0, 0x13572468, 0x5A5A5A5A, 0xC0FFEE11)


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


def _idle_actions(orc, o):
    """An ineffective action per env (a move that counts and draws nothing); 0 where every action is effective."""
    a = np.zeros(o.n, np.int32)
    for i in range(o.n):
        free = np.nonzero(~orc.effective_mask(o.board[i])[0])[0]
        a[i] = free[0] if free.size else 0
    return a


def _regenerate_both_ways(emu, L, shape, w, what):
    """The streams w through reset, then again through the same-step
    autoreset after the last move of an episode of one move (an ineffective
    move, so the regeneration starts from w itself).  Returns the cover counts
    of the two passes."""
    from oracle import oracle as orc
    R, C, k = shape
    e = emu.EmuBatch(L, R, C, k, 0, 1, w)
    o = orc.OracleBatch(R, C, k, 0, 1, w)
    emu.cover(L, True)
    e.reset()
    o.reset()
    _same(e, o, f"{what}: reset")
    h_reset = _hits(emu, L)
    a = _idle_actions(orc, o)
    e.rng[:] = w
    o.rng[:] = w
    e.step(a, True)
    o.step(a, True)
    _same(e, o, f"{what}: autoreset")
    assert (o.flags & 1).all(), "every env's episode ended"
    h_step = _hits(emu, L)
    assert L.emu_status() == 0
    return h_reset, h_step


def _predicted(shape, w):
    from oracle import oracle as orc
    R, C, k = shape
    tot = np.zeros(3, np.int64)
    longest = 0
    for i in range(w.shape[0]):
        rows = trace_generate(orc, R, C, k, w[i])[0]
        tot += pair_rounds(rows)
        longest = max(longest, len(rows))
    return int(tot[1]), int(tot[2]), longest


def test_flagship_shape_emulated(emu_lib):
    """10x10 k4, 300 streams, one of them picked with the oracle's trace for a
    board of more than 300 redraws: every field, both ways, and exactly the
    accepted and rejected second redraws the traces predict."""
    from oracle import oracle as orc
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    shape = (10, 10, 4)
    long_seed = long_board_seed(orc, *shape, range(2000, 2300), 300)
    w = batch_rng_words([long_seed] + list(range(5000, 5299)))
    acc, rej, longest = _predicted(shape, w)
    assert longest > 300 and acc > 0 and rej > 0
    for h in _regenerate_both_ways(emu, L, shape, w, "10x10 k4"):
        assert h["shuffle_gen"] == 0 and h["reject_gen"] == 0, h
        assert (h["bp_pair_acc"], h["bp_pair_rej"]) == (acc, rej), (h, acc, rej)


def test_buffered_half_word_emulated(emu_lib):
    """Streams that start with a buffered half-word: the ring's first colour
    sits at index 127 (cons0 = 127) and the first batch begins at 128."""
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    shape = (10, 10, 4)
    w = batch_rng_words(range(6000, 6032))
    for i in range(w.shape[0]):
        w[i, 4] = np.uint64((1 << 32) | BUF_VALUES[i % len(BUF_VALUES)])
    acc, rej, _ = _predicted(shape, w)
    for h in _regenerate_both_ways(emu, L, shape, w, "buffered"):
        assert (h["bp_pair_acc"], h["bp_pair_rej"]) == (acc, rej), (h, acc, rej)


def test_rejections_emulated(emu_lib):
    """10x10 k5: a Lemire-rejected word among the colours of an accepted
    second redraw (the board is redone exactly), and one that is the first
    draw past the board's last colour (filled ahead, never consumed: the
    result is the oracle's either way)."""
    from oracle import oracle as orc
    emu, L = emu_lib
    shape = (10, 10, 5)
    inside, beyond = rejection_cases(orc, *shape)
    for what, (w, _) in (("inside", inside), ("beyond", beyond)):
        assert {int(x >> np.uint64(32)) for x in w[:, 4]} == {0, 1}, "with and without a buffered half-word"
        h_reset, h_step = _regenerate_both_ways(emu, L, shape, w, f"rejection {what}")
        if what == "inside":
            assert h_reset["reject_gen"] == w.shape[0] and h_step["reject_gen"] == w.shape[0], (h_reset, h_step)
            assert h_reset["bp_pair_acc"] >= w.shape[0], h_reset


@pytest.mark.parametrize("shape", [s for s in PAIR_SHAPES if s != (10, 10, 4)])
def test_shapes_emulated(emu_lib, shape):
    """10x10 k5; 4x4 k3 and 3x28 k6, whose guesses fall below row 0, past the
    last row and on each other; 16x8 k4, a row on the last lane of a 16-lane
    group; 5x6 k7, three planes, boards that shuffle while they are generated."""
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    R, C, k = shape
    w = batch_rng_words(range(7000, 7128))
    acc, rej, _ = _predicted(shape, w)
    assert acc > 0
    shuffled = 0
    for h in _regenerate_both_ways(emu, L, shape, w, str(shape)):
        if h["shuffle_gen"] == 0 and h["reject_gen"] == 0:
            assert (h["bp_pair_acc"], h["bp_pair_rej"]) == (acc, rej), (h, acc, rej)
        else:
            assert h["bp_pair_acc"] >= acc, (h, acc)          # a shuffled board is searched again
        shuffled += h["shuffle_gen"]
    if shape == (5, 6, 7):
        assert shuffled > 0, "5x6 k7 was meant to shuffle while generating"
    if R > 3:
        assert rej > 0
    else:
        assert rej == 0                                       # rows 1 and 2 only: every guess holds


def test_tall_board_keeps_the_old_loop_emulated(emu_lib):
    """17x7 k4 is outside bp_pair_shape: one redraw per search, no pair site."""
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    w = batch_rng_words(range(8000, 8064))
    for h in _regenerate_both_ways(emu, L, OLD_LOOP_SHAPE, w, "17x7 k4"):
        assert h["bp_pair_acc"] == 0 and h["bp_pair_rej"] == 0, h


def test_one_redraw_build_emulated():
    """The A/B side (TMG_BP_PAIR=0) computes the same and never enters the paired loop."""
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = _load("libwave_emu_bpp0.so")
    w = batch_rng_words(range(5000, 5064))
    for h in _regenerate_both_ways(emu, L, (10, 10, 4), w, "TMG_BP_PAIR=0"):
        assert h["bp_pair_acc"] == 0 and h["bp_pair_rej"] == 0, h
