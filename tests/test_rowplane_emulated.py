"""The row-plane lean cascade (csrc/tmg_rp.hip) on the host wave emulator:
rollouts with the effective-action policy on every shape class the path
covers, hand-written boards showing one feature of the cascade each, and the
refill of more than 64 cells — always against the oracle (oracle/tmg_oracle.c),
every field, every step."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rowplane_cases import (FEATURES, FIELDS, INJECTED, K10, MOVES, SHAPES, STEPS, crafted, stream_words, trace_move)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    return emu, emu.load()


def _same(e, o, what):
    for f in FIELDS:
        got, want = getattr(e, f), getattr(o, f)
        if not np.array_equal(got, want):
            n = got.shape[0]
            bad = np.nonzero((got.reshape(n, -1) != want.reshape(n, -1)).any(axis=1))[0]
            raise AssertionError(f"{what}: {f} differs in {bad.size} envs, first {bad[:5]}")


@pytest.mark.parametrize("shape", SHAPES)
def test_rollout_emulated(emu_lib, shape):
    """64 envs, 40 policy-effective steps, episodes of 10 moves (inline
    autoreset every 10th step); on 10x10 k5 and 5x6 k7 a Lemire rejection in
    the refill range (draws 0-7, half with a buffered half-word) before every
    5th step.  The new branches the oracle rollout reaches are counted."""
    from oracle import oracle as orc
    from oracle.policy_np import sample_effective_np
    from rejection_states import words_rejecting_at
    from tile_match_gym_amd._native import COVER_NAMES
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    R, C, k = shape
    n = 64
    w = batch_rng_words(range(500, 500 + n))
    e = emu.EmuBatch(L, R, C, k, 0, MOVES, w)
    o = orc.OracleBatch(R, C, k, 0, MOVES, w)
    emu.cover(L, True)
    e.reset()
    o.reset()
    A = 2 * R * C - R - C
    rs = np.random.default_rng(3)
    for t in range(STEPS):
        if shape in INJECTED and t % 5 == 1:
            ww = words_rejecting_at(o.rng, rs.integers(0, 8, n), buffered=rs.random(n) < 0.5)
            o.rng[:] = ww
            e.rng[:] = ww
        a = sample_effective_np(o.eff, A, 7, 0, t)
        e.step(a, True)
        o.step(a, True)
        _same(e, o, f"{shape} step {t}")
    assert L.emu_status() == 0
    hits = dict(zip(COVER_NAMES, emu.cover(L, True)))
    want = ["sb_lean", "rp_passes", "rp_perp"]
    if R >= 4:
        want.append("rp_vlong")
    if shape in INJECTED:
        want.append("rp_reject")
    missing = [s for s in want if hits[s] == 0]
    assert not missing, (shape, {s: int(hits[s]) for s in want})


def _crafted_batch(emu, L, orc):
    cases = crafted()
    names = sorted(cases)
    n = len(names)
    w = np.stack([stream_words(cases[nm][2]) for nm in names])
    boards = np.stack([np.stack([cases[nm][0], np.ones_like(cases[nm][0])]) for nm in names]).astype(np.int8)
    acts = np.array([cases[nm][1] for nm in names], np.int32)
    return names, n, w, boards, acts


def test_crafted_boards_emulated(emu_lib):
    """Each hand-written board: one untrusted step with an ineffective action
    (the general kernel: it only computes the mask), then the move on the
    row-plane path.  The feature is asserted on the oracle's own lines."""
    from oracle import oracle as orc
    from tile_match_gym_amd._native import COVER_NAMES
    emu, L = emu_lib
    names, n, w, boards, acts = _crafted_batch(emu, L, orc)
    for i, nm in enumerate(names):
        assert orc.get_colour_lines(boards[i], K10, 0) == [], nm
        its, fb, rng = trace_move(orc, boards[i], w[i], int(acts[i]), K10)
        mb, mrng, res, err = orc.move(boards[i], w[i], int(acts[i]), K10, 0)
        assert err == 0 and np.array_equal(fb, mb) and np.array_equal(rng, mrng), nm
        assert FEATURES[nm][0](its), f"{nm}: the oracle's cascade does not show the feature"
        assert res[0] == sum(len({c for ln in lines for c in ln}) for lines in its) > 0, nm
    e = emu.EmuBatch(L, 10, 10, K10, 0, 30, w)
    o = orc.OracleBatch(10, 10, K10, 0, 30, w)
    e.board[:] = boards
    o.board[:] = boards
    idle = np.array([int(np.nonzero(~orc.effective_mask(b)[0])[0][0]) for b in boards], np.int32)
    e.trust = False
    e.step(idle, False)
    o.step(idle, False)
    _same(e, o, "crafted, mask step")
    assert (o.reward == 0).all()
    e.trust = True
    for i, nm in enumerate(names):                    # one env at a time: the cover counts are the case's own
        emu.cover(L, True)
        e1 = emu.EmuBatch(L, 10, 10, K10, 0, 30, e.rng[i:i + 1])
        for f in ("board", "timer", "eff"):
            getattr(e1, f)[:] = getattr(e, f)[i:i + 1]
        e1.trust = True
        e1.step(acts[i:i + 1], False)
        hits = dict(zip(COVER_NAMES, emu.cover(L, True)))
        assert hits["sb_lean"] > 0, nm
        site = FEATURES[nm][1]
        if site:
            assert hits[site] > 0, (nm, site)
        if nm == "six_iterations":
            assert hits["sb_lean"] >= 6
    e.step(acts, False)
    o.step(acts, False)
    _same(e, o, "crafted, move")
    assert (o.reward >= 3).all()
    assert L.emu_status() == 0


@pytest.mark.parametrize("shape", [(16, 8, 4), (3, 28, 6), (16, 8, 5)])
def test_wide_refill_emulated(emu_lib, shape):
    """A refill of more than 64 cells (two ballots per plane, slices past bit
    64): every column one colour from top to bottom, so the first cascade
    iteration clears (nearly) the whole board — a hand-edited board with its
    cached mask written beside it."""
    from oracle import oracle as orc
    from rejection_states import words_rejecting_at
    from tile_match_gym_amd._native import COVER_NAMES
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    R, C, k = shape
    n = 8
    w = batch_rng_words(range(40, 40 + n))
    if k == 5:                                         # a rejection far into the wide refill, half with a buffered half-word
        w = words_rejecting_at(w, np.arange(n) * 9 + 40, buffered=np.arange(n) % 2 == 1)
    col = np.tile((1 + np.arange(C) % 2).astype(np.int8), (R, 1))
    b = np.stack([col, np.ones_like(col)])
    boards = np.stack([b] * n)
    e = emu.EmuBatch(L, R, C, k, 0, 30, w)
    o = orc.OracleBatch(R, C, k, 0, 30, w)
    e.board[:] = boards
    o.board[:] = boards
    mask = orc.effective_mask(b)[0]                    # lines everywhere: every action is effective
    A = mask.size
    words = np.packbits(np.pad(mask, (0, -A % 64)).reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()
    e.eff[:] = words                                   # the cached mask, as a step would have left it
    o.eff[:] = words
    emu.cover(L, True)
    e.trust = True
    acts = np.nonzero(mask)[0][np.arange(n) * 3 % int(mask.sum())].astype(np.int32)
    e.step(acts, False)
    o.step(acts, False)
    _same(e, o, f"{shape} move")
    assert (o.reward > 64).all()
    hits = dict(zip(COVER_NAMES, emu.cover(L, True)))
    assert hits["rp_reject" if k == 5 else "rp_wide"] > 0       # the replay comes before the wide slices
    assert L.emu_status() == 0
