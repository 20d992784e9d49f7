"""The move-level colour batch of the row-plane cascade (csrc/tmg_rp.hip,
RpBatch) on the host wave emulator: iterations served from a batch an earlier
iteration drew from, a second batch within one move, Lemire rejections inside
and just beyond the colours a move takes, rollouts with rejections injected
into later iterations, and the per-iteration draw of the TMG_RP_BATCH=0 build
— always against the oracle (oracle/tmg_oracle.c), every field."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rowplane_batch_cases import (REJECT_SHAPES, ROLLOUT_POSITIONS, WIDE_SHAPES, bookkeeping, carry_cases, draws,
                                  rebatch_cases, rejection_cases)
from rowplane_cases import FIELDS, INJECTED, K10, MOVES, SHAPES, STEPS, trace_move

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


def test_carry_emulated(emu_lib):
    """The crafted cascades, one env at a time, as seeded and with a buffered
    half-word: later iterations take their colours from the move's batch, and
    the position written back is the oracle's after an even and after an odd
    number of half-words taken from the batch's outputs."""
    from oracle import oracle as orc
    emu, L = emu_lib
    flag = set()
    for nm, b, a, w in carry_cases(orc):
        its, fb, rng = trace_move(orc, b, w, a, K10)
        carry, again = bookkeeping(draws(its))
        assert carry > 0 and again == 0, nm
        if nm.startswith("six_iterations") and "+" not in nm:
            assert len(its) == 12
        e = emu.EmuBatch(L, 10, 10, K10, 0, 30, w[None])
        o = orc.OracleBatch(10, 10, K10, 0, 30, w[None])
        e.board[:] = b
        o.board[:] = b
        idle = np.array([int(np.nonzero(~orc.effective_mask(b)[0])[0][0])], np.int32)
        e.trust = False
        e.step(idle, False)                               # the general kernel: computes the mask
        o.step(idle, False)
        _same(e, o, f"{nm}, mask step")
        e.trust = True
        emu.cover(L, True)
        e.step(np.array([a], np.int32), False)
        o.step(np.array([a], np.int32), False)
        _same(e, o, f"{nm}, move")
        assert np.array_equal(o.rng[0], rng) and np.array_equal(o.board[0], fb), nm
        hits = _hits(emu, L)
        assert hits["rp_carry"] == carry and hits["rp_rebatch"] == 0, (nm, hits)
        flag.add(int(rng[4] >> np.uint64(32)))
    assert flag == {0, 1}, "moves ending with and without a buffered half-word"
    assert L.emu_status() == 0


@pytest.mark.parametrize("shape", WIDE_SHAPES)
def test_rebatch_emulated(emu_lib, shape):
    """Striped boards whose first refill takes (nearly) a whole batch and whose
    cascade goes on: a second batch within the move, from the exact position."""
    from oracle import oracle as orc
    emu, L = emu_lib
    R, C, k = shape
    b, words, acts, w = rebatch_cases(orc, shape)
    n = w.shape[0]
    again = 0
    for i in range(n):
        ts = draws(trace_move(orc, b, w[i], int(acts[i]), k)[0])
        assert len(ts) >= 2, (shape, i)
        again += bookkeeping(ts)[1]
    assert again >= n or R * C < 128                     # 84 cells leave 44 colours of the batch: see rebatch_cases
    e = emu.EmuBatch(L, R, C, k, 0, 30, w)
    o = orc.OracleBatch(R, C, k, 0, 30, w)
    for x in (e, o):
        x.board[:] = b
        x.eff[:] = words                                  # the cached mask, as a step would have left it
    e.trust = True
    emu.cover(L, True)
    e.step(acts, False)
    o.step(acts, False)
    _same(e, o, f"{shape} move")
    hits = _hits(emu, L)
    assert hits["rp_reject"] == 0 and hits["rp_wide"] == n, (shape, hits)
    assert hits["rp_rebatch"] == again, (shape, hits)
    if R * C >= 128:
        assert hits["rp_rebatch"] > 0, (shape, hits)
    else:
        assert hits["rp_carry"] >= n, (shape, hits)
    assert L.emu_status() == 0


@pytest.mark.parametrize("shape", REJECT_SHAPES)
def test_rejection_in_carried_range_emulated(emu_lib, shape):
    """A rejected word among the colours the move's second iteration takes
    from the carried batch: serial replay from the exact position.  A rejected
    word just beyond the move's last draw: no effect at all."""
    from oracle import oracle as orc
    emu, L = emu_lib
    R, C, k = shape
    o0, inside, beyond = rejection_cases(orc, shape)
    for what, (idx, acts, w) in (("inside", inside), ("beyond", beyond)):
        n = idx.size
        e = emu.EmuBatch(L, R, C, k, 0, 30, w)
        o = orc.OracleBatch(R, C, k, 0, 30, w)
        for x in (e, o):
            x.board[:] = o0.board[idx]
            x.eff[:] = o0.eff[idx]
        e.trust = True
        emu.cover(L, True)
        e.step(acts, False)
        o.step(acts, False)
        _same(e, o, f"{shape} {what}")
        hits = _hits(emu, L)
        if what == "inside":
            assert hits["rp_reject"] >= n and hits["rp_carry"] >= n, (shape, hits)
        else:
            assert hits["rp_reject"] == 0, (shape, hits)  # and _same: the position is the oracle's
    assert L.emu_status() == 0


def _rollout(emu, L, shape, carry_expected):
    from oracle import oracle as orc
    from oracle.policy_np import sample_effective_np
    from rejection_states import words_rejecting_at
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k = shape
    n = 64
    w = batch_rng_words(range(700, 700 + n))
    e = emu.EmuBatch(L, R, C, k, 0, MOVES, w)
    o = orc.OracleBatch(R, C, k, 0, MOVES, w)
    emu.cover(L, True)
    e.reset()
    o.reset()
    A = 2 * R * C - R - C
    rs = np.random.default_rng(5)
    for t in range(STEPS):
        if shape in INJECTED and t % 5 == 1:
            ww = words_rejecting_at(o.rng, rs.integers(0, ROLLOUT_POSITIONS, n), buffered=rs.random(n) < 0.5)
            o.rng[:] = ww
            e.rng[:] = ww
        a = sample_effective_np(o.eff, A, 7, 0, t)
        e.step(a, True)
        o.step(a, True)
        _same(e, o, f"{shape} step {t}")
    assert L.emu_status() == 0
    hits = _hits(emu, L)
    assert hits["sb_lean"] > 0
    if shape in INJECTED:
        assert hits["rp_reject"] > 0, (shape, hits)
    if carry_expected:
        assert hits["rp_carry"] > 0, (shape, hits)
    else:
        assert hits["rp_carry"] == 0 and hits["rp_rebatch"] == 0, (shape, hits)


@pytest.mark.parametrize("shape", SHAPES)
def test_rollout_batch_emulated(emu_lib, shape):
    """64 envs, 40 policy-effective steps, episodes of 10 moves; on 10x10 k5
    and 5x6 k7 a Lemire rejection at draw 0-15 (half with a buffered
    half-word) before every 5th step, so that it also lands in later
    iterations of a move."""
    emu, L = emu_lib
    _rollout(emu, L, shape, True)


def test_rollout_per_iteration_build_emulated():
    """The A/B side (TMG_RP_BATCH=0: a jump-ahead batch per iteration) still
    computes the same."""
    emu, L = _load("libwave_emu_rpb0.so")
    _rollout(emu, L, (10, 10, 5), False)
