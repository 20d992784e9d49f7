"""The lean step's three-row gravity shift (csrc/tmg_rp.hip, rp_move,
TMG_RP_VSHIFT) and its effective-mask scan on the cascade's own planes
(rp_scan, TMG_RP_SCAN2) on the host wave emulator, against the oracle
(oracle/tmg_oracle.c): every field, every step.  Boards picked with the
oracle's trace for one feature of the gravity each, rollouts on every shape
class of the two paths, each cached mask beside a fresh scan of the same board,
and the A/B side of each macro."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lean_levers_cases import (CASE_SHAPES, CASES, FIELDS, GRAVITY_SHAPES, MOVES, PREDICATES, SCAN_NEW_PATH, SCAN_SHAPES,
                               SITES, STEPS, case_arrays, case_predicates)
from rowplane_cases import trace_move

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")
ROLLOUT_SHAPES = GRAVITY_SHAPES + [s for s in SCAN_SHAPES if s not in GRAVITY_SHAPES]


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


def _fresh_mask(L, e):
    out = np.zeros_like(e.eff)
    L.emu_effective(e.R, e.C, e.k, 0, e.n, e.board.ctypes.data, out.ctypes.data)
    return out


def _rollout(emu, L, shape, n=32, steps=STEPS, seed0=900):
    """Policy-effective steps, episodes of MOVES moves with the inline
    autoreset; every field against the oracle after every step, and the cached
    mask beside a fresh scan (tmg_effective's kernel) of the board it belongs
    to, both against the oracle's.  Returns the cover counts."""
    from oracle import oracle as orc
    from oracle.policy_np import sample_effective_np
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k = shape
    w = batch_rng_words(range(seed0, seed0 + n))
    e = emu.EmuBatch(L, R, C, k, 0, MOVES, w)
    o = orc.OracleBatch(R, C, k, 0, MOVES, w)
    emu.cover(L, True)
    e.reset()
    o.reset()
    A = 2 * R * C - R - C
    for t in range(steps):
        a = sample_effective_np(o.eff, A, 5, 0, t)
        e.step(a, True)
        o.step(a, True)
        _same(e, o, f"{shape} step {t}")
        assert np.array_equal(_fresh_mask(L, e), o.eff), f"{shape} step {t}: fresh scan"
    assert L.emu_status() == 0
    return _hits(emu, L)


@pytest.mark.parametrize("shape", ROLLOUT_SHAPES)
def test_rollout_emulated(emu_lib, shape):
    emu, L = emu_lib
    h = _rollout(emu, L, shape)
    assert h["sb_lean"] > 0 and h["rp_vshift"] > 0 and h["rp_passes"] >= h["rp_vshift"], (shape, h)
    assert (h["rp_scan2"] > 0) == (shape[2] in SCAN_NEW_PATH), (shape, h)
    if shape == (10, 10, 4):
        assert h["rp_vmore"] > 0, h


def test_new_scan_path_shapes():
    """The shapes meant for the new scan are those whose colour value needs a
    plane more than colour - 1, the others keep the old one."""
    planes = lambda n: max(1, int(n - 1).bit_length())       # noqa: E731
    for R, C, k in SCAN_SHAPES:
        assert (planes(k + 1) > planes(k)) == (k in SCAN_NEW_PATH), k
    ks = {k for _, _, k in SCAN_SHAPES}
    assert {2, 4, 8, 3, 5} <= ks
    assert {3, 28} <= {C for _, C, _ in SCAN_SHAPES} and 3 in {R for R, _, _ in SCAN_SHAPES}


def _case_batch(shape):
    names = sorted(nm for nm in CASES if CASES[nm][1] == shape)
    arr = [case_arrays(nm) for nm in names]
    boards = np.stack([a[2] for a in arr])
    acts = np.array([a[3] for a in arr], np.int32)
    w = np.stack([a[4] for a in arr])
    return names, boards, acts, w


@pytest.mark.parametrize("shape", CASE_SHAPES)
def test_gravity_cases_emulated(emu_lib, shape):
    """Each board: the feature asserted on the oracle's own trace of the move,
    one untrusted step with an ineffective action (it only computes the mask),
    then the move on the row-plane path: alone for the case's own cover
    counts, and in one batch against the oracle."""
    from oracle import oracle as orc
    emu, L = emu_lib
    R, C, k = shape
    names, boards, acts, w = _case_batch(shape)
    for i, nm in enumerate(names):
        assert orc.get_colour_lines(boards[i], k, 0) == [], nm
        its, fb, rng = trace_move(orc, boards[i], w[i], int(acts[i]), k)
        mb, mrng, res, err = orc.move(boards[i], w[i], int(acts[i]), k, 0)
        assert err == 0 and np.array_equal(fb, mb) and np.array_equal(rng, mrng), nm
        for pred in case_predicates(nm):
            assert PREDICATES[pred](its, R), f"{nm}: the oracle's cascade does not show {pred}"
    e = emu.EmuBatch(L, R, C, k, 0, 30, w)
    o = orc.OracleBatch(R, C, k, 0, 30, w)
    e.board[:] = boards
    o.board[:] = boards
    idle = np.array([int(np.nonzero(~orc.effective_mask(b)[0])[0][0]) for b in boards], np.int32)
    e.trust = False
    e.step(idle, False)
    o.step(idle, False)
    _same(e, o, f"{shape} cases, mask step")
    assert (o.reward == 0).all()
    for i, nm in enumerate(names):
        emu.cover(L, True)
        e1 = emu.EmuBatch(L, R, C, k, 0, 30, e.rng[i:i + 1])
        for f in ("board", "timer", "eff"):
            getattr(e1, f)[:] = getattr(e, f)[i:i + 1]
        e1.trust = True
        e1.step(acts[i:i + 1], False)
        h = _hits(emu, L)
        assert h["rp_vshift"] > 0 and h["rp_passes"] >= h["rp_vshift"], (nm, h)
        for site in {SITES[pred] for pred in case_predicates(nm)} - {None}:
            assert h[site] > 0, (nm, site, h)
    e.trust = True
    e.step(acts, False)
    o.step(acts, False)
    _same(e, o, f"{shape} cases, move")
    assert (o.reward >= 3).all()
    assert L.emu_status() == 0


@pytest.mark.parametrize("lib,off", [("libwave_emu_vs0.so", "rp_vshift"), ("libwave_emu_sc0.so", "rp_scan2")])
def test_ab_side_emulated(lib, off):
    """TMG_RP_VSHIFT=0 / TMG_RP_SCAN2=0: the parent's code computes the same;
    the one-row passes never count the three-row site and still count
    rp_passes; the scan on colour-value planes never counts rp_scan2."""
    emu, L = _load(lib)
    for shape in ((10, 10, 4), (6, 6, 8)):
        h = _rollout(emu, L, shape, n=16, steps=20)
        assert h["rp_passes"] > 0, h
        assert h[off] == 0, h
        if off == "rp_vshift":
            assert h["rp_vmore"] == 0 and h["rp_scan2"] > 0, h
        else:
            assert h["rp_vshift"] > 0, h
