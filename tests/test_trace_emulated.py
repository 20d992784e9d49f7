"""tmg_trace on the host wave emulator (CPU): the trace kernels of
csrc/tmg_trace.hip and their spill pass, against the stage-by-stage walk of the
oracle's primitives (tests/trace_cases.py oracle_trace).  Everything is compared
as integers and bytes; nothing here has a tolerance.  The cases are those of
tests/test_gpu_trace.py that need no device (the checks themselves are shared:
trace_cases.check_*)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import peek_cases
import trace_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


class EmuDev:
    """trace_cases' `dev` on the emulator."""

    def __init__(self, emu, L):
        self.emu, self.L = emu, L

    def run(self, shape, board, rng, eff, trust_eff, actions, stage_mask, max_frames, stop, bufs, lead):
        R, C, k, sm = shape
        out = {f: a[lead:] for f, a in bufs.items()}
        self.emu.trace(self.L, R, C, k, sm, board, rng, eff, trust_eff, actions, stage_mask, max_frames, stop, out=out)

    def status_clear(self, shape=None):
        return self.L.emu_status_clear()

    def spills(self, shape=None):
        return self.L.emu_spills()

    def step(self, shape, board, rng, actions):
        R, C, k, sm = shape
        e = self.emu.EmuBatch(self.L, R, C, k, sm, 1 << 20, rng)
        e.board[:] = board
        e.step(actions, autoreset=False)
        return e.board, e.rng, e.reward, e.n_new, e.n_act, e.flags


@pytest.fixture(scope="module")
def dev():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    L = emu.load()
    L.emu_status_clear()
    return EmuDev(emu, L)


@pytest.mark.parametrize("shape", tc.FIELD_SHAPES + tc.EMU_LIMIT_SHAPES, ids=tc.case_id)
def test_trace_vs_oracle(dev, shape):
    tc.check_fields(dev, shape)


@pytest.mark.parametrize("shape", tc.STEP_SHAPES, ids=tc.case_id)
def test_trace_last_frame_is_the_stepped_board(dev, shape):
    tc.check_step(dev, shape)


@pytest.mark.parametrize("max_frames", tc.CUT_FRAMES)
@pytest.mark.parametrize("stage_mask", tc.CUT_MASKS, ids=lambda m: f"mask{m:#x}")
@pytest.mark.parametrize("shape", tc.CUT_SHAPES, ids=tc.case_id)
def test_trace_masks_and_cuts(dev, shape, stage_mask, max_frames):
    tc.check_cut(dev, shape, stage_mask, max_frames)


@pytest.mark.parametrize("shape,mode,many", peek_cases.spill_params(device=False))
def test_trace_untrusted_and_spill(dev, shape, mode, many):
    tc.check_adversarial(dev, shape, mode, many)


@pytest.mark.parametrize("seqs", tc.EXTENT_SEQS)
@pytest.mark.parametrize("n", tc.EXTENT_N)
@pytest.mark.parametrize("shape", [tc.EXTENT_SHAPE, tc.EXTENT_ODD_SHAPE], ids=tc.case_id)
def test_trace_extent(dev, shape, n, seqs):
    tc.check_extent(dev, shape, n, seqs)


def test_trace_refusals_and_noops(dev):
    """The argument checks the emulator's entry point shares with the library:
    each refusal of the list, and n == 0."""
    L = dev.L
    shape = (10, 10, 4, 14)
    R, C, k, sm = shape
    board, rng, acts, want = tc.field_case(shape)
    board, rng, acts = (np.ascontiguousarray(x).copy() for x in (board, rng, acts))
    eff = tc.masks_of(board)
    n, Q, F = board.shape[0], acts.shape[0], 4
    rew = np.zeros((Q, n), np.int32)
    fr = np.zeros(Q * n * F * 2 * R * C + 4, np.int8)
    fr = fr[(-fr.ctypes.data) % 4:]

    def call(n=n, board=board, rng=rng, eff=eff, trust=1, q=Q, acts=acts, mask=tc.ALL_STAGES, F=F, frames=None):
        p = lambda a: None if a is None else a.ctypes.data          # noqa: E731
        return L.emu_trace(R, C, k, sm, n, p(board), p(rng), p(eff), trust, q, p(acts), mask, F, 0, p(frames), None,
                           None, None, p(rew), None, None, None, None)

    assert call() == 0
    assert np.array_equal(rew, want["reward"])
    assert call(n=-1) == -2 and call(q=0) == -2 and call(F=0) == -2
    assert call(mask=0) == -2 and call(mask=1) == -2 and call(mask=1 << 7) == -2 and call(mask=tc.ALL_STAGES | 0x100) == -2
    assert call(n=2 ** 26 - 8, q=2) == -2
    assert call(board=None) == -1 and call(rng=None) == -1 and call(acts=None) == -1
    assert call(eff=None) == -1 and call(eff=None, trust=0) == 0
    assert call(frames=fr[2:]) == -2 and call(frames=fr) == 0
    rew[:] = -7
    assert call(n=0, board=None, rng=None, acts=None, eff=None) == 0 and (rew == -7).all()
    dev.status_clear()
