"""The fused step outputs of tmg_plan_config on the host wave emulator (CPU):
the schedule of tests/fused_cases.py over every kernel family and autoreset
mode, and spilled steps that end an episode — the twins of
tests/test_gpu_fused.py, which judges the device's code generation."""
import os
import subprocess
import sys

import pytest

import fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")
N = 11
# 4x29 k4 redraws for ~0.3 s of host time per board (a line-free one is rare): fewer envs, the same schedule
N_OF = {(4, 29, 4, 0): 7}


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    return emu, emu.load()


@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.case_id)
def test_fused_outputs_emulated(emu_lib, shape, mode):
    """Every output after every step equals the oracle's (fused_cases.drive):
    staggered 4-move episodes, effective / uniform / in-kernel policy actions,
    two untrusted steps after a hand edit, final boards over all rows."""
    emu, L = emu_lib
    be = fc.EmuBackend(emu, L, shape, fc.M, N_OF.get(shape, N), mode)
    try:
        fc.drive(be, fc.oracle_for(be, shape, fc.M), mode)
    finally:
        L.emu_status_clear()            # mode none leaves the caller's bit: not the next test's business


@pytest.mark.parametrize("timers", fc.SPILL_TIMERS)
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("shape", fc.SPILL_SHAPES, ids=fc.case_id)
def test_fused_outputs_of_spilled_steps_emulated(emu_lib, shape, mode, timers):
    """Every env's first step is re-run by spill_kernel, which then writes all
    of its outputs (junk before); with the timers at M - 1 it ends the episode."""
    emu, L = emu_lib
    be = fc.EmuBackend(emu, L, shape, fc.SPILL_M, 4 * len(fc.SPILL_BOARDS), mode, seed=300)
    try:
        fc.drive_spill(be, fc.oracle_for(be, shape, fc.SPILL_M), mode, timers)
    finally:
        L.emu_status_clear()
