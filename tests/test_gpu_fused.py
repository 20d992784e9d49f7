"""The fused step outputs of tmg_plan_config on the device, for every
step_kernel / reset_kernel instantiation and spill_kernel: terminated / info
bytes, action-mask bytes, moves left, same-step final boards, int32 boards and
float32 one-hot planes against the oracle after every step, over all rows
(tests/fused_cases.py holds the shapes, the schedule and the comparisons;
tests/test_fused_emulated.py plays the same on the host wave emulator)."""
import pytest

import fused_cases as fc

pytestmark = pytest.mark.gpu


def _batch(shape):
    """(envs, groups): group bounds 0/67/135/203, or 0/33/67 where the oracle is slow."""
    R, C = shape[:2]
    return (67, 2) if shape in fc.SLOW or R * C > 128 else (203, 3)


@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.case_id)
def test_fused_outputs_gpu(shape, mode):
    """fused_cases.drive on TileMatchVecEnv: staggered 4-move episodes on env
    groups, effective / uniform / in-kernel policy actions, two untrusted steps
    after a hand edit; every output, one-hot planes included, equals the
    oracle's after every step, and final_board changes in no other row."""
    n, groups = _batch(shape)
    be = fc.DeviceBackend(shape, fc.M, n, mode, groups)
    fc.drive(be, fc.oracle_for(be, shape, fc.M, threads=16), mode)


@pytest.mark.parametrize("timers", fc.SPILL_TIMERS)
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("shape", fc.SPILL_SHAPES, ids=fc.case_id)
def test_fused_outputs_of_spilled_steps_gpu(shape, mode, timers):
    """Adversarial boards that all outgrow the LDS lists on their first step:
    spill_kernel writes every output of that step (junk before), and with the
    timers at M - 1 the spilled step ends the episode (same-step final boards,
    next-step deferred resets)."""
    be = fc.DeviceBackend(shape, fc.SPILL_M, 4 * len(fc.SPILL_BOARDS), mode, groups=2, seed=300)
    fc.drive_spill(be, fc.oracle_for(be, shape, fc.SPILL_M, threads=16), mode, timers)
