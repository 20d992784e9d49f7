"""The extent of every entry point on the MI355X: a call on n rows writes rows
0..n-1 of each of its arrays and nothing else, at n = 1, 3, 9 and 65, where
most of a padded grid, of a wave of several envs or of a block is idle, and at
the lane kernel's sizes.  Every array of every call, inputs included, sits
between guard rows of 0x5A bytes (tests/extent_cases.py Band) and the C ABI is
driven with pointers into them (_native.Context / _native.Plan), never through
TileMatchVecEnv, whose tensors are exactly n rows inside torch's allocator.
After each call the rows below n are compared with the oracle as the parity
and fused tests do, every guard byte must be intact and every input unchanged.

tmg_seed (tests/test_gpu_seed.py) and tmg_expand (tests/test_gpu_expand.py)
have this check of their own.  Only stores show here; the loads are
tools/wave_emu/extent_asan.cpp's, on the host (tests/test_extent_host.py)."""
import pytest
import torch

import extent_cases as ec

pytestmark = pytest.mark.gpu

CALLS = [pytest.param(s, n, g, id=f"{ec.case_id(s)}-n{n}-{g}") for s, n in ec.CASES for g in ec.GROUPS
         if not (g == "plan" and n < 2)]          # a plan of an empty group, a group of one and the rest needs 2 rows


def test_band_guards_see_one_byte():
    """A torch write of one byte into either guard makes guards_intact() false;
    writes to the payload do not."""
    for row_shape, dtype in (((2, 7, 9), torch.int8), ((), torch.uint8), ((5,), torch.int64), ((4, 3, 5), torch.float32)):
        b = ec.Band(9, row_shape, dtype)
        lo, hi = ec.FRONT * b.row_bytes, (ec.FRONT + 9) * b.row_bytes
        assert b.raw.numel() == (ec.FRONT + 9 + ec.BACK) * b.row_bytes and bool((b.raw == ec.FILL).all())
        assert b.data_ptr() == b.raw.data_ptr() + lo and b.guards_intact()
        b.view.zero_()
        assert b.guards_intact() and not b.payload_bytes().any()
        for at in (0, lo - 1, hi, b.raw.numel() - 1):
            b.raw[at] = 0
            assert not b.guards_intact(), (row_shape, at)
            b.raw[at] = ec.FILL
            assert b.guards_intact()
        for at in (lo, hi - 1):
            b.raw[at] = 1
            assert b.guards_intact()


@pytest.mark.parametrize("shape,n,group", CALLS)
def test_extent(shape, n, group):
    ec.RUN[group](shape, n)


@pytest.mark.parametrize("shape,n", ec.LANE_CASES, ids=lambda v: ec.case_id(v) if isinstance(v, tuple) else f"n{v}")
def test_extent_lane_policy(shape, n):
    ec.run_lane(shape, n)


def test_extent_lane_given_actions():
    ec.run_lane_given((10, 10, 4, 0), ec.LANE_MIN + 1)


@pytest.mark.parametrize("call", ec.SPILL_CALLS)
@pytest.mark.parametrize("shape", ec.SPILL_SHAPES, ids=ec.case_id)
def test_extent_spill(shape, call):
    ec.run_spill(shape, call)
