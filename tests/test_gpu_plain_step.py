"""The plain c2 step kernel (plain_step_kernel, csrc/tmg_board.hip) on the
MI355X against the oracle: the schedule of tests/plain_step_cases.py, every
field after every step, in each autoreset mode at n = 1, 3, 9, 65, through a
one-group tmg_plan (the call bench.py's flagship line makes).

Every array of every case sits between guard rows (tests/extent_cases.py's
Band): the exit's and the write-back's stores address an env by 32-bit byte
offsets from the array bases, and nothing outside rows 0..n-1 may be written.

The TMG_COVER build shows which kernel ran: the plain calls count plain_exit /
plain_step; with a fused output attached (moves_left) the same schedule gives
the same results and counts neither, only step_kernel<..., kFixC2>'s sites."""
import os

import numpy as np
import pytest
import torch

import plain_step_cases as pc
from deep_rollouts import COVER_LIB
from extent_cases import Bands, stream

pytestmark = pytest.mark.gpu


class _Device:
    def __init__(self, n, mode, fused=False, lib_path=None):
        from tile_match_gym_amd import _native
        R, C, k, sm = pc.SHAPE
        self.n = n
        self.ctx = _native.Context(0, R, C, k, sm, pc.MOVES, lib_path=lib_path)
        assert self.ctx.num_actions == pc.A and self.ctx.mask_words == 3
        b = self.b = Bands()
        b.add("board", n, (2, R, C), torch.int8)
        b.add("rng", n, (5,), torch.int64)
        b.add("eff", n, (3,), torch.int64)
        for f in ("timer", "actions", "reward", "n_new", "n_act"):
            b.add(f, n, (), torch.int32)
        b.add("flags", n, (), torch.uint8)
        b.add("moves_left", n, (), torch.int64)
        self.plan = _native.Plan(self.ctx, n, *b.ptrs("board", "rng", "timer", "reward", "n_new", "n_act", "flags", "eff"),
                                 [0, n], [0])
        self.plan.config(mode, moves_left=b.ptr("moves_left") if fused else None)
        self.t = 0
        if lib_path:
            self.ctx.cover(True)

    def load(self, o):
        for f in ("board", "rng", "timer", "eff"):
            self.b[f].put(getattr(o, f))

    def step(self, a, mode, fused):
        self.b["actions"].put(a)
        self.before = self.b.snapshot("actions")
        self.plan.step(self.b.ptr("actions"), self.t, 1, stream())
        self.plan.join(stream())
        self.t += 1
        torch.cuda.synchronize()

    def get(self, f):
        v = self.b[f].host()
        return v.view(np.uint64) if f in ("rng", "eff") else v

    def set_timer(self, row, value):
        t = self.b["timer"].host().copy()
        t[row] = value
        self.b["timer"].put(t)

    def after_step(self, what):
        self.b.check(what, self.before)

    def counts(self):
        from tile_match_gym_amd import _native
        c = self.ctx.cover(True)
        return {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}

    def close(self):
        self.plan.close()
        self.ctx.close()


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("n", pc.SIZES)
def test_plain_step_vs_oracle(n, mode):
    """Product library, arrays between guard rows."""
    be = _Device(n, mode)
    total = pc.drive(be, n, mode)
    pc.check_census(total, n, mode)
    assert be.ctx.status(clear=True) == (pc.STATUS_CALLER if total["bad_low"] + total["bad_high"] or mode == "none"
                                         else 0)
    assert (be.b["moves_left"].raw == 0x5A).all().item(), "no fused output was attached"
    be.close()


@pytest.mark.parametrize("mode", pc.MODES)
def test_plain_sites_taken(mode):
    """TMG_COVER build: every wave of the plain calls counts one of the plain kernel's two sites."""
    assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
    n = 65
    be = _Device(n, mode, lib_path=COVER_LIB)
    total = pc.drive(be, n, mode)
    c = be.counts()
    assert c["plain_exit"] + c["plain_step"] == n * pc.STEPS, (c, total)
    assert c["plain_exit"] >= total["exit_last"], (c, total)
    assert c["plain_step"] >= total["last_move"] + total["bad_low"] + total["bad_high"], (c, total)
    be.close()


@pytest.mark.parametrize("mode", pc.MODES)
def test_fused_output_keeps_the_old_kernel(mode):
    """TMG_COVER build, moves_left attached: the same results, none of the plain kernel's sites."""
    assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
    n = 9
    be = _Device(n, mode, fused=True, lib_path=COVER_LIB)
    pc.drive(be, n, mode, fused=True)
    c = be.counts()
    assert c["plain_exit"] == 0 and c["plain_step"] == 0, c
    assert c["sb_lean"] > 0, c
    be.close()
