"""bp_generate's paired redraw loop (csrc/tmg_board.hip, bp_redraw_pairs) on
the MI355X, against the oracle (oracle/tmg_oracle.c): the shapes of
tests/test_bp_pair_emulated.py at 2048 envs through reset_kernel (bare and
masked) and through the lean step kernel's inline autoreset in the three
autoreset modes, on the product library and on the TMG_COVER build, whose
counts show the second redraws accepted and rejected.  The library pairs
redraws in the kernels specialised for one shape (10x10 k4 here); the generic
kernels keep the one-redraw loop (csrc/tmg_board.hip, TMG_BP_PAIR), so the
other shapes must compute the same and count no pair site: their paired loop
runs on the host wave emulator, which builds it for every shape.  Half of the
streams start with a buffered half-word; where k is no power of two a quarter
hold a Lemire-rejected word among the first colours."""
import functools
import os

import numpy as np
import pytest
import torch

from bp_pair_cases import OLD_LOOP_SHAPE, PAIR_SHAPES
from deep_rollouts import COVER_LIB
from oracle import oracle as orc
from rejection_states import words_rejecting_at
from rowplane_cases import FIELDS
from vector_ref import reset_subset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENVS = 2048
MOVES = 2                        # an episode ends, and its board is regenerated, every second step
STEPS = 5
SHAPES = PAIR_SHAPES + [OLD_LOOP_SHAPE]
PAIRED_ON_DEVICE = [(10, 10, 4)]  # the shapes of SHAPES with a kernel of their own (tmg_dispatch.h is_shape)
LIBS = ["product", "cover"]
MODES = ["none", "same_step", "next_step"]


def _lib(lib):
    if lib == "product":
        return None
    assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
    return COVER_LIB


def _host(env, f):
    if f == "rng":
        return env.rng_words()
    v = getattr(env, f).cpu().numpy()
    return v.view(np.uint64) if f == "eff" else v


def _same(env, o, what, fields=FIELDS):
    n = env.num_envs
    for f in fields:
        got, want = _host(env, f), getattr(o, f)
        if not np.array_equal(got, want):
            bad = np.nonzero((got.reshape(n, -1) != want.reshape(n, -1)).any(axis=1))[0]
            raise AssertionError(f"{what}: {f} differs in {bad.size} envs, first {bad[:5]}")


def _set_rng(env, w):
    env.rng.copy_(torch.from_numpy(np.array(w).view(np.int64)).to(DEV))


def _counts(env):
    from tile_match_gym_amd import _native
    c = env.ctx.cover(True)
    return {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}


def _base(shape):
    return 700_000 + 10_000 * SHAPES.index(shape)


@functools.lru_cache(maxsize=None)
def _start_words(shape):
    """The streams every case of a shape starts from (computed once, read only)."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k = shape
    rs = np.random.default_rng(_base(shape))
    w = batch_rng_words(range(_base(shape), _base(shape) + ENVS))
    buf = rs.random(ENVS) < 0.5
    w[buf, 4] = (np.uint64(1) << np.uint64(32)) | rs.integers(0, 2 ** 32, int(buf.sum()), dtype=np.uint64)
    if k & (k - 1):
        q = ENVS // 4
        w[:q] = words_rejecting_at(w[:q], rs.integers(0, 3 * R * C, q), buffered=buf[:q])
    w.setflags(write=False)
    return w


def _check_sites(shape, counts, what, injected=True):
    R, C, k = shape
    if shape in PAIRED_ON_DEVICE:
        assert counts["bp_pair_acc"] > 0 and counts["bp_pair_rej"] > 0, (what, counts)
    else:
        assert counts["bp_pair_acc"] == 0 and counts["bp_pair_rej"] == 0, (what, counts)
    if injected and k & (k - 1):
        assert counts["reject_gen"] > 0, (what, counts)


@functools.lru_cache(maxsize=None)
def _reset_reference(shape):
    """(state after the bare reset, the mask, state after the masked reset that follows)."""
    R, C, k = shape
    o = orc.OracleBatch(R, C, k, 0, MOVES, _start_words(shape).copy(), threads=16)
    o.reset()
    first = {f: getattr(o, f).copy() for f in ("board", "rng", "timer", "eff")}
    mask = np.random.default_rng(_base(shape) + 1).random(ENVS) < 0.5
    reset_subset(o, np.nonzero(mask)[0])
    return first, mask, o


class _State:
    def __init__(self, d):
        self.__dict__.update(d)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_reset_kernel(shape, lib):
    """reset() of every env, then reset(env_mask=...) of half of them from where their streams stand."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    path = _lib(lib)
    first, mask, o = _reset_reference(shape)
    env = TileMatchVecEnv(ENVS, R, C, k, MOVES, [], [], seeds=range(ENVS), device=DEV, lib_path=path)
    _set_rng(env, _start_words(shape))
    if path:
        env.ctx.cover(True)
    env.reset()
    _same(env, _State(first), f"{shape} reset", ("board", "rng", "timer", "eff"))
    if path:
        _check_sites(shape, _counts(env), "bare reset")
    env.reset(env_mask=mask.astype(np.uint8))
    _same(env, o, f"{shape} masked reset", ("board", "rng", "timer", "eff"))
    if path:
        _check_sites(shape, _counts(env), "masked reset", injected=False)
    assert env.status() == 0
    env.close()


@functools.lru_cache(maxsize=None)
def _step_reference(shape, mode):
    """Per step: (actions, expected fields).  Uniform actions: an ineffective
    move counts too, so every env's episode ends on every second step."""
    R, C, k = shape
    A = 2 * R * C - R - C
    o = orc.OracleBatch(R, C, k, 0, MOVES, _start_words(shape).copy(), threads=16)
    o.reset()
    rs = np.random.default_rng(_base(shape) + 2)
    pending = np.zeros(ENVS, bool)
    out = []
    for t in range(STEPS):
        a = rs.integers(0, A, ENVS).astype(np.int32)
        resets = None
        if mode == "same_step":
            o.step(a, autoreset=True)
        elif mode == "next_step":
            idx = np.nonzero(pending)[0]
            o.step(np.where(pending, 0, a).astype(np.int32), autoreset=False)
            reset_subset(o, idx)
            o.reward[idx] = 0
            o.flags[idx] = 8                                  # FL_RESET: regenerated instead of stepped
            pending = (o.flags & 1) != 0
        else:
            o.step(a, autoreset=False)
            resets = (o.flags & 1) != 0                       # mode none: the caller resets what ended
        exp = {f: getattr(o, f).copy() for f in FIELDS}
        after = None
        if resets is not None and resets.any():
            reset_subset(o, np.nonzero(resets)[0])
            after = {f: getattr(o, f).copy() for f in ("board", "rng", "timer", "eff")}
        out.append((a, exp, resets, after))
    return out


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_step_autoreset(shape, mode, lib):
    """Five steps of episodes of two moves: same-step and next-step autoreset
    regenerate inside the lean step kernel; with none the ended envs go
    through a masked reset, as a caller without autoreset does it."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    path = _lib(lib)
    env = TileMatchVecEnv(ENVS, R, C, k, MOVES, [], [], seeds=range(ENVS), device=DEV, lib_path=path,
                          autoreset=mode != "none")
    if mode == "next_step":
        env.set_step_outputs("next_step")
    _set_rng(env, _start_words(shape))
    env.reset()
    if path:
        env.ctx.cover(True)
    for t, (a, exp, resets, after) in enumerate(_step_reference(shape, mode)):
        env.step_raw(torch.from_numpy(a).to(DEV))
        env.join()
        _same(env, _State(exp), f"{shape} {mode} step {t}")
        if after is not None:
            env.reset(env_mask=resets.astype(np.uint8))
            _same(env, _State(after), f"{shape} {mode} reset after step {t}", ("board", "rng", "timer", "eff"))
    assert env.status() == 0
    if path:
        _check_sites(shape, _counts(env), f"{mode} steps", injected=False)   # the crafted words went at the reset
    env.close()
