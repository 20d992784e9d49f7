"""The redraw round of bp_redraw_pairs (csrc/tmg_board.hip, TMG_BP_ROUND) on the
MI355X, against the oracle (oracle/tmg_oracle.c), on the product library
(which leaves the round's parts off: DESIGN.md 7.17) and on the TMG_COVER
build, which carries parts (a) and (c) and counts them: 10x10 k4, the shape whose kernels pair redraws on the
device, with streams picked with the oracle's trace (a board of more than 300
redraws, rounds going reject, reject, accept, buffered half-words) through
reset_kernel bare and masked and the same-step autoreset; and episodes of one
effective move, where the row-plane move leaves out its closing LDS write
ahead of the regeneration.  tests/test_gpu_bp_pair.py runs its shapes, the
masked reset and the three autoreset modes on the same kernels; the paired
loop of the other shapes, and the rejected word in a carried redraw on 10x10
k5, run on the host wave emulator (tests/test_bp_round_emulated.py)."""
import functools
import os

import numpy as np
import pytest
import torch

from bp_round_cases import ROUND_SHAPE, predicted, round_words
from deep_rollouts import COVER_LIB
from oracle import oracle as orc
from rowplane_cases import FIELDS
from vector_ref import reset_subset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIBS = ["product", "cover"]
COPIES = 8                        # the picked streams, repeated: more than one workgroup per XCD


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


@functools.lru_cache(maxsize=None)
def _words():
    w = np.tile(round_words(orc), (COPIES, 1))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _reference():
    """(prediction of one pass over the streams, state after reset, mask, state
    after the masked reset, idle actions, state after the autoreset step from
    the same streams)."""
    R, C, k = ROUND_SHAPE
    w = _words()
    pred = predicted(orc, ROUND_SHAPE, w)
    o = orc.OracleBatch(R, C, k, 0, 1, w.copy(), threads=16)
    o.reset()
    first = {f: getattr(o, f).copy() for f in ("board", "rng", "timer", "eff")}
    idle = np.array([int(np.nonzero(~orc.effective_mask(b)[0])[0][0]) for b in o.board], np.int32)
    mask = np.arange(w.shape[0]) % 2 == 0
    reset_subset(o, np.nonzero(mask)[0])
    second = {f: getattr(o, f).copy() for f in ("board", "rng", "timer", "eff")}
    o2 = orc.OracleBatch(R, C, k, 0, 1, w.copy(), threads=16)
    o2.reset()
    o2.rng[:] = w
    o2.step(idle, autoreset=True)
    stepped = {f: getattr(o2, f).copy() for f in FIELDS}
    return pred, first, mask, second, idle, stepped


class _State:
    def __init__(self, d):
        self.__dict__.update(d)


@pytest.mark.parametrize("lib", LIBS)
def test_round_sequences(lib):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = ROUND_SHAPE
    path = _lib(lib)
    (acc, rej, longest), first, mask, second, idle, stepped = _reference()
    assert longest > 300 and rej > 0
    w = _words()
    env = TileMatchVecEnv(w.shape[0], R, C, k, 1, [], [], seeds=range(w.shape[0]), device=DEV, lib_path=path)
    _set_rng(env, w)
    if path:
        env.ctx.cover(True)
    env.reset()
    _same(env, _State(first), "reset", ("board", "rng", "timer", "eff"))
    if path:
        h = _counts(env)
        assert h["shuffle_gen"] == 0 and h["reject_gen"] == 0, h
        assert (h["bp_pair_acc"], h["bp_pair_rej"], h["bp_round_carry"]) == (acc, rej, rej), (h, acc, rej)
    env.reset(env_mask=mask.astype(np.uint8))
    _same(env, _State(second), "masked reset", ("board", "rng", "timer", "eff"))
    if path:
        h = _counts(env)
        assert h["bp_round_carry"] == h["bp_pair_rej"] > 0, h
    # the same streams again through the lean step kernel's inline regeneration
    _set_rng(env, w)
    env.reset()                                   # the boards of `first` again: `idle` is ineffective on them
    _set_rng(env, w)
    if path:
        env.ctx.cover(True)
    env.step_raw(torch.from_numpy(idle).to(DEV))
    env.join()
    _same(env, _State(stepped), "same-step autoreset")
    if path:
        h = _counts(env)
        assert (h["bp_pair_acc"], h["bp_pair_rej"], h["bp_round_carry"]) == (acc, rej, rej), (h, acc, rej)
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shape", [(10, 10, 4), (16, 8, 4), (4, 4, 3)], ids=str)
def test_effective_last_move(shape, lib):
    """Episodes of one move, every move effective (drawn on the host from the
    device's mask), same-step autoreset: the move and the regeneration run in
    one wave, and the move's board reaches LDS only for a shuffle."""
    from oracle.policy_np import sample_effective_np
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    n = 1024
    path = _lib(lib)
    env = TileMatchVecEnv(n, R, C, k, 1, [], [], seeds=range(31_000, 31_000 + n), device=DEV, lib_path=path)
    o = orc.OracleBatch(R, C, k, 0, 1, env.rng_words().copy(), threads=16)
    env.reset()
    o.reset()
    if path:
        env.ctx.cover(True)
    for t in range(4):
        a = sample_effective_np(_host(env, "eff"), env.num_actions, 13, 0, t)
        env.step_raw(torch.from_numpy(a).to(DEV))
        env.join()
        o.step(a, autoreset=True)
        _same(env, o, f"{shape} step {t}")
        assert (o.flags & 1).all() and (o.reward >= 3).all()
    assert env.status() == 0
    if path:
        h = _counts(env)
        assert h["sb_lean"] > 0 and h["rp_nolds"] > 0, h
    env.close()
