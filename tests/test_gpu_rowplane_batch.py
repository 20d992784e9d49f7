"""The move-level colour batch of the row-plane cascade (csrc/tmg_rp.hip,
RpBatch) on the MI355X, against the oracle (oracle/tmg_oracle.c): the cases of
tests/test_rowplane_batch_emulated.py as single small batches, and rollouts
with rejections injected into later iterations — on the product library and on
the TMG_COVER build, whose branch counts show the batch was carried, made
again and dropped as the oracle's trace of each move says."""
import os

import numpy as np
import pytest
import torch

from deep_rollouts import COVER_LIB
from oracle import oracle as orc
from rejection_states import words_rejecting_at
from rowplane_batch_cases import (REJECT_SHAPES, ROLLOUT_POSITIONS, WIDE_SHAPES, bookkeeping, carry_cases, draws,
                                  mask_words, rebatch_cases, rejection_cases)
from rowplane_cases import FIELDS, INJECTED, K10, MOVES, STEPS, trace_move

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY = 777
ENVS = 2048
ROLLOUT_SHAPES = [(10, 10, 4), (10, 10, 5), (16, 8, 4)]
LIBS = ["product", "cover"]


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


def _same(env, o, what):
    n = env.num_envs
    for f in FIELDS:
        got, want = _host(env, f), getattr(o, f)
        if not np.array_equal(got, want):
            bad = np.nonzero((got.reshape(n, -1) != want.reshape(n, -1)).any(axis=1))[0]
            raise AssertionError(f"{what}: {f} differs in {bad.size} envs, first {bad[:5]}")


def _set_rng(env, w):
    env.rng.copy_(torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(DEV))


def _counts(env):
    from tile_match_gym_amd import _native
    c = env.ctx.cover()
    return {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}


def _move(lib, shape, boards, eff, words, acts, what):
    """One trusted step of hand-set envs (board, cached mask, stream) against
    the oracle; returns the cover counts of that step on the cover build."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    n = words.shape[0]
    assert n <= 64
    path = _lib(lib)
    env = TileMatchVecEnv(n, R, C, k, 30, [], [], seeds=range(n), device=DEV, lib_path=path)
    env.reset()
    env.join()
    env.board.copy_(torch.from_numpy(np.ascontiguousarray(boards, dtype=np.int8)).to(DEV).reshape(env.board.shape))
    env.eff.copy_(torch.from_numpy(np.ascontiguousarray(eff, dtype=np.uint64).view(np.int64)).to(DEV).reshape(env.eff.shape))
    _set_rng(env, words)
    env.timer.zero_()
    o = orc.OracleBatch(R, C, k, 0, 30, words, threads=1)
    o.board[:] = boards
    o.eff[:] = np.asarray(eff, dtype=np.uint64).reshape(o.eff.shape)
    if path:
        env.ctx.cover(True)
    env.step(torch.from_numpy(np.ascontiguousarray(acts, dtype=np.int32)).to(DEV))
    o.step(np.ascontiguousarray(acts, dtype=np.int32), autoreset=True)
    _same(env, o, what)
    assert env.status() == 0
    counts = _counts(env) if path else None
    env.close()
    return o, counts


@pytest.mark.parametrize("lib", LIBS)
def test_carry(lib):
    """The crafted cascades as seeded and with a buffered half-word, one batch:
    later iterations take their colours from the move's batch; the position
    written back is the oracle's after moves that end with and without a
    buffered half-word."""
    cases = carry_cases(orc)
    carry = 0
    flag = set()
    for nm, b, a, w in cases:
        its, fb, rng = trace_move(orc, b, w, a, K10)
        c, again = bookkeeping(draws(its))
        assert c > 0 and again == 0, nm
        carry += c
        flag.add(int(rng[4] >> np.uint64(32)))
    assert flag == {0, 1}
    boards = np.stack([c[1] for c in cases])
    eff = np.stack([mask_words(orc.effective_mask(c[1])[0]) for c in cases])
    words = np.stack([c[3] for c in cases])
    acts = np.array([c[2] for c in cases], np.int32)
    o, counts = _move(lib, (10, 10, K10), boards, eff, words, acts, "carry")
    assert (o.reward >= 3).all()
    if counts:
        assert counts["rp_carry"] == carry and counts["rp_rebatch"] == 0, counts


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shape", WIDE_SHAPES)
def test_rebatch(shape, lib):
    """Striped boards whose first refill takes (nearly) a whole batch and whose
    cascade goes on: a second batch within the move where the board has the
    cells for it (16x8), carried iterations after a refill of more than 64
    where it has not (3x28: rowplane_batch_cases.rebatch_cases)."""
    R, C, k = shape
    b, eff, acts, w = rebatch_cases(orc, shape)
    n = w.shape[0]
    again = 0
    for i in range(n):
        ts = draws(trace_move(orc, b, w[i], int(acts[i]), k)[0])
        assert len(ts) >= 2, (shape, i)
        again += bookkeeping(ts)[1]
    assert again >= n or R * C < 128
    o, counts = _move(lib, shape, np.stack([b] * n), np.stack([eff] * n), w, acts, f"{shape} re-batch")
    assert (o.reward > 64).all()
    if counts:
        assert counts["rp_reject"] == 0 and counts["rp_wide"] == n, counts
        assert counts["rp_rebatch"] == again, counts
        if R * C >= 128:
            assert counts["rp_rebatch"] > 0, counts
        else:
            assert counts["rp_carry"] >= n, counts


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shape", REJECT_SHAPES)
def test_rejection_in_carried_range(shape, lib):
    """A rejected word among the colours the move's second iteration takes
    from the carried batch: serial replay from the exact position.  A rejected
    word just beyond the move's last draw: no effect at all."""
    o0, inside, beyond = rejection_cases(orc, shape)
    for what, (idx, acts, w) in (("inside", inside), ("beyond", beyond)):
        n = idx.size
        _, counts = _move(lib, shape, o0.board[idx], o0.eff[idx], w, acts, f"{shape} {what}")
        if counts and what == "inside":
            assert counts["rp_reject"] >= n and counts["rp_carry"] >= n, counts
        if counts and what == "beyond":
            assert counts["rp_reject"] == 0, counts


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shape", ROLLOUT_SHAPES)
def test_rollout(shape, lib):
    """2048 envs, 40 policy-effective steps, episodes of 10 moves; on 10x10 k5
    a Lemire rejection at draw 0-15 (half with a buffered half-word) before
    every 5th step.  Product build: every field against the oracle at every
    step.  Cover build, same trajectories: the batch was carried (and dropped
    by a rejection where one is injected)."""
    from oracle.policy_np import sample_effective_np
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    path = _lib(lib)
    base = 90_000 + 5_000 * ROLLOUT_SHAPES.index(shape)
    env = TileMatchVecEnv(ENVS, R, C, k, MOVES, [], [], seeds=range(base, base + ENVS), device=DEV, lib_path=path)
    o = None if path else orc.OracleBatch(R, C, k, 0, MOVES, env.rng_words().copy(), threads=16)
    env.reset()
    if o:
        o.reset()
    rs = np.random.default_rng(base)
    for t in range(STEPS):
        if shape in INJECTED and t % 5 == 1:
            w = words_rejecting_at(env.rng_words(), rs.integers(0, ROLLOUT_POSITIONS, ENVS), buffered=rs.random(ENVS) < 0.5)
            _set_rng(env, w)
            if o:
                o.rng[:] = w
        # actions drawn on the host from the device's own mask and handed over:
        # with the in-kernel draw the 10x10 shapes would run on the lane kernel
        a = sample_effective_np(_host(env, "eff"), env.num_actions, KEY, 0, t)
        env.step_raw(torch.from_numpy(a).to(DEV))
        env.join()
        if o:
            o.step(a, autoreset=True)
            _same(env, o, f"{shape} step {t}")
    torch.cuda.synchronize()
    assert env.status() == 0
    if path:
        counts = _counts(env)
        assert counts["sb_lean"] > 0 and counts["rp_carry"] > 0, counts
        if shape in INJECTED:
            assert counts["rp_reject"] > 0, counts
    env.close()
