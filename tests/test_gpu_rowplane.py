"""The row-plane lean cascade (csrc/tmg_rp.hip) on the MI355X, against the
oracle (oracle/tmg_oracle.c): rollouts with the effective-action policy on
every shape class the path covers (with crafted Lemire rejections in the
refill on 10x10 k5 and 5x6 k7), hand-written boards showing one feature of
the cascade each, and the same runs on the TMG_COVER build counting the new
branches."""
import os

import numpy as np
import pytest
import torch

from deep_rollouts import COVER_LIB
from oracle import oracle as orc
from rejection_states import words_rejecting_at
from rowplane_cases import (FEATURES, FIELDS, INJECTED, K10, MOVES, SHAPES, STEPS, crafted, stream_words, trace_move)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY = 777
ENVS = 2048


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


def _rollout(shape, lib_path=None, ref=True):
    from oracle.policy_np import sample_effective_np
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    base = 50_000 + 5_000 * SHAPES.index(shape)
    env = TileMatchVecEnv(ENVS, R, C, k, MOVES, [], [], seeds=range(base, base + ENVS), device=DEV, lib_path=lib_path)
    o = orc.OracleBatch(R, C, k, 0, MOVES, env.rng_words().copy(), threads=16) if ref else None
    env.reset()
    if ref:
        o.reset()
    rs = np.random.default_rng(base)
    for t in range(STEPS):
        if shape in INJECTED and t % 5 == 1:
            w = words_rejecting_at(env.rng_words(), rs.integers(0, 8, ENVS), buffered=rs.random(ENVS) < 0.5)
            _set_rng(env, w)
            if ref:
                o.rng[:] = w
        # the examples' policy, drawn on the host from the device's own mask and
        # handed over as actions: with the in-kernel draw (step_effective) the
        # 10x10 shapes would run on the lane-per-board kernel instead
        a = sample_effective_np(_host(env, "eff"), env.num_actions, KEY, 0, t)
        env.step_raw(torch.from_numpy(a).to(DEV))
        env.join()
        if ref:
            o.step(a, autoreset=True)
            _same(env, o, f"{shape} step {t}")
    torch.cuda.synchronize()
    return env


def _sites(shape):
    want = ["sb_lean", "rp_passes", "rp_perp"]          # the events tests/test_rowplane_emulated.py finds in 64 envs
    if shape[0] >= 4:
        want.append("rp_vlong")
    if shape in INJECTED:
        want.append("rp_reject")
    return want


@pytest.mark.parametrize("shape", SHAPES)
def test_rollout_vs_oracle(shape):
    env = _rollout(shape)
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_rollout_sites_taken(shape):
    """TMG_COVER build, same trajectories: every new branch the shape reaches was taken."""
    from tile_match_gym_amd import _native
    assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
    env = _rollout(shape, lib_path=COVER_LIB, ref=False)
    c = env.ctx.cover()
    counts = {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}
    assert env.status() == 0
    missing = {s: counts[s] for s in _sites(shape) if counts[s] == 0}
    assert not missing, f"{shape}: sites never taken: {missing} (counts {counts})"
    env.close()


def _crafted_env(lib_path, names, cases):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    n = len(names)
    w = np.stack([stream_words(cases[nm][2]) for nm in names])
    boards = np.stack([np.stack([cases[nm][0], np.ones_like(cases[nm][0])]) for nm in names]).astype(np.int8)
    env = TileMatchVecEnv(n, 10, 10, K10, 30, [], [], seeds=range(n), device=DEV, lib_path=lib_path)
    env.reset()
    env.join()
    env.board.copy_(torch.from_numpy(boards).to(DEV).reshape(env.board.shape))
    _set_rng(env, w)
    env.timer.zero_()
    env.invalidate_effective_cache()
    return env, w, boards


@pytest.mark.parametrize("lib", ["product", "cover"])
def test_crafted_boards(lib):
    """Each hand-written board: one untrusted step with an ineffective action
    (the general kernel; the row-plane path needs a trusted mask), then the
    move.  The feature is asserted on the oracle's own lines, and on the cover
    build by the branch count of that board alone."""
    from tile_match_gym_amd import _native
    cases = crafted()
    names = sorted(cases)
    for nm in names:
        col, a, seed = cases[nm]
        b = np.stack([col, np.ones_like(col)]).astype(np.int8)
        w = stream_words(seed)
        assert orc.get_colour_lines(b, K10, 0) == [], nm
        its, fb, rng = trace_move(orc, b, w, a, K10)
        mb, mrng, res, err = orc.move(b, w, a, K10, 0)
        assert err == 0 and np.array_equal(fb, mb) and np.array_equal(rng, mrng), nm
        assert FEATURES[nm][0](its), f"{nm}: the oracle's cascade does not show the feature"
        assert res[0] >= 3
    if lib == "product":
        groups = [names]
        path = None
    else:
        assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
        groups = [[nm] for nm in names if FEATURES[nm][1] or nm == "six_iterations"]
        path = COVER_LIB
    for g in groups:
        env, w, boards = _crafted_env(path, g, cases)
        o = orc.OracleBatch(10, 10, K10, 0, 30, w, threads=1)
        o.board[:] = boards
        idle = np.array([int(np.nonzero(~orc.effective_mask(b)[0])[0][0]) for b in boards], np.int32)
        env.step(torch.from_numpy(idle).to(DEV))
        o.step(idle, autoreset=True)
        _same(env, o, f"{g} mask step")
        if path:
            env.ctx.cover(True)
        acts = np.array([cases[nm][1] for nm in g], np.int32)
        env.step(torch.from_numpy(acts).to(DEV))
        o.step(acts, autoreset=True)
        _same(env, o, f"{g} move")
        assert (o.reward >= 3).all()
        assert env.status() == 0
        if path:
            c = env.ctx.cover()
            counts = {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}
            site = FEATURES[g[0]][1]
            if site:
                assert counts[site] > 0, (g[0], site, counts)
            if g[0] == "six_iterations":
                assert counts["sb_lean"] >= 6, counts
        env.close()
