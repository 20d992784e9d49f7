"""The lean step's three-row gravity shift (csrc/tmg_rp.hip, rp_move,
TMG_RP_VSHIFT) and its effective-mask scan on the cascade's own planes
(rp_scan, TMG_RP_SCAN2) on the MI355X, against the oracle
(oracle/tmg_oracle.c): every field, every step.  Rollouts on every shape class
of the two paths, each cached mask beside a fresh tmg_effective of the same
board, the boards picked with the oracle's trace for one gravity feature each,
and the same on the TMG_COVER build counting the two new sites."""
import os

import numpy as np
import pytest
import torch

from deep_rollouts import COVER_LIB
from lean_levers_cases import (CASE_SHAPES, CASES, FIELDS, GRAVITY_SHAPES, MOVES, PREDICATES, SCAN_SHAPES, SITES, STEPS,
                               case_arrays, case_predicates)
from oracle import oracle as orc
from rowplane_cases import trace_move

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY = 31
ENVS = 1024
ROLLOUT_SHAPES = GRAVITY_SHAPES + [s for s in SCAN_SHAPES if s not in GRAVITY_SHAPES]


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


def _counts(env):
    from tile_match_gym_amd import _native
    c = env.ctx.cover()
    return {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}


def _rollout(shape, lib_path=None, ref=True):
    """Actions drawn on the host from the device's own mask (the in-kernel
    draw would send the 10x10 shapes to the lane-per-board kernel), episodes
    of MOVES moves with the inline autoreset."""
    from oracle.policy_np import sample_effective_np
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    base = 70_000 + 3_000 * ROLLOUT_SHAPES.index(shape)
    env = TileMatchVecEnv(ENVS, R, C, k, MOVES, [], [], seeds=range(base, base + ENVS), device=DEV, lib_path=lib_path)
    o = orc.OracleBatch(R, C, k, 0, MOVES, env.rng_words().copy(), threads=16) if ref else None
    env.reset()
    if ref:
        o.reset()
    for t in range(STEPS):
        a = sample_effective_np(_host(env, "eff"), env.num_actions, KEY, 0, t)
        env.step_raw(torch.from_numpy(a).to(DEV))
        env.join()
        if ref:
            o.step(a, autoreset=True)
            _same(env, o, f"{shape} step {t}")
            env.compute_effective()                       # a fresh tmg_effective of the same boards
            assert np.array_equal(_host(env, "eff"), o.eff), f"{shape} step {t}: fresh mask"
    torch.cuda.synchronize()
    return env


@pytest.mark.parametrize("shape", ROLLOUT_SHAPES)
def test_rollout_vs_oracle(shape):
    env = _rollout(shape)
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4), (16, 8, 4), (3, 28, 6)])
def test_rollout_sites_taken(shape):
    """TMG_COVER build, same trajectories: the three-row shift ran, passes were
    still needed after it somewhere (10x10 k4), and rp_passes still counts
    every iteration that needed more than one one-row pass: those that clear a
    vertical run (without one every cleared cell lies in the bottom row of the
    lines, one hole per column), so the two counts are equal."""
    assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
    env = _rollout(shape, lib_path=COVER_LIB, ref=False)
    counts = _counts(env)
    assert env.status() == 0
    assert counts["rp_vshift"] > 0 and counts["rp_passes"] == counts["rp_vshift"], counts
    if shape == (10, 10, 4):
        assert 0 < counts["rp_vmore"] < counts["rp_vshift"], counts
    env.close()


def _set_rng(env, w):
    env.rng.copy_(torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(DEV))


def _case_env(lib_path, shape, names):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    arr = [case_arrays(nm) for nm in names]
    boards = np.stack([a[2] for a in arr])
    acts = np.array([a[3] for a in arr], np.int32)
    w = np.stack([a[4] for a in arr])
    env = TileMatchVecEnv(len(names), R, C, k, 30, [], [], seeds=range(len(names)), device=DEV, lib_path=lib_path)
    env.reset()
    env.join()
    env.board.copy_(torch.from_numpy(boards).to(DEV).reshape(env.board.shape))
    _set_rng(env, w)
    env.timer.zero_()
    env.invalidate_effective_cache()
    return env, w, boards, acts


@pytest.mark.parametrize("lib", ["product", "cover"])
@pytest.mark.parametrize("shape", CASE_SHAPES)
def test_gravity_cases(shape, lib):
    """Each board: the feature asserted on the oracle's own trace, one
    untrusted step with an ineffective action (the general kernel; the
    row-plane path needs a trusted mask), then the move.  On the cover build
    one board at a time, for its own counts."""
    R, C, k = shape
    names = sorted(nm for nm in CASES if CASES[nm][1] == shape)
    for nm in names:
        _, _, b, a, w = case_arrays(nm)
        assert orc.get_colour_lines(b, k, 0) == [], nm
        its, fb, rng = trace_move(orc, b, w, a, k)
        mb, mrng, res, err = orc.move(b, w, a, k, 0)
        assert err == 0 and np.array_equal(fb, mb) and np.array_equal(rng, mrng), nm
        for pred in case_predicates(nm):
            assert PREDICATES[pred](its, R), f"{nm}: the oracle's cascade does not show {pred}"
    if lib == "product":
        groups, path = [names], None
    else:
        assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
        groups, path = [[nm] for nm in names], COVER_LIB
    for g in groups:
        env, w, boards, acts = _case_env(path, shape, g)
        o = orc.OracleBatch(R, C, k, 0, 30, w, threads=1)
        o.board[:] = boards
        idle = np.array([int(np.nonzero(~orc.effective_mask(b)[0])[0][0]) for b in boards], np.int32)
        env.step(torch.from_numpy(idle).to(DEV))
        o.step(idle, autoreset=True)
        _same(env, o, f"{g} mask step")
        if path:
            env.ctx.cover(True)
        env.step(torch.from_numpy(acts).to(DEV))
        o.step(acts, autoreset=True)
        _same(env, o, f"{g} move")
        assert (o.reward >= 3).all()
        assert env.status() == 0
        if path:
            counts = _counts(env)
            assert counts["rp_vshift"] > 0 and counts["rp_passes"] >= counts["rp_vshift"], (g[0], counts)
            for site in {SITES[pred] for pred in case_predicates(g[0])} - {None}:
                assert counts[site] > 0, (g[0], site, counts)
        env.close()
