"""The lane-per-board step (csrc/tmg_lane.h, lane_step_kernel<10,10,K,EPW>) on
the MI355X, on the branches random 10x10 play never takes, against the oracle
(oracle/tmg_oracle.c):

* crafted boards whose move shuffles (tests/lane_cases.py): shuffle with its
  per-lane LDS index array, interval, redraw_rows, on 32-env and on 64-env
  waves (lanes 32..63 included), and the moves that follow on those boards;
* crafted Lemire rejections of draw_code<5> in the refill and in the redraws
  after a shuffle (tests/rejection_states.py);
* the next-step autoreset (kernel code 4, then the masked reset);
* given actions with out-of-range values (the caller-error exit);
* the same crafted k4 states on the specialised c2 wave kernel
  (step_kernel<128,false,2,false,kFixC2>), which had never shuffled either.

Every parity check compares every field of every env after every step with
OracleBatch, and the sticky status with what the oracle's flags imply.  Which
envs shuffle is asserted on the oracle's flags.  The lib="cover" cases run the
same trajectories on the TMG_COVER build and assert the lane sites by their
counters (and sb_lean == 0: the lane kernel, not a wave kernel, took the
trusted steps)."""
import os

import numpy as np
import pytest
import torch

import lane_cases as lc
from deep_rollouts import COVER_LIB
from oracle import oracle as orc
from oracle.policy_np import sample_effective_np
from rejection_states import words_rejecting_at
from vector_ref import reset_subset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIBS = ["product", "cover"]
STATUS_CALLER = 4
LANE_SMALL = 32768              # kLaneSmallEnvs: launches from this size on take 64 envs per wave
LANE_MIN = 131072               # kLaneMinEnvs: given-action launches from this size on run on the lane kernel


def _lib_path(lib):
    if lib == "product":
        return None
    assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
    return COVER_LIB


def _host(env, f):
    if f == "rng":
        return env.rng_words()
    v = getattr(env, f).cpu().numpy()
    return v.view(np.uint64) if f == "eff" else v


def _same(env, o, what, actions=None):
    """Every field of every env equals the oracle's; the sticky status is the
    caller-error bit exactly when the oracle flagged an env."""
    n = env.num_envs
    for f in lc.FIELDS:
        got, want = _host(env, f), getattr(o, f)
        if not np.array_equal(got, want):
            bad = np.nonzero((got.reshape(n, -1) != want.reshape(n, -1)).any(axis=1))[0]
            raise AssertionError(f"{what}: {f} differs in {bad.size} envs, first {bad[:5]}")
    if actions is not None:
        assert np.array_equal(env.actions.cpu().numpy(), actions), f"{what}: sampled actions"
    assert env.status(clear=True) == (STATUS_CALLER if (o.flags & 0x80).any() else 0), f"{what}: status"


def _set_rng(env, o, w):
    env.rng.copy_(torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(DEV))
    o.rng[:] = w


def _counts(env, case):
    from tile_match_gym_amd import _native
    c = env.ctx.cover()
    counts = {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}
    out = os.environ.get("TMG_EVIDENCE_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"lane_{case}.txt"), "w") as f:
            f.write(repr(counts) + "\n")
    return counts


def _crafted_run(case, lib, k, n, steps, inject_seed=None, host_policy=False):
    """The crafted batch on the device and on the oracle: the boards and fresh
    streams go into the env's tensors, one untrusted step with an ineffective
    action lets the library write the masks (the general kernel), then `steps`
    trusted steps of the policy follow (t = 1..).  Returns the envs whose first
    trusted move shuffles on the oracle, the effective moves the oracle made,
    and the cover counts of the trusted steps (lib="cover")."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    path = _lib_path(lib)
    env = TileMatchVecEnv(n, lc.R, lc.C, k, 30, seeds=range(lc.SEED0, lc.SEED0 + n), device=DEV, lib_path=path)
    env.reset()
    env.join()
    o, idle = lc.crafted_oracle(k, n)
    env.board.copy_(torch.from_numpy(o.board).to(DEV))
    _set_rng(env, o, o.rng.copy())
    env.timer.zero_()
    env.invalidate_effective_cache()
    env.step(torch.from_numpy(idle).to(DEV))
    o.step(idle, autoreset=True)
    _same(env, o, f"{case}: mask step")
    assert (o.timer == 1).all() and (o.flags == 0).all()
    if inject_seed is not None:
        _set_rng(env, o, words_rejecting_at(o.rng, *lc.redraw_positions(n, inject_seed)))
    if path:
        env.ctx.cover(True)
    moves, shuffled = 0, None
    for t in range(1, 1 + steps):
        a = sample_effective_np(o.eff, lc.A, lc.KEY, 0, t)
        if host_policy:
            d_a = torch.from_numpy(a).to(DEV)
            env.step_raw(d_a)
        else:
            env.step_effective(t, key=lc.KEY)
        env.join()
        o.step(a, autoreset=True)
        _same(env, o, f"{case}: step {t}", None if host_policy else a)
        moves += int((o.reward > 0).sum())
        if t == 1:
            assert (o.reward >= 3).all(), "every crafted env's move is effective"
            shuffled = np.nonzero(o.flags & 4)[0]
    counts = _counts(env, case) if path else None
    env.close()
    return shuffled, moves, counts


def _lane_sites(counts, moves, shuffled, redraw=True):
    """The lane kernel took every effective move of the trusted steps (no wave
    kernel's cascade ran), shuffled at least once per shuffling env, and redrew."""
    assert counts["sb_lean"] == 0 and counts["fast"] == 0 and counts["serial_step"] == 0, counts
    assert counts["lane_step"] == moves, counts
    assert counts["lane_shuffle"] >= shuffled and counts["shuffle"] == 0, counts
    if redraw:
        assert counts["lane_redraw"] > 0, counts


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k", [4, 5])
def test_crafted_shuffles(k, lib):
    """32-env waves (2048 envs): the crafted move, then 8 more on the boards it left."""
    n = 2048
    shuffled, moves, counts = _crafted_run(f"crafted_k{k}", lib, k, n, 9)
    assert shuffled.size >= lc.MIN_SHUFFLED[k], f"only {shuffled.size} envs shuffle on the oracle"
    if counts:
        _lane_sites(counts, moves, shuffled.size)


@pytest.mark.parametrize("lib", LIBS)
def test_crafted_shuffles_wave64(lib):
    """64-env waves with a ragged last wave: shuffles on lanes 32..63 too."""
    k, n = 5, LANE_SMALL + 37
    shuffled, moves, counts = _crafted_run("wave64_k5", lib, k, n, 4)
    assert (shuffled % 64 >= 32).any(), "no shuffling env on lanes 32..63"
    if counts:
        _lane_sites(counts, moves, shuffled.size)


@pytest.mark.parametrize("lib", LIBS)
def test_redraw_rejections(lib):
    """draw_code<5>'s rejection loop inside redraw_rows: rejected words at draws
    100..400 of the crafted states.  The new streams change which envs shuffle;
    the oracle's count is asserted again."""
    k, n = 5, 2048
    shuffled, moves, counts = _crafted_run("redraw_reject_k5", lib, k, n, 4, inject_seed=77)
    assert shuffled.size >= lc.MIN_SHUFFLED[k], f"only {shuffled.size} envs shuffle on the oracle"
    if counts:
        _lane_sites(counts, moves, shuffled.size)
        assert counts["lane_reject_redraw"] > 0, counts


@pytest.mark.parametrize("lib", LIBS)
def test_refill_rejections(lib):
    """draw_code<5>'s rejection loop inside a refill: a plain rollout of the
    policy, a rejected word put at draw 0..2 of every env before every 5th
    step (half of the states with a buffered half-word).  Episodes of 10 moves:
    the masked reset after the lane kernel runs too."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    k, n, M, steps = 5, 2048, 10, 20
    path = _lib_path(lib)
    env = TileMatchVecEnv(n, lc.R, lc.C, k, M, seeds=range(lc.SEED0, lc.SEED0 + n), device=DEV, lib_path=path)
    o = orc.OracleBatch(lc.R, lc.C, k, 0, M, env.rng_words().copy(), threads=16)
    env.reset()
    o.reset()
    rs = np.random.default_rng(k)
    moves = injected = 0
    for t in range(steps):
        if t % 5 == 1:
            _set_rng(env, o, words_rejecting_at(o.rng, rs.integers(0, 3, n), buffered=rs.random(n) < 0.5))
            injected += n
        a = sample_effective_np(o.eff, lc.A, lc.KEY, 0, t)
        env.step_effective(t, key=lc.KEY)
        env.join()
        o.step(a, autoreset=True)
        _same(env, o, f"refill rejections: step {t}", a)
        assert (o.reward >= 3).all()
        moves += n
    if path:
        counts = _counts(env, "refill_reject_k5")
        _lane_sites(counts, moves, 0, redraw=False)
        # every injected word is met: each env's move refills at least 3 cells
        assert counts["lane_reject"] >= injected and counts["lane_reject_redraw"] == 0, counts
    env.close()


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k", [4, 5])
def test_next_step_autoreset(k, lib):
    """Kernel autoreset code 4: an env that ended last step is regenerated
    instead of stepped (reward 0, flags 8, the policy's draw from its zeroed
    mask still written), by the masked reset behind the lane kernel."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    n, M, steps = 2048, 5, 17
    path = _lib_path(lib)
    env = TileMatchVecEnv(n, lc.R, lc.C, k, M, seeds=range(9000, 9000 + n), device=DEV, lib_path=path)
    env.set_step_outputs("next_step")
    o = orc.OracleBatch(lc.R, lc.C, k, 0, M, env.rng_words().copy(), threads=16)
    env.reset()
    o.reset()
    pending = np.zeros(n, bool)
    moves = resets = 0
    for t in range(steps):
        a = sample_effective_np(o.eff, lc.A, lc.KEY, 0, t)
        env.step_effective(t, key=lc.KEY)
        env.join()
        idx = np.nonzero(pending)[0]
        o.step(np.where(pending, 0, a), autoreset=False)
        moves += int((o.reward[~pending] > 0).sum())
        reset_subset(o, idx)
        o.reward[idx] = 0
        o.flags[idx] = 8
        resets += idx.size
        pending = (o.flags & 1) != 0
        _same(env, o, f"next-step k{k}: step {t}", a)
    assert resets == 2 * n                  # episodes end at t = 4, 10, 16: every env is regenerated at t = 5 and 11
    if path:
        counts = _counts(env, f"next_step_k{k}")
        _lane_sites(counts, moves, 0, redraw=False)
    env.close()


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("mode", ["none", "same_step"])
def test_given_actions_and_caller_errors(mode, lib):
    """Given actions on the lane kernel (>= kLaneMinEnvs envs, 64-env waves, a
    ragged last wave): half uniform, half effective, 1 % out of range (-1, A,
    2^31 - 1, -2^31).  Those envs stay as they were with flags 0x80
    (tile_match_env.py:94-95) and raise the caller-error status; episodes of 2
    moves, so the second step ends every live episode and, without autoreset,
    the third is a caller error of every env that ended."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    k, n, M = 4, LANE_MIN + 37, 2
    path = _lib_path(lib)
    env = TileMatchVecEnv(n, lc.R, lc.C, k, M, seeds=range(lc.SEED0, lc.SEED0 + n), device=DEV,
                          autoreset=mode == "same_step", lib_path=path)
    o = orc.OracleBatch(lc.R, lc.C, k, 0, M, env.rng_words().copy(), threads=16)
    env.reset()
    o.reset()
    rs = np.random.default_rng(131)
    bad_values = np.array([-1, lc.A, 2**31 - 1, -2**31], np.int64)
    moves = 0
    for t in range(3):
        a = rs.integers(0, lc.A, n).astype(np.int64)
        eff = sample_effective_np(o.eff, lc.A, 99, 0, t)
        a = np.where(rs.random(n) < 0.5, eff, a)
        bad = np.nonzero(rs.random(n) < 0.01)[0]
        bad = np.union1d(bad, [31, 32, 63, n - 1])              # both half-waves, the ragged tail
        a[bad] = bad_values[np.arange(bad.size) % 4]
        a = a.astype(np.int32)
        before = {f: _host(env, f)[bad].copy() for f in ("board", "rng", "timer", "eff")}
        d_a = torch.from_numpy(a).to(DEV)
        env.step_raw(d_a)
        env.join()
        o.step(a, autoreset=mode == "same_step")
        assert (o.flags[bad] == 0x80).all()
        _same(env, o, f"given actions {mode}: step {t}")        # status == STATUS_CALLER: bad is never empty
        for f, v in before.items():
            assert np.array_equal(_host(env, f)[bad], v), f"step {t}: {f} of an env with a bad action changed"
        assert (_host(env, "flags")[bad] == 0x80).all()
        moves += int((o.reward > 0).sum())
    if path:
        _lane_sites(_counts(env, f"given_{mode}"), moves, 0, redraw=False)
    env.close()


@pytest.mark.parametrize("lib", LIBS)
def test_c2_wave_kernel_shuffles(lib):
    """The crafted k4 states with the policy's draw made on the host and given
    as actions: 2048 envs run on step_kernel<128,false,2,false,kFixC2>
    (row-plane cascade, then sb_ensure), which shuffles inside the move."""
    k, n = 4, 2048
    shuffled, moves, counts = _crafted_run("c2_wave_k4", lib, k, n, 9, host_policy=True)
    assert shuffled.size >= lc.MIN_SHUFFLED[k], f"only {shuffled.size} envs shuffle on the oracle"
    if counts:
        assert counts["lane_step"] == 0 and counts["sb_lean"] >= moves, counts
        assert counts["shuffle"] >= shuffled.size, counts
