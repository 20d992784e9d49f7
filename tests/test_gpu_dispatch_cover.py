"""Every kernel instantiation of csrc/tmg_dispatch.h, and the bitboard lean
cascade (sb_move, tmg_sb.hip), on the MI355X against the oracle.

The row-plane cascade (tmg_rp.hip) takes every lean move with R <= 16 and
C <= 28, so the older parity shapes no longer run sb_move; the tall and wide
boards of tests/dispatch_cases.py do, with vertical lines longer than a DPP
row, rows wider than the row scan (C > 28) and than bp_generate (C > 32).  The
same table carries the general bitboard kernels over those boundaries and the
plane counts, the C = 64 kernels and the 512-cell resets no other list
launches (the census in tests/test_dispatch_route.py keeps it complete).

* rollouts: even steps take the in-kernel effective-action policy, odd steps
  uniform given actions (the ineffective quick exit and the cascade), episodes
  of 10 moves; every field of every env at every step equals the oracle;
* the same trajectories on the TMG_COVER build: the tall / wide lean shapes
  count sb_lean and no row-plane site, the row-plane control the row-plane
  sites, so a change of the rule that takes a shape from one cascade to the
  other cannot pass unseen;
* hand-built tall and wide boards, the feature asserted on the oracle first.

The masked resets of the new reset instantiations are cases of
tests/test_gpu_paths.py's test_masked_reset_subsets_vs_oracle."""
import os

import numpy as np
import pytest
import torch

import dispatch_cases as dc
from deep_rollouts import COVER_LIB, specials
from oracle import oracle as orc
from oracle.policy_np import sample_effective_np
from rejection_states import words_rejecting_at
from rowplane_cases import _cleared, _horizontal, _vertical, f_plus, f_T, haction, trace_move, vaction
from test_gpu_paths import _inject

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY = 4242
MOVES = 10          # test_gpu_paths._inject places its far rejections before every 10th step
ENVS = 1024
STEPS = 30
FIELDS = ("board", "rng", "timer", "eff", "reward", "n_new", "n_act", "flags")
RP_SITES = ("rp_passes", "rp_perp", "rp_vlong", "rp_wide", "rp_reject", "rp_carry", "rp_rebatch")
ROLLOUTS = dc.CASES + [dc.ROW_PLANE_CONTROL]


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


def _rollout(shape, mode="same_step", lib_path=None, ref=True):
    """30 steps of 1024 envs.  Returns (env, shuffles in moves on the oracle)."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, sm = shape
    cl, co = specials(sm)
    base = 300_000 + 4_000 * ROLLOUTS.index(shape)
    n = ENVS
    env = TileMatchVecEnv(n, R, C, k, MOVES, cl, co, seeds=range(base, base + n), device=DEV, groups=1,
                          lib_path=lib_path)
    if mode == "next_step":
        env.set_step_outputs("next_step")
    o = orc.OracleBatch(R, C, k, sm, MOVES, env.rng_words().copy(), threads=16) if ref else None
    env.reset()
    if ref:
        o.reset()
        _same_state(env, o, f"{shape} reset")
    rs = np.random.default_rng(base)
    A = env.num_actions
    pending = np.zeros(n, bool)
    shuffled = 0
    for t in range(STEPS):
        if shape in dc.WIDE_EXACT:
            inj = _inject(t, n, rs)
            if inj is not None:
                w = words_rejecting_at(env.rng_words(), inj[0], buffered=inj[1])
                _set_rng(env, w)
                if ref:
                    o.rng[:] = w
        uniform = rs.integers(0, A, n).astype(np.int32)         # drawn every step: the same stream with and without ref
        if t % 2:
            a = uniform
            env.step(torch.from_numpy(a).to(DEV))
        elif shape == dc.ROW_PLANE_CONTROL:
            # the in-kernel draw would put this shape on the lane-per-board
            # kernel: the same draw made on the host, from the device's own mask
            a = sample_effective_np(_host(env, "eff"), A, KEY, 0, t)
            env.step_raw(torch.from_numpy(a).to(DEV))
        else:
            a = sample_effective_np(o.eff, A, KEY, 0, t) if ref else None
            env.step_effective(t, key=KEY)
        env.join()
        if not ref:
            continue
        if mode == "next_step":
            idx = np.nonzero(pending)[0]
            o.step(np.where(pending, 0, a).astype(np.int32), autoreset=False)
            shuffled += int(((o.flags[~pending] & 4) != 0).sum())
            _reset_subset(o, idx)
            o.reward[idx] = 0
            o.flags[idx] = 8                                    # FL_RESET: regenerated instead of stepped
            pending = (o.flags & 1) != 0
        else:
            o.step(a, autoreset=True)
            shuffled += int(((o.flags & 4) != 0).sum())
        _same(env, o, f"{shape} {mode} step {t}")
        assert not (_host(env, "flags") & 0xC0).any(), f"{shape} step {t}: error / overflow flag"
    torch.cuda.synchronize()
    return env, shuffled


def _reset_subset(o, idx):
    """vector_ref.reset_subset on 16 threads (4x29 k4 boards take many redraws to come out line-free)."""
    if len(idx):
        sub = orc.OracleBatch(o.R, o.C, o.k, o.smask, o.num_moves, o.rng[idx].copy(), threads=16)
        sub.reset()
        o.board[idx], o.rng[idx], o.timer[idx], o.eff[idx] = sub.board, sub.rng, sub.timer, sub.eff


def _same_state(env, o, what):
    for f in ("board", "rng", "timer", "eff"):
        assert np.array_equal(_host(env, f), getattr(o, f)), f"{what}: {f}"


@pytest.mark.parametrize("shape", ROLLOUTS, ids=dc.case_id)
def test_rollout_vs_oracle(shape):
    """Product library, same-step autoreset (two per env): every field of every env at every step."""
    env, shuffled = _rollout(shape)
    assert env.status() == 0
    if shape in dc.SHUFFLES:
        assert shuffled > 0, "the rollout was meant to shuffle inside moves"
    env.close()


@pytest.mark.parametrize("shape", dc.LEAN, ids=dc.case_id)
def test_rollout_next_step_vs_oracle(shape):
    """The lean shapes with next-step autoreset (kernel code 3 inline, 4 for
    the 512-cell ones): an env that ended is regenerated by the call after,
    reward 0 and flags 8, on a policy step (t = 10) and a given-action step (t = 21)."""
    env, _ = _rollout(shape, mode="next_step")
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", ROLLOUTS, ids=dc.case_id)
def test_sites_taken(shape):
    """TMG_COVER build, the trajectories of test_rollout_vs_oracle: which cascade ran."""
    assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
    env, _ = _rollout(shape, lib_path=COVER_LIB, ref=False)
    counts = _counts(env)
    out = os.environ.get("TMG_EVIDENCE_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"dispatch_cover_{dc.case_id(shape)}.txt"), "w") as f:
            f.write(repr(counts) + "\n")
    assert env.status() == 0
    rp = {s: counts[s] for s in RP_SITES if counts[s]}
    if shape in dc.LEAN_TALL_WIDE:
        assert counts["sb_lean"] > 0, f"{shape}: sb_move never ran (counts {counts})"
        assert not rp, f"{shape}: row-plane sites counted on a shape outside rp_shape: {rp}"
    elif shape == dc.ROW_PLANE_CONTROL:
        # rp_move counts sb_lean per cascade iteration as sb_move does; its own sites tell them apart
        missing = [s for s in ("rp_passes", "rp_perp", "rp_vlong", "rp_carry") if counts[s] == 0]
        assert counts["sb_lean"] > 0 and not missing, f"{shape}: rp_move sites never taken: {missing} (counts {counts})"
        assert counts["lane_step"] == 0, counts
    elif shape[3] == 0 and shape[0] * shape[1] <= 128 and shape[1] <= 28:
        assert counts["sb_lean"] > 0 and rp, f"{shape}: the row-plane cascade never ran (counts {counts})"
    if shape in dc.SHUFFLES:
        assert counts["shuffle"] > 0, f"{shape}: no shuffle inside a move (counts {counts})"
    if shape in dc.WIDE_EXACT:
        # the crafted rejections (words_rejecting_at) land in the step's refill and,
        # before an autoreset, in generate_board's draw-by-draw path
        assert counts["reject"] > 0, f"{shape}: no crafted rejection replayed (counts {counts})"
    env.close()


# ---------------------------------------------------------------- hand-built boards
def _bg(R, C):
    """No line: 1 + (r + c) % 4 differs from every cell at distance 1 and 2 in its row and column (k >= 4)."""
    r, c = np.mgrid[0:R, 0:C]
    return (1 + (r + c) % 4).astype(np.int8)


def _plain(col):
    return np.stack([col, np.ones_like(col)]).astype(np.int8)


def _first(its, pred):
    return bool(its) and any(pred(ln) for ln in its[0])


def crafted():
    """name -> (shape, board (2, R, C) int8, action, seed, feature predicate over
    (iterations of trace_move or None, board after the first detect / resolve))."""
    out = {}
    # 42x3 k3: column 1 holds 1s in rows 5..24 but for row 15, whose 1 comes from (15, 0):
    # one vertical line of 20 cells, longer than a DPP row
    r, c = np.mgrid[0:42, 0:3]
    b = (1 + (r + c) % 3).astype(np.int8)
    b[5:25, 1] = 1
    b[15, 1], b[15, 0] = 2, 1
    b[4, 1], b[25, 1] = 3, 3
    out["vertical_20"] = ((42, 3, 3, 0), _plain(b), haction(15, 0, 42, 3), 11,
                          lambda its, _: _first(its, lambda ln: _vertical(ln) and len(ln) >= 17))
    # 17x7: rowplane_cases' T and plus boards eight rows down (rows past the DPP row's 16 lanes' worth of R)
    b = _bg(17, 7)
    b[14, 4] = b[15, 4] = b[12, 4] = b[13, 3] = b[13, 5] = 3
    b[13, 4], b[11, 4], b[16, 4], b[13, 2], b[13, 6] = 1, 1, 1, 4, 4
    out["T_cross_17"] = ((17, 7, 4, 0), _plain(b), vaction(12, 4, 7), 12, lambda its, _: f_T(its))
    b = _bg(17, 7)
    b[13, 4] = b[14, 4] = b[12, 3] = 4
    b[12, 4] = 1
    b[10, 4] = b[11, 4] = b[15, 4] = b[14, 3] = b[14, 5] = 2
    b[9, 4], b[16, 4], b[14, 2], b[14, 6], b[11, 3], b[11, 5] = 3, 3, 1, 1, 1, 3
    out["plus_cross_17"] = ((17, 7, 4, 0), _plain(b), haction(12, 3, 17, 7), 13, lambda its, _: f_plus(its))
    # 2x63: (1, 60) (1, 61) completed in the last column from (0, 62)
    b = _bg(2, 63)
    b[1, 60] = b[1, 61] = b[0, 62] = 5
    b[1, 62] = 6
    b[0, 10] = b[0, 11] = b[1, 12] = 6              # a move left afterwards: no shuffle, which trace_move does not model
    out["last_column_63"] = ((2, 63, 6, 0), _plain(b), vaction(0, 62, 63), 14,
                             lambda its, _: _first(its, lambda ln: _horizontal(ln) and max(c for _, c in ln) == 62))
    # 4x32: the same in column 31
    b = _bg(4, 32)
    b[3, 29] = b[3, 30] = b[2, 31] = 5
    b[3, 31] = 6
    out["last_column_32"] = ((4, 32, 7, 0), _plain(b), vaction(2, 31, 32), 15,
                             lambda its, _: _first(its, lambda ln: _horizontal(ln) and max(c for _, c in ln) == 31))
    # 4x32: rows 1..3 of columns 8..31 hold one colour but for (1, 15), whose 5 comes from (0, 15):
    # row 3 is a run of 24 with a vertical line ending in it in every column, so one refill
    # draws 72 colours (columns 0..7 stay plain: the mask step needs an ineffective action)
    b = _bg(4, 32)
    b[1:, 8:] = 5
    b[1, 15], b[0, 15] = 6, 5
    out["refill_over_64"] = ((4, 32, 7, 0), _plain(b), vaction(0, 15, 32), 16,
                             lambda its, _: bool(its) and len(_cleared(its[0])) > 64)
    # 17x7, lasers and bombs: a vertical laser at (16, 3) in the run (16, 2..4) clears its column of 17
    b = _plain(_bg(17, 7))
    b[0, 16, 2] = b[0, 16, 3] = b[0, 15, 4] = 1
    b[0, 16, 4], b[0, 16, 1], b[0, 16, 5], b[0, 14, 4] = 2, 3, 3, 3
    b[1, 16, 3] = 2
    out["v_laser_17"] = ((17, 7, 4, 14), b, vaction(15, 4, 7), 17, lambda _, after: (after[1][:, 3] == 0).all())
    # 3x33, every special: a horizontal laser at (2, 11) in the run (2, 10..12) clears its row of 33
    b = _plain(_bg(3, 33))
    b[0, 2, 10] = b[0, 2, 11] = b[0, 1, 12] = 1
    b[0, 2, 12], b[0, 2, 9], b[0, 2, 13], b[0, 0, 12] = 2, 3, 3, 3
    b[1, 2, 11] = 3
    out["h_laser_33"] = ((3, 33, 5, 15), b, vaction(1, 12, 33), 18, lambda _, after: (after[1][2, :] == 0).all())
    return out


def _swapped(board, R, C, a):
    from rowplane_cases import action_cells
    (r1, c1), (r2, c2) = action_cells(R, C, a)
    b = board.copy()
    b[:, r1, c1], b[:, r2, c2] = board[:, r2, c2], board[:, r1, c1]
    return b


@pytest.mark.parametrize("lib", ["product", "cover"])
def test_crafted_tall_wide(lib):
    """Each hand-built board: one untrusted step with an ineffective action
    (the general kernel computes the mask), then the move.  The feature is
    asserted on the oracle's own lines (no specials) or on its first detect /
    resolve (specials) before the device is compared with the oracle.  Two
    boards hold lines before the move (a vertical line of 20 and a refill of
    72 cannot come from one swap on a line-free board); their mask step takes
    an action far from those lines (is_move_effective looks two cells around
    the swap, board.py:735-787), and the move clears them as the oracle does."""
    from tile_match_gym_amd.seeding import batch_rng_words
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    cases = crafted()
    assert sorted({c[0] for c in cases.values()}) == sorted(dc.CRAFTED_SHAPES)
    path = None
    if lib == "cover":
        assert os.path.exists(COVER_LIB), "build() makes libtmg_cover.so"
        path = COVER_LIB
    for nm, (shape, b, a, seed, feature) in sorted(cases.items()):
        R, C, k, sm = shape
        w = batch_rng_words([seed])
        assert orc.effective_mask(b)[0][a], f"{nm}: the move is not effective"
        mb, mrng, res, err = orc.move(b, w[0], a, k, sm)
        assert err == 0, nm
        its = None
        if sm == 0:
            its, fb, rng = trace_move(orc, b, w[0], a, k)
            assert np.array_equal(fb, mb) and np.array_equal(rng, mrng), nm
        after, _, _, derr = orc.detect_resolve(_swapped(b, R, C, a), k, sm)
        assert derr == 0 and feature(its, after), f"{nm}: the oracle's move does not show the feature"
        cl, co = specials(sm)
        env = TileMatchVecEnv(1, R, C, k, 30, cl, co, seeds=[seed], device=DEV, lib_path=path)
        env.reset()
        env.join()
        env.board.copy_(torch.from_numpy(b[None]).to(DEV))
        _set_rng(env, w)
        env.timer.zero_()
        env.invalidate_effective_cache()
        o = orc.OracleBatch(R, C, k, sm, 30, w, threads=1)
        o.board[:] = b[None]
        idle = np.array([int(np.nonzero(~orc.effective_mask(b)[0])[0][0])], np.int32)
        env.step(torch.from_numpy(idle).to(DEV))
        o.step(idle, autoreset=True)
        _same(env, o, f"{nm} mask step")
        if path:
            env.ctx.cover(True)
        act = np.array([a], np.int32)
        env.step(torch.from_numpy(act).to(DEV))
        o.step(act, autoreset=True)
        _same(env, o, f"{nm} move")
        assert o.reward[0] == res[0] >= 3, nm
        assert env.status() == 0, nm
        if path:
            counts = _counts(env)
            if sm == 0:
                assert counts["sb_lean"] >= len(its), (nm, counts)
                assert not any(counts[s] for s in RP_SITES), (nm, counts)
            else:
                assert counts["sb_closure"] + counts["serial_act"] > 0, (nm, counts)
        env.close()
