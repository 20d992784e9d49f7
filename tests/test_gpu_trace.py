"""tmg_trace on the MI355X: one move's cascade stage by stage on copies of every
env, against the stage-by-stage walk of the oracle's primitives
(tests/trace_cases.py oracle_trace), never against tmg_step but where a test
says so (the last frame is the stepped board).  Boards are compared as bytes
and counts as integers; nothing here has a tolerance.  The checks are shared
with the host wave emulator's file (tests/test_trace_emulated.py):
trace_cases.check_*; every call they make has its arrays between guard rows."""
import numpy as np
import pytest
import torch

import peek_cases
import trace_cases as tc
from deep_rollouts import specials
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MOVES = 30
# tmg_trace's output pointers, in the order of its parameters (include/tmg.h)
ABI_ORDER = ("frames", "kind", "frame_elim", "n_frames", "reward", "n_new", "n_act", "flags", "out_rng")
assert sorted(ABI_ORDER) == sorted(tc.FIELDS)


def _t(a):
    a = np.array(a, order="C")                                   # a writable copy: torch takes no read-only array
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


class GpuDev:
    """trace_cases' `dev` on the library: one context per shape, kept."""

    def __init__(self):
        self.ctxs = {}

    def ctx(self, shape):
        from tile_match_gym_amd import _native
        if shape not in self.ctxs:
            R, C, k, sm = shape
            self.ctxs[shape] = _native.Context(0, R, C, k, sm, 1 << 20)
        return self.ctxs[shape]

    def run(self, shape, board, rng, eff, trust_eff, actions, stage_mask, max_frames, stop, bufs, lead):
        ctx = self.ctx(shape)
        Q, n = actions.shape
        d = {f: _t(a) for f, a in bufs.items()}
        ins = [_t(board), _t(rng), None if eff is None else _t(eff), _t(actions)]
        ptr = {f: t[lead:].data_ptr() for f, t in d.items()}
        ctx.trace(n, _p(ins[0]), _p(ins[1]), _p(ins[2]), trust_eff, Q, _p(ins[3]), stage_mask, max_frames, stop,
                  *(ptr.get(f) for f in ABI_ORDER), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for f, t in d.items():
            h = t.cpu().numpy()
            bufs[f][...] = h.view(bufs[f].dtype) if h.dtype != bufs[f].dtype else h
        for x, t in zip((board, rng, eff, actions), ins):          # what the device holds now: trace() compares it
            if x is not None:
                h = t.cpu().numpy()
                x[...] = h.view(x.dtype) if h.dtype != x.dtype else h

    def status_clear(self, shape):
        return self.ctx(shape).status(clear=True)

    def spills(self, shape):
        return self.ctx(shape).spills()

    def step(self, shape, board, rng, actions):
        ctx = self.ctx(shape)
        n = board.shape[0]
        b, g, a = _t(board), _t(rng), _t(np.asarray(actions, np.int32))
        timer = torch.zeros(n, dtype=torch.int32, device=DEV)
        eff = torch.zeros((n, ctx.mask_words), dtype=torch.int64, device=DEV)
        out = torch.zeros((3, n), dtype=torch.int32, device=DEV)
        flags = torch.zeros(n, dtype=torch.uint8, device=DEV)
        ctx.step(n, _p(b), _p(g), _p(timer), _p(a), _p(out[0]), _p(out[1]), _p(out[2]), _p(flags), _p(eff), 0, 0,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        return b.cpu().numpy(), g.cpu().numpy().view(np.uint64), o[0], o[1], o[2], flags.cpu().numpy()

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def dev():
    d = GpuDev()
    yield d
    d.close()


@pytest.mark.parametrize("shape", tc.FIELD_SHAPES + tc.LIMIT_SHAPES, ids=tc.case_id)
def test_trace_vs_oracle_gpu(dev, shape):
    tc.check_fields(dev, shape)


@pytest.mark.parametrize("shape", tc.STEP_SHAPES, ids=tc.case_id)
def test_trace_last_frame_is_the_stepped_board_gpu(dev, shape):
    tc.check_step(dev, shape)


@pytest.mark.parametrize("max_frames", tc.CUT_FRAMES)
@pytest.mark.parametrize("stage_mask", tc.CUT_MASKS, ids=lambda m: f"mask{m:#x}")
@pytest.mark.parametrize("shape", tc.CUT_SHAPES, ids=tc.case_id)
def test_trace_masks_and_cuts_gpu(dev, shape, stage_mask, max_frames):
    tc.check_cut(dev, shape, stage_mask, max_frames)


@pytest.mark.parametrize("shape,mode,many", peek_cases.spill_params(device=True))
def test_trace_untrusted_and_spill_gpu(dev, shape, mode, many):
    tc.check_adversarial(dev, shape, mode, many)


@pytest.mark.parametrize("seqs", tc.EXTENT_SEQS)
@pytest.mark.parametrize("n", tc.EXTENT_N)
@pytest.mark.parametrize("shape", [tc.EXTENT_SHAPE, tc.EXTENT_ODD_SHAPE], ids=tc.case_id)
def test_trace_extent_gpu(dev, shape, n, seqs):
    tc.check_extent(dev, shape, n, seqs)


def test_trace_refusals_and_noops_gpu(dev):
    """Each refusal of the contract's list, a tmg_create_scan context, and n == 0."""
    from tile_match_gym_amd import _native
    shape = (10, 10, 4, 14)
    R, C, k, sm = shape
    ctx = dev.ctx(shape)
    board, rng, acts, want = tc.field_case(shape)
    n, Q, F = board.shape[0], acts.shape[0], 4
    d_board, d_rng, d_acts, d_eff = _t(board), _t(rng), _t(acts), _t(tc.masks_of(board))
    rew = torch.full((Q, n), -7, dtype=torch.int32, device=DEV)
    fr = torch.zeros(Q * n * F * 2 * R * C + 8, dtype=torch.int8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(c=ctx, n=n, board=d_board, rng=d_rng, eff=d_eff, trust=1, q=Q, acts=d_acts, mask=tc.ALL_STAGES, F=F,
             frames=None):
        try:
            c.trace(n, _p(board), _p(rng), _p(eff), trust, q, _p(acts), mask, F, 0, frames, None, None, None, _p(rew),
                    None, None, None, None, stream)
        except _native.TmgError:
            return False
        return True

    assert call()
    torch.cuda.synchronize()
    assert np.array_equal(rew.cpu().numpy(), want["reward"])
    assert not call(n=-1) and not call(q=0) and not call(F=0)
    assert not call(mask=0) and not call(mask=1) and not call(mask=1 << 7) and not call(mask=tc.ALL_STAGES | 0x100)
    assert not call(n=2 ** 26 - 8, q=2)
    assert not call(board=None) and not call(rng=None) and not call(acts=None)
    assert not call(eff=None) and call(eff=None, trust=0)
    assert not call(frames=fr.data_ptr() + 2) and call(frames=fr.data_ptr())
    scan = _native.Context(0, R, C, scan_only=True)
    assert not call(c=scan)
    scan.close()
    torch.cuda.synchronize()
    rew.fill_(-7)
    assert call(n=0, board=None, rng=None, acts=None, eff=None)
    torch.cuda.synchronize()
    assert (rew.cpu().numpy() == -7).all()
    assert ctx.status(clear=True) == _native.STATUS_CALLER           # the action row that holds A


# ---------------------------------------------------------------- the Python surface
def _env(shape, n, **kw):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, sm = shape
    cl, co = specials(sm)
    return TileMatchVecEnv(n, R, C, k, MOVES, cl, co, seeds=range(500, 500 + n), device=DEV, **kw)


def _state(env):
    return [env.board.cpu().numpy().copy(), env.rng_words().copy(), env.timer.cpu().numpy().copy(),
            env.eff.cpu().numpy().copy()]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", [(4, 4, 3, 0), (10, 10, 4, 14)], ids=tc.case_id)
def test_vec_env_trace_and_afterstates(shape):
    """TileMatchVecEnv.trace with (N,) and (Q, N) actions and afterstates()
    against the walk; board, RNG words, timer and mask unchanged after each."""
    R, C, k, sm = shape
    n = 4
    env = _env(shape, n)
    env.reset()
    rs = np.random.default_rng(3)
    for _ in range(5):
        env.step_raw(_t(rs.integers(0, env.num_actions, n).astype(np.int32)))
    env.join()
    before = _state(env)
    board, rng = before[0], before[1]
    A = env.num_actions
    acts = np.stack([np.array([tc.greedy_action(board[i], rs) for i in range(n)]), rs.integers(0, A, n)]).astype(np.int32)
    for a in (acts[0], acts):
        a2 = np.atleast_2d(a)
        out = env.trace(_t(a), stages=("swap", "combo", "clear", "fall", "refill", "shuffle"), max_frames=tc.WHOLE)
        torch.cuda.synchronize()
        got = {f: v.cpu().numpy() for f, v in out.items()}
        want = tc.expected(board, rng, a2, k, sm, tc.ALL_STAGES, tc.WHOLE, 0)
        written = np.arange(tc.WHOLE)[None, None, :] < np.minimum(want["n_frames"], tc.WHOLE)[:, :, None]
        assert np.array_equal(got["frames"][written], want["frames"][written])
        tc.assert_trace_equal(got, want, str(shape), tc.SMALL)
        assert _same(_state(env), before)
    out = env.trace(_t(acts[0]))                                   # the defaults: clear / fall / refill, 16 frames
    torch.cuda.synchronize()
    want = tc.expected(board, rng, acts[:1], k, sm, tc.DEFAULT_STAGES, 16, 0)
    tc.assert_trace_equal({f: v.cpu().numpy() for f, v in out.items()}, want, str(shape), tc.SMALL)
    assert out["frames"].shape == (1, n, 16, 2, R, C) and env.trace(_t(acts[0]), frames=False)["frames"] is None
    # every action's afterstate
    boards, reward, effective = env.afterstates()
    torch.cuda.synchronize()
    assert _same(_state(env), before)
    boards, reward, effective = boards.cpu().numpy(), reward.cpu().numpy(), effective.cpu().numpy()
    assert boards.shape == (A, n, 2, R, C) and reward.shape == (A, n) and effective.dtype == np.bool_
    for i in range(n):
        mask = orc.effective_mask(board[i])[0]
        assert np.array_equal(effective[:, i], mask)
        for a in range(A):
            stages = tc.oracle_trace(board[i], rng[i], a, k, sm)[0]
            if not stages:
                assert np.array_equal(boards[a, i], board[i]) and reward[a, i] == 0
                continue
            j = next(j for j, s in enumerate(stages) if s.kind == tc.FALL)
            assert np.array_equal(boards[a, i], stages[j].board), (i, a)
            assert reward[a, i] == sum(s.elim for s in stages[:j + 1]) + stages[j].n_new, (i, a)
    some, r2, e2 = env.afterstates(_t(acts))
    torch.cuda.synchronize()
    assert np.array_equal(some.cpu().numpy(), boards[acts, np.arange(n)[None, :]])
    assert np.array_equal(r2.cpu().numpy(), reward[acts, np.arange(n)[None, :]])
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(4, 4, 3, 0), (10, 10, 4, 14)], ids=tc.case_id)
def test_single_env_trace(shape):
    """TileMatchEnv.trace against the walk; the env is unchanged, and the step
    that follows reports the traced results and leaves the last frame."""
    from tile_match_gym_amd.tile_match_env import TileMatchEnv
    R, C, k, sm = shape
    cl, co = specials(sm)
    env = TileMatchEnv(R, C, k, MOVES, cl, co, seed=5, device=DEV)
    env.reset()
    rs = np.random.default_rng(9)
    for _ in range(3):
        board = np.asarray(env.board.board, np.int8).copy()
        words = env.board.rng_words.copy()
        timer = env.timer
        mask = orc.effective_mask(board)[0]
        a = int(rs.choice(np.nonzero(mask)[0]))
        dead = int(np.nonzero(~mask)[0][0])
        frames, res = env.trace(a)
        assert np.array_equal(np.asarray(env.board.board, np.int8), board) and env.timer == timer
        assert np.array_equal(env.board.rng_words, words)
        assert env.trace(dead) == ([], (0, False, 0, 0, False))
        stages, _, _, wres = tc.oracle_trace(board, words, a, k, sm)
        assert [f[0] for f in frames] == [tc.STAGE_NAMES[s.kind] for s in stages]
        assert all(np.array_equal(f[1], s.board) and f[1].dtype == np.int32 and f[2] == s.elim
                   for f, s in zip(frames, stages))
        assert res == (wres[0], bool(wres[1]), wres[2], wres[3], bool(wres[4]))
        assert frames[0][0] == "swap" and sum(f[2] for f in frames) + res[2] == res[0]
        only = env.trace(a, stages=("clear",))[0]
        assert [f[0] for f in only] == ["clear"] * len(only) and len(only) == sum(f[0] == "clear" for f in frames)
        _, reward, _, _, info = env.step(a)
        assert reward == res[0] and np.array_equal(np.asarray(env.board.board), frames[-1][1])
    env.close()
