"""tmg_rollout on the MI355X: every action's policy rollout of every env and
sample, without stepping, against the oracle's moves and policy draws of each
(sample, env, action) (tests/rollout_cases.py oracle_rollout), never against
tmg_step.  Boards are compared as bytes and counts as integers; nothing here
has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import dispatch_cases as dc
import peek_cases
import rollout_cases as rc
from adversarial import adversarial_boards
from deep_rollouts import COVER_LIB, specials
from oracle import oracle as orc
from peek_cases import oracle_peek
from rollout_cases import assert_rollout_equal, oracle_rollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("ret", "plies", "flags", "total")
STATE = ("board", "rng", "timer", "eff")
STEP_FIELDS = STATE + ("reward", "n_new", "n_act", "flags")
MOVES = 30
POLICY = dict(key=rc.KEY, first_env=rc.FIRST_ENV, t=rc.T)


@functools.lru_cache(maxsize=None)
def _rolled(shape, steps, n=None):
    """The oracle state the tests roll out from (shared, never changed: users copy)."""
    n = n or peek_cases.envs_of(shape)
    return peek_cases.rolled_batch(shape, range(500, 500 + n), steps=steps, num_moves=MOVES)


def _env(shape, n, num_moves=MOVES, lib_path=None, **kw):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, sm = shape
    cl, co = specials(sm)
    return TileMatchVecEnv(n, R, C, k, num_moves, cl, co, seeds=range(500, 500 + n), device=DEV, lib_path=lib_path, **kw)


def _load(env, o, timer=None):
    """Put the oracle's state (boards, RNG words, timers, this library's own masks) on the device."""
    env.load_state_dict({"board": o.board, "rng": o.rng, "timer": o.timer if timer is None else timer, "eff": o.eff,
                         "eff_valid": True, "config": env.config()})


def _words(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(DEV)


def _host(env, f):
    if f == "rng":
        return env.rng_words()
    v = getattr(env, f).cpu().numpy()
    return v.view(np.uint64) if f == "eff" else v


def _rollout(env, depth, samples=1, rng=None, **kw):
    out = env.rollout(depth, samples, rng=rng, outputs=ALL, best=True, **dict(POLICY, **kw))
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items()}


def _want(o, rng, timer, depth, samples):
    return oracle_rollout(o.board, rng, timer, o.num_moves, o.k, o.smask, depth, samples, rc.KEY, rc.FIRST_ENV, rc.T)


@pytest.mark.parametrize("shape", peek_cases.SHAPES + peek_cases.LIMIT_SHAPES, ids=peek_cases.case_id)
def test_rollout_vs_oracle_gpu(shape):
    """After 7 uniform-random steps (boards that hold specials) and after a
    reset; env 0 two moves from the end of its episode and, after the reset,
    the last env at its end; sample 0 with the envs' own RNG words, sample 1
    with words of other seeds."""
    from tile_match_gym_amd.seeding import batch_rng_words
    n = peek_cases.envs_of(shape)
    env = _env(shape, n)
    other = batch_rng_words(range(7000, 7000 + n))
    depth, samples = 4, 2
    for steps in (7, 0):
        o = _rolled(shape, steps)
        timer = rc.horizon_timers(o, finished=steps == 0)
        _load(env, o, timer)
        rng = np.stack([o.rng, other])
        got = _rollout(env, depth, samples, _words(rng))
        assert_rollout_equal(got, _want(o, rng, timer, depth, samples), f"{shape} steps={steps}")
        assert (got["plies"][:, 0] <= 2).all() and (got["plies"][:, 0] == 2).any()
        if steps == 0:
            assert not got["plies"][:, -1].any()
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)], ids=peek_cases.case_id)
def test_rollout_depth1_is_peek_gpu(shape):
    """depth 1, one sample, the envs' own words: the oracle's peek, and tmg_peek's arrays."""
    R, C, k, sm = shape
    o = _rolled(shape, 7)
    env = _env(shape, o.n)
    _load(env, o)
    got = _rollout(env, 1)
    want = oracle_peek(o.board, o.rng, k, sm)
    assert np.array_equal(got["ret"][0], want["reward"])
    assert np.array_equal(got["flags"][0], want["flags"])
    assert np.array_equal(got["total"], want["reward"])
    assert np.array_equal(got["best_action"], want["best_action"])
    assert np.array_equal(got["best_total"], want["best_reward"])
    peeked = env.peek(outputs=("reward", "flags"))
    assert np.array_equal(got["ret"][0], peeked["reward"].cpu().numpy())
    assert np.array_equal(got["flags"][0], peeked["flags"].cpu().numpy())
    assert env.status() == 0
    env.close()


def test_rollout_no_horizon_gpu():
    shape = (8, 8, 3, 15)
    o = _rolled(shape, 7)
    env = _env(shape, o.n)
    timer = o.timer.copy()
    timer[1] = MOVES                            # not passed on: the rollouts of env 1 run to the full depth too
    _load(env, o, timer)
    depth = 5
    got = _rollout(env, depth, horizon=False)
    assert_rollout_equal(got, _want(o, o.rng[None], None, depth, 1), str(shape))
    mask = np.stack([orc.effective_mask(o.board[i])[0] for i in range(o.n)])
    assert np.array_equal(got["plies"][0], np.where(mask, depth, 0))
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)], ids=peek_cases.case_id)
def test_rollout_leaves_state_alone(shape):
    from tile_match_gym_amd.seeding import batch_rng_words
    o = _rolled(shape, 7)
    env = _env(shape, o.n)
    _load(env, o)
    other = _words(np.stack([batch_rng_words(range(7000, 7000 + o.n)), batch_rng_words(range(7100, 7100 + o.n))]))
    before = {f: _host(env, f).copy() for f in STATE}
    words = other.clone()
    _rollout(env, 3)
    _rollout(env, 3, 2, other)
    for f in STATE:
        assert np.array_equal(_host(env, f), before[f]), f
        assert np.array_equal(before[f], getattr(o, f)), f
    assert torch.equal(other, words)
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14)], ids=peek_cases.case_id)
def test_rollout_agrees_with_real_steps(shape):
    """Env i alone in a 1-env batch, stepped for real: a_i, then the policy's
    steps with key + a_i, first_env + i and t + d.  The summed rewards are the
    rollout's return, and the final state is OracleBatch's, driven the same way."""
    R, C, k, sm = shape
    src = _rolled(shape, 7)
    n, depth, big = src.n, 4, 1000
    env = _env(shape, n)
    _load(env, src)
    got = _rollout(env, depth)
    env.close()
    mask = np.unpackbits(src.eff.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")[:, :src.A]
    rs = np.random.default_rng(3)
    one = _env(shape, 1, num_moves=big)
    for i in range(n):
        a = int(rs.choice(np.nonzero(mask[i])[0]))
        o = orc.OracleBatch(R, C, k, sm, big, src.rng[i:i + 1].copy())
        o.board[:], o.eff[:] = src.board[i:i + 1], src.eff[i:i + 1]
        _load(one, o)
        one.step(torch.tensor([a], dtype=torch.int32, device=DEV))
        o.step(np.array([a], np.int32), autoreset=True)
        total = int(one.reward.item())
        for d in range(1, depth):
            from oracle.policy_np import sample_effective_np
            act = sample_effective_np(o.eff, o.A, rc.KEY + a, rc.FIRST_ENV + i, rc.T + d)
            one.step_effective(rc.T + d, key=rc.KEY + a, first_env=rc.FIRST_ENV + i)
            one.join()
            o.step(act, autoreset=True)
            assert np.array_equal(one.actions.cpu().numpy(), act), (i, d)
            total += int(one.reward.item())
        assert total == got["ret"][0, i, a], (i, a)
        assert got["plies"][0, i, a] == depth
        for f in STATE:
            assert np.array_equal(_host(one, f), getattr(o, f)), (i, f)
    assert one.status() == 0
    one.close()


@pytest.mark.parametrize("shape,mode,many", peek_cases.spill_params(device=True))
def test_rollout_untrusted_and_spill_gpu(shape, mode, many):
    """Hand-written boards, trust_eff = 0 and no mask given, through
    Context.rollout: the general kernels, and the spill pass for the virtual
    envs one of whose plies outgrows the LDS lists.  many: more spilling
    virtual envs than the spill pass has waves."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k, sm = shape
    n = peek_cases.MANY_SPILLS[shape][1] if many else peek_cases.envs_of(shape)
    depth, samples = 2 if many else 3, 2
    b = adversarial_boards(n, R, C, k, sm, 11, mode)
    words = np.stack([batch_rng_words(range(300, 300 + n)), batch_rng_words(range(340, 340 + n))])
    env = _env(shape, n)
    A = env.num_actions
    board, rng = torch.from_numpy(b).to(DEV), _words(words)
    out = {f: torch.full((samples, n, A), 85, dtype=torch.uint8 if f == "flags" else torch.int32, device=DEV)
           for f in ("ret", "plies", "flags")}
    out["total"] = torch.full((n, A), -1, dtype=torch.int32, device=DEV)
    out.update({f: torch.full((n,), -1, dtype=torch.int32, device=DEV) for f in ("best_action", "best_total")})
    s0 = env.ctx.spills()
    env.ctx.rollout(n, board.data_ptr(), rng.data_ptr(), None, None, 0, depth, samples, rc.KEY, rc.FIRST_ENV, rc.T,
                    *(out[f].data_ptr() for f in rc.FIELDS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {f: v.cpu().numpy() for f, v in out.items()}
    want = oracle_rollout(b, words, None, MOVES, k, sm, depth, samples, rc.KEY, rc.FIRST_ENV, rc.T)
    assert_rollout_equal(got, want, f"{shape} {mode}")
    assert env.status() == 0
    if (R, C) in ((20, 20), (10, 10)) and mode != "stripes":
        assert env.ctx.spills() > s0, "the adversarial boards were meant to outgrow the LDS lists"
    if many:
        assert env.ctx.spills() - s0 > peek_cases.SPILL_WAVES
    if mode == "combo_grid":
        assert (got["flags"] & rc.FLAG_COMBO).any()
    assert np.array_equal(board.cpu().numpy(), b) and np.array_equal(rng.cpu().numpy().view(np.uint64), words)
    env.close()


def _counts(env):
    from tile_match_gym_amd import _native
    c = env.ctx.cover(clear=True)
    return {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}


SHUFFLE_ENVS = 16


def test_rollout_cover():
    """The TMG_COVER build: continuation plies and timer-shortened rollouts on
    every shape, the spill tier on the adversarial boards, and the boards of
    dispatch_cases.SHUFFLES shuffle inside continuation plies (asserted on the
    oracle first)."""
    for shape in peek_cases.SHAPES:
        o = _rolled(shape, 7)
        env = _env(shape, o.n, lib_path=COVER_LIB)
        _load(env, o, rc.horizon_timers(o, finished=False))
        _counts(env)
        env.rollout(3, **POLICY)
        c = _counts(env)
        assert c["roll_ply"] > 0 and c["roll_horizon"] > 0, (shape, c)
        assert c["roll_spill"] == c["roll_spill_run"], shape
        assert env.status() == 0
        env.close()
    shape = (10, 10, 4, 14)
    n = peek_cases.envs_of(shape)
    env = _env(shape, n, lib_path=COVER_LIB)
    env.board.copy_(torch.from_numpy(adversarial_boards(n, *shape, 11, "laser_sea")))
    env.invalidate_effective_cache()
    _counts(env)
    env.rollout(2, **POLICY)
    c = _counts(env)
    assert c["roll_ply"] > 0 and c["roll_spill"] > 0 and c["roll_spill"] == c["roll_spill_run"], c
    assert env.status() == 0
    env.close()
    depth = 4
    for shape in dc.SHUFFLES:
        o = _rolled(shape, 7, SHUFFLE_ENVS)
        at = []
        want = oracle_rollout(o.board, o.rng[None], o.timer, MOVES, shape[2], shape[3], depth, 1, rc.KEY, rc.FIRST_ENV,
                              rc.T, shuffled_at=at)
        assert any(d >= 1 for d in at), f"{shape}: no continuation ply shuffles on the oracle"
        env = _env(shape, o.n, lib_path=COVER_LIB)
        _load(env, o)
        _counts(env)
        got = env.rollout(depth, outputs=("flags",), **POLICY)["flags"].cpu().numpy()
        c = _counts(env)
        assert c["shuffle"] > 0 and c["roll_ply"] > 0, shape
        assert np.array_equal(got, want["flags"]), shape
        assert env.status() == 0
        env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14)], ids=peek_cases.case_id)
def test_step_rollout_greedy(shape):
    """10 rollout-greedy steps of 8 envs with episodes of 6 moves and same-step
    autoreset, against OracleBatch driven by oracle_rollout's best action."""
    R, C, k, sm = shape
    n, moves, depth = 8, 6, 3
    env = _env(shape, n, num_moves=moves)
    o = orc.OracleBatch(R, C, k, sm, moves, env.rng_words().copy())
    env.reset()
    o.reset()
    for t in range(10):
        want = oracle_rollout(o.board, o.rng[None], o.timer, moves, k, sm, depth, 1, rc.KEY, rc.FIRST_ENV, t)
        best = env.step_rollout_greedy(depth, key=rc.KEY, first_env=rc.FIRST_ENV, t=t)
        env.join()
        o.step(want["best_action"], autoreset=True)
        assert np.array_equal(env.actions.cpu().numpy(), want["best_action"]), t
        assert np.array_equal(best.cpu().numpy(), want["best_total"]), t
        for f in STEP_FIELDS:
            assert np.array_equal(_host(env, f), getattr(o, f)), (t, f)
    assert env.status() == 0
    env.close()


def test_rollout_lean_precondition():
    """A special tile written into a no-specials env with the mask left
    trusted: the lean kernel flags every action of that env in every sample
    and raises TMG_STATUS_INTERNAL; the other envs still equal the oracle."""
    from tile_match_gym_amd import _native
    from tile_match_gym_amd.seeding import batch_rng_words
    shape = (10, 10, 4, 0)
    o = _rolled(shape, 0)
    env = _env(shape, o.n)
    _load(env, o)
    bad = 1
    env.board[bad, 1, 4, 5] = 2                 # a vertical laser; _eff_valid stays set
    depth, samples = 3, 2
    rng = np.stack([o.rng, batch_rng_words(range(7000, 7000 + o.n))])
    got = _rollout(env, depth, samples, _words(rng))
    want = _want(o, rng, o.timer, depth, samples)
    assert (got["flags"][:, bad] & rc.FLAG_ERROR).all()
    assert env.status(clear=True) & _native.STATUS_INTERNAL
    ok = np.arange(o.n) != bad
    for f in ("ret", "plies", "flags"):
        assert np.array_equal(got[f][:, ok], want[f][:, ok]), f
    for f in ("total", "best_action", "best_total"):
        assert np.array_equal(got[f][ok], want[f][ok]), f
    env.close()


def test_single_env_rollout():
    """TileMatchEnv.rollout: numpy arrays of shape (S, A), the env left as it was."""
    from tile_match_gym_amd.seeding import batch_rng_words
    from tile_match_gym_amd.tile_match_env import TileMatchEnv
    moves, depth = 10, 4
    env = TileMatchEnv(8, 8, 4, moves, [], ["vertical_laser", "horizontal_laser", "bomb"], seed=5, device=DEV)
    env.reset()
    board, words = env.board.board.copy(), env.board.rng_words.copy()
    b8, timer = board.astype(np.int8)[None], np.array([env.timer], np.int32)
    got = env.rollout(depth)
    want = oracle_rollout(b8, words[None, None], timer, moves, 4, 14, depth, 1, 12345, 0, 0)
    assert got["ret"].shape == (1, env.num_actions)
    assert np.array_equal(got["ret"], want["ret"][:, 0]) and np.array_equal(got["plies"], want["plies"][:, 0])
    assert np.array_equal(got["shuffled"], (want["flags"][:, 0] & rc.FLAG_SHUFFLED) != 0)
    seeds = [11, 12, 13]
    got = env.rollout(depth, samples=3, seeds=seeds, key=7, t=2)
    want = oracle_rollout(b8, batch_rng_words(seeds)[:, None], timer, moves, 4, 14, depth, 3, 7, 0, 2)
    assert got["ret"].shape == (3, env.num_actions)
    assert np.array_equal(got["ret"], want["ret"][:, 0]) and np.array_equal(got["plies"], want["plies"][:, 0])
    assert np.array_equal(got["is_combination_match"], (want["flags"][:, 0] & rc.FLAG_COMBO) != 0)
    assert np.array_equal(env.board.board, board) and np.array_equal(env.board.rng_words, words)
    env.close()


def test_rollout_bad_arguments():
    from tile_match_gym_amd import _native
    shape = (10, 10, 4, 0)
    o = _rolled(shape, 0)
    env = _env(shape, o.n)
    _load(env, o)
    n, A = o.n, env.num_actions
    with pytest.raises(ValueError, match="depth"):
        env.rollout(0)
    with pytest.raises(ValueError, match="samples"):
        env.rollout(2, samples=0)
    with pytest.raises(ValueError, match="samples == 1"):
        env.rollout(2, samples=2)
    with pytest.raises(ValueError, match="rng must be"):
        env.rollout(2, samples=2, rng=torch.zeros((n, 5), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="rng must be"):
        env.rollout(2, rng=torch.zeros((n, 4), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="unknown rollout output"):
        env.rollout(2, outputs=("reward",))
    # the C ABI's own checks
    total = torch.zeros((n, A), dtype=torch.int32, device=DEV)
    ret = torch.zeros((1, n, A), dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (n, env.board.data_ptr(), env.rng.data_ptr(), env.timer.data_ptr(), env.eff.data_ptr(), 1)
    with pytest.raises(_native.TmgError, match="need ret"):
        env.ctx.rollout(*args, 2, 1, 0, 0, 0, None, None, None, total.data_ptr(), None, None, stream)
    with pytest.raises(_native.TmgError, match="depth"):
        env.ctx.rollout(*args, 0, 1, 0, 0, 0, ret.data_ptr(), None, None, None, None, None, stream)
    with pytest.raises(_native.TmgError, match="samples"):
        env.ctx.rollout(*args, 2, 0, 0, 0, 0, ret.data_ptr(), None, None, None, None, None, stream)
    with pytest.raises(_native.TmgError, match="n \\* samples"):
        env.ctx.rollout(*args, 2, 2 ** 30, 0, 0, 0, ret.data_ptr(), None, None, None, None, None, stream)
    env.ctx.rollout(0, None, None, None, None, 1, 2, 1, 0, 0, 0, None, None, None, None, None, None, stream)   # n == 0: a no-op
    assert env.status() == 0
    env.close()
