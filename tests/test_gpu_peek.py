"""tmg_peek on the MI355X: every action's step outcome of every env, without
stepping, against the oracle's Board.move of each (env, action)
(tests/peek_cases.py oracle_peek), never against tmg_step.  Boards are compared
as bytes and counts as integers; nothing here has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import dispatch_cases as dc
import peek_cases
from adversarial import adversarial_boards
from deep_rollouts import COVER_LIB, specials
from oracle import oracle as orc
from peek_cases import assert_peek_equal, oracle_peek

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("reward", "n_new", "n_act", "flags")
STATE = ("board", "rng", "timer", "eff")
STEP_FIELDS = STATE + ("reward", "n_new", "n_act", "flags")


@functools.lru_cache(maxsize=None)
def _rolled(shape, steps, n=None, num_moves=30):
    """The oracle state the tests peek at (shared, never changed: users copy)."""
    n = n or peek_cases.envs_of(shape)
    return peek_cases.rolled_batch(shape, range(500, 500 + n), steps=steps, num_moves=num_moves)


def _env(shape, n, num_moves=30, lib_path=None, **kw):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, sm = shape
    cl, co = specials(sm)
    return TileMatchVecEnv(n, R, C, k, num_moves, cl, co, seeds=range(500, 500 + n), device=DEV, lib_path=lib_path, **kw)


def _load(env, o):
    """Put the oracle's state (boards, RNG words, timers, this library's own masks) on the device."""
    env.load_state_dict({"board": o.board, "rng": o.rng, "timer": o.timer, "eff": o.eff, "eff_valid": True,
                         "config": env.config()})


def _words(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(DEV)


def _host(env, f):
    if f == "rng":
        return env.rng_words()
    v = getattr(env, f).cpu().numpy()
    return v.view(np.uint64) if f == "eff" else v


def _peek(env, rng=None):
    out = env.peek(rng=rng, outputs=ALL, best=True)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items()}


@pytest.mark.parametrize("shape", peek_cases.SHAPES + peek_cases.LIMIT_SHAPES, ids=peek_cases.case_id)
def test_peek_vs_oracle_gpu(shape):
    """After 7 uniform-random steps (boards that hold specials) and after a
    reset, with the envs' own RNG words and with words of other seeds."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k, sm = shape
    n = peek_cases.envs_of(shape)
    env = _env(shape, n)
    other = batch_rng_words(range(7000, 7000 + n))
    for steps in (7, 0):
        o = _rolled(shape, steps)
        _load(env, o)
        assert_peek_equal(_peek(env), oracle_peek(o.board, o.rng, k, sm), f"{shape} steps={steps} own rng")
        assert_peek_equal(_peek(env, _words(other)), oracle_peek(o.board, other, k, sm), f"{shape} steps={steps} other rng")
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)], ids=peek_cases.case_id)
def test_peek_leaves_state_alone(shape):
    o = _rolled(shape, 7)
    env = _env(shape, o.n)
    _load(env, o)
    before = {f: _host(env, f).copy() for f in STATE}
    _peek(env)
    for f in STATE:
        assert np.array_equal(_host(env, f), before[f]), f
        assert np.array_equal(before[f], getattr(o, f)), f
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (8, 8, 3, 15), (20, 20, 6, 15)],
                         ids=peek_cases.case_id)
def test_peek_agrees_with_next_step(shape):
    """Peek, then step one effective action per env (from the oracle's mask):
    the step reports what peek said, both what the oracle says, and the state
    after it is OracleBatch's."""
    R, C, k, sm = shape
    src = _rolled(shape, 7)
    n = src.n
    o = orc.OracleBatch(R, C, k, sm, 30, src.rng.copy())
    o.board[:], o.timer[:], o.eff[:] = src.board, src.timer, src.eff
    env = _env(shape, n)
    _load(env, o)
    mask = np.unpackbits(o.eff.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")[:, :o.A]
    rs = np.random.default_rng(3)
    a = np.array([rs.choice(np.nonzero(mask[i])[0]) for i in range(n)], np.int32)
    got = _peek(env)
    want = oracle_peek(o.board, o.rng, k, sm)
    assert_peek_equal(got, want, str(shape))
    env.step(torch.from_numpy(a).to(DEV))
    o.step(a, autoreset=True)
    for f in STEP_FIELDS:
        assert np.array_equal(_host(env, f), getattr(o, f)), f
    idx = np.arange(n)
    for f in ("reward", "n_new", "n_act"):
        assert np.array_equal(got[f][idx, a], _host(env, f)), f
        assert np.array_equal(got[f][idx, a], getattr(o, f)), f
    assert np.array_equal(got["flags"][idx, a] & 6, _host(env, "flags") & 6)     # combo / shuffled
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape,mode,many", peek_cases.spill_params(device=True))
def test_peek_untrusted_and_spill_gpu(shape, mode, many):
    """Hand-written boards, trust_eff = 0 and no mask given: the general
    kernels, and the spill pass for the envs one of whose actions outgrows the
    LDS lists.  many: more spilling envs than the spill pass has waves."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k, sm = shape
    n = peek_cases.MANY_SPILLS[shape][0] if many else peek_cases.envs_of(shape)
    b = adversarial_boards(n, R, C, k, sm, 11, mode)
    words = batch_rng_words(range(300, 300 + n))
    env = _env(shape, n)
    A = env.num_actions
    board, rng = torch.from_numpy(b).to(DEV), _words(words)
    out = {f: torch.full((n, A), 85, dtype=torch.uint8 if f == "flags" else torch.int32, device=DEV) for f in ALL}
    out.update({f: torch.full((n,), -1, dtype=torch.int32, device=DEV) for f in ("best_action", "best_reward")})
    s0 = env.ctx.spills()
    env.ctx.peek(n, board.data_ptr(), rng.data_ptr(), None, 0, *(out[f].data_ptr() for f in peek_cases.FIELDS),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {f: v.cpu().numpy() for f, v in out.items()}
    assert_peek_equal(got, oracle_peek(b, words, k, sm), f"{shape} {mode}")
    assert env.status() == 0
    if (R, C) in ((20, 20), (10, 10)) and mode != "stripes":
        assert env.ctx.spills() > s0, "the adversarial boards were meant to outgrow the LDS lists"
    if many:
        assert env.ctx.spills() - s0 > peek_cases.SPILL_WAVES
    if mode == "combo_grid":
        assert (got["flags"] & peek_cases.FLAG_COMBO).any()
    assert np.array_equal(board.cpu().numpy(), b) and np.array_equal(rng.cpu().numpy().view(np.uint64), words)
    env.close()


def _counts(env):
    from tile_match_gym_amd import _native
    c = env.ctx.cover(clear=True)
    return {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}


SHUFFLE_ENVS = 16


def test_peek_cover():
    """The TMG_COVER build: an action is simulated on every shape, the spill
    tier runs on the adversarial boards, and the boards of
    dispatch_cases.SHUFFLES shuffle inside peeked moves (counted on the oracle
    first)."""
    for shape in peek_cases.SHAPES:
        o = _rolled(shape, 7)
        env = _env(shape, o.n, lib_path=COVER_LIB)
        _load(env, o)
        _counts(env)
        env.peek()
        c = _counts(env)
        assert c["peek_move"] > 0, shape
        assert c["peek_spill"] == c["peek_spill_run"], shape
        assert env.status() == 0
        env.close()
    shape = (10, 10, 4, 14)
    n = peek_cases.envs_of(shape)
    env = _env(shape, n, lib_path=COVER_LIB)
    env.board.copy_(torch.from_numpy(adversarial_boards(n, *shape, 11, "laser_sea")))
    env.invalidate_effective_cache()
    _counts(env)
    env.peek()
    c = _counts(env)
    assert c["peek_move"] > 0 and c["peek_spill"] > 0 and c["peek_spill_run"] > 0, c
    assert env.status() == 0
    env.close()
    for shape in dc.SHUFFLES:
        o = _rolled(shape, 7, SHUFFLE_ENVS)
        want = oracle_peek(o.board, o.rng, shape[2], shape[3])
        assert (want["flags"] & peek_cases.FLAG_SHUFFLED).any(), f"{shape}: no peeked move shuffles on the oracle"
        env = _env(shape, o.n, lib_path=COVER_LIB)
        _load(env, o)
        _counts(env)
        got = env.peek(outputs=("flags",))["flags"].cpu().numpy()
        c = _counts(env)
        assert c["shuffle"] > 0, shape
        assert np.array_equal(got, want["flags"]), shape
        assert env.status() == 0
        env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14)], ids=peek_cases.case_id)
def test_step_greedy_rollout(shape):
    """14 greedy steps of 8 envs with episodes of 6 moves and same-step
    autoreset, against OracleBatch driven by oracle_peek's best action."""
    R, C, k, sm = shape
    n, moves = 8, 6
    env = _env(shape, n, num_moves=moves)
    o = orc.OracleBatch(R, C, k, sm, moves, env.rng_words().copy())
    env.reset()
    o.reset()
    for t in range(14):
        want = oracle_peek(o.board, o.rng, k, sm)
        best = env.step_greedy()
        env.join()
        o.step(want["best_action"], autoreset=True)
        assert np.array_equal(env.actions.cpu().numpy(), want["best_action"]), t
        assert np.array_equal(best.cpu().numpy(), want["best_reward"]), t
        assert np.array_equal(best.cpu().numpy(), _host(env, "reward")), t
        for f in STEP_FIELDS:
            assert np.array_equal(_host(env, f), getattr(o, f)), (t, f)
    assert env.status() == 0
    env.close()


def test_peek_lean_precondition():
    """A special tile written into a no-specials env with the mask left
    trusted: the lean kernel flags every action of that env and raises
    TMG_STATUS_INTERNAL; the other envs still equal the oracle."""
    from tile_match_gym_amd import _native
    shape = (10, 10, 4, 0)
    R, C, k, sm = shape
    o = _rolled(shape, 0)
    env = _env(shape, o.n)
    _load(env, o)
    bad = 1
    env.board[bad, 1, 4, 5] = 2                 # a vertical laser; _eff_valid stays set
    got = _peek(env)
    want = oracle_peek(o.board, o.rng, k, sm)
    assert (got["flags"][bad] & peek_cases.FLAG_ERROR).all()
    assert env.status(clear=True) & _native.STATUS_INTERNAL
    ok = np.arange(o.n) != bad
    assert_peek_equal({f: got[f][ok] for f in peek_cases.FIELDS}, {f: want[f][ok] for f in peek_cases.FIELDS}, "other envs")
    env.close()


def test_single_env_peek():
    """TileMatchEnv.peek: numpy arrays of shape (A,), the env left as it was."""
    from tile_match_gym_amd.tile_match_env import TileMatchEnv
    env = TileMatchEnv(8, 8, 4, 10, [], ["vertical_laser", "horizontal_laser", "bomb"], seed=5, device=DEV)
    env.reset()
    board, words = env.board.board.copy(), env.board.rng_words.copy()
    got = env.peek()
    want = oracle_peek(board.astype(np.int8)[None], words[None], 4, 14)
    assert got["reward"].shape == (env.num_actions,)
    assert np.array_equal(got["reward"], want["reward"][0])
    assert np.array_equal(got["num_new_specials"], want["n_new"][0])
    assert np.array_equal(got["num_specials_activated"], want["n_act"][0])
    assert np.array_equal(got["shuffled"], (want["flags"][0] & peek_cases.FLAG_SHUFFLED) != 0)
    assert np.array_equal(env.board.board, board) and np.array_equal(env.board.rng_words, words)
    env.close()
