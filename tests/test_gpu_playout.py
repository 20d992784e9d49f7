"""tmg_playout on the MI355X: given action sequences played on copies of every
env, against the oracle's mask and move of every (sequence, env, ply)
(tests/playout_cases.py oracle_playout), never against tmg_step but where a
test says so (agreement with real steps).  Boards are compared as bytes and
counts as integers; nothing here has a tolerance.  The cases that need no
device run on the host wave emulator too (tests/test_playout_emulated.py)."""
import numpy as np
import pytest
import torch

import extent_cases as ec
import peek_cases
import playout_cases as pc
from deep_rollouts import specials
from oracle import oracle as orc
from peek_cases import oracle_peek
from playout_cases import assert_playout_equal, oracle_playout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MOVES = pc.MOVES
STATE = ("board", "rng", "timer", "eff")
OUTS = ("ret", "n_new", "n_act", "plies", "flags", "ply_reward")


def _env(shape, n, num_moves=MOVES, **kw):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, sm = shape
    cl, co = specials(sm)
    return TileMatchVecEnv(n, R, C, k, num_moves, cl, co, seeds=range(500, 500 + n), device=DEV, **kw)


def _load(env, o, timer=None):
    """Put the oracle's state (boards, RNG words, timers, this library's own masks) on the device."""
    env.load_state_dict({"board": o.board, "rng": o.rng, "timer": np.array(o.timer if timer is None else timer), "eff": o.eff,
                         "eff_valid": True, "config": env.config()})


def _dev(a):
    a = np.array(a, order="C")                                   # a writable copy: torch takes no read-only array
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def _host(env, f):
    if f == "rng":
        return env.rng_words()
    v = getattr(env, f).cpu().numpy()
    return v.view(np.uint64) if f == "eff" else v


def _playout(env, acts, rng=None):
    """env.playout with every output; the final rows as out_board / out_rng / out_timer / out_eff.
    acts / rng: numpy arrays, or device tensors the caller keeps."""
    acts, rng = (x if x is None or torch.is_tensor(x) else _dev(x) for x in (acts, rng))
    out = env.playout(acts, rng=rng, outputs=OUTS, best=True, final=True)
    torch.cuda.synchronize()
    got = {f: v.cpu().numpy() for f, v in out.items() if f != "env"}
    child = out["env"]
    got.update(out_board=_host(child, "board"), out_rng=_host(child, "rng"), out_timer=_host(child, "timer"),
               out_eff=_host(child, "eff"))
    return got, child


@pytest.mark.parametrize("shape", peek_cases.SHAPES + peek_cases.LIMIT_SHAPES, ids=pc.case_id)
def test_playout_vs_oracle_gpu(shape):
    """Case 1, and case 3 on the same calls: the emulated test's states and
    sequences.  Every output and final-state array; nothing of board / rng /
    timer / eff / actions is written."""
    env = _env(shape, peek_cases.envs_of(shape))
    for steps in (7, 0):
        case = pc.vs_oracle_case(shape, steps)
        o, timer, acts, rng, want, _ = case
        pc.check_vs_oracle_conditions(shape, case)
        _load(env, o, timer)
        d_acts, d_rng = _dev(acts), _dev(rng)
        got, _ = _playout(env, d_acts, d_rng)
        assert_playout_equal(got, want, f"{shape} steps={steps}")
        for f, w in zip(STATE, (o.board, o.rng, timer, o.eff)):
            assert np.array_equal(_host(env, f), w), f
        assert np.array_equal(d_acts.cpu().numpy(), acts) and np.array_equal(d_rng.cpu().numpy().view(np.uint64), rng)
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)], ids=pc.case_id)
def test_playout_agrees_with_real_steps(shape):
    """Case 2: the state tiled Q times and stepped D times for real (autoreset
    off, the sequences' own words): the final state and the summed rewards are
    playout's.  The envs are 7 moves into episodes of 30, so no row ends, and
    the sequences are the ones without padding: q0, q1 and q4."""
    o, _, acts, rng, _, _ = pc.vs_oracle_case(shape, 7)
    sel = [0, 1, 4]
    acts, rng = np.ascontiguousarray(acts[sel]), np.ascontiguousarray(rng[sel])
    n, nq = o.n, len(sel)
    assert (o.timer + pc.D < MOVES).all() and (acts >= 0).all()
    env = _env(shape, n)
    _load(env, o)
    got, _ = _playout(env, acts, rng)
    assert env.status() == 0
    env.close()
    big = _env(shape, nq * n, autoreset=False)
    big.load_state_dict({"board": np.tile(o.board, (nq, 1, 1, 1)), "rng": rng.reshape(nq * n, 5),
                         "timer": np.tile(o.timer, nq), "eff": np.tile(o.eff, (nq, 1)), "eff_valid": True,
                         "config": big.config()})
    total = np.zeros(nq * n, np.int64)
    for d in range(pc.D):
        big.step_raw(_dev(acts[:, :, d].reshape(-1)))
        big.join()
        total += big.reward.cpu().numpy()
    assert big.status() == 0
    assert np.array_equal(total, got["ret"].reshape(-1))
    for f, g in zip(STATE, ("out_board", "out_rng", "out_timer", "out_eff")):
        assert np.array_equal(_host(big, f).reshape(got[g].shape), got[g]), f
    big.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14)], ids=pc.case_id)
def test_playout_final_rows_are_an_env(shape):
    """Case 4: playout(final=True)["env"].peek() is the oracle's peek of the
    oracle's final boards and words (a done row has a zero mask: zeros)."""
    o, timer, acts, rng, want, _ = pc.vs_oracle_case(shape, 7)
    env = _env(shape, o.n)
    _load(env, o, timer)
    got, child = _playout(env, acts, rng)
    peeked = child.peek(outputs=("reward", "n_new", "n_act", "flags"), best=True)
    torch.cuda.synchronize()
    ref = oracle_peek(want["out_board"], want["out_rng"], o.k, o.smask)
    done = (want["flags"].reshape(-1) & pc.FLAG_DONE) != 0
    assert done.any() and not done.all()
    for f in peek_cases.FIELDS:
        w = ref[f].copy()
        w[done] = 0                                              # an all-zero mask: nothing is simulated
        assert np.array_equal(peeked[f].cpu().numpy(), w), f
    assert child.autoreset_mode == "none" and child.num_envs == pc.Q * o.n
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)], ids=pc.case_id)
def test_playout_bad_action_gpu(shape):
    """Case 5: an action >= A at ply 2 of sequence 0 of env 1."""
    from tile_match_gym_amd import _native
    o, timer, acts, rng, clean, _ = pc.vs_oracle_case(shape, 7)
    bad = acts.copy()
    bad[0, 1, 2] = o.A
    want = oracle_playout(o.board, rng, timer, MOVES, o.k, o.smask, bad)
    assert want["flags"][0, 1] & pc.FLAG_ERROR and want["plies"][0, 1] == 2
    env = _env(shape, o.n)
    _load(env, o, timer)
    got, _ = _playout(env, bad, rng)
    assert_playout_equal(got, want, str(shape))
    assert env.status(clear=True) == _native.STATUS_CALLER
    others = np.ones((pc.Q, o.n), bool)
    others[0, 1] = False
    for f in ("ret", "plies", "flags"):
        assert np.array_equal(got[f][others], clean[f][others]), f
    assert np.array_equal(got["out_board"][others.reshape(-1)], clean["out_board"][others.reshape(-1)])
    env.close()


@pytest.mark.parametrize("shape,seed0,n", pc.SHUFFLE_CASES, ids=[pc.case_id(c[0]) for c in pc.SHUFFLE_CASES])
def test_playout_shuffle_at_later_ply_gpu(shape, seed0, n):
    """Case 6: boards that go dead inside a sequence (asserted on the oracle first)."""
    o, acts, want, at = pc.shuffle_case(shape, seed0, n)
    assert any(d >= 1 for d in at), f"{shape}: no move at a ply >= 1 shuffles on the oracle"
    env = _env(shape, o.n)
    _load(env, o)
    got, _ = _playout(env, acts)
    assert_playout_equal(got, want, str(shape))
    assert env.status() == 0
    env.close()


def _ctx_playout(ctx, n, W, shape, board, rng, per_seq, timer, eff, trust, acts, fields=pc.FIELDS):
    """Context.playout on fresh device tensors of a sentinel fill; the dict of `fields`."""
    R, C, k, sm = shape
    nq, _, depth = acts.shape
    m = nq * n
    shapes = {"ply_reward": (nq, n, depth), "flags": (nq, n), "out_board": (m, 2, R, C), "out_rng": (m, 5),
              "out_eff": (m, W), "out_timer": (m,), "best_seq": (n,), "best_ret": (n,)}
    dt = {"flags": torch.uint8, "out_board": torch.int8, "out_rng": torch.int64, "out_eff": torch.int64}
    out = {f: torch.full(shapes.get(f, (nq, n)), 85, dtype=dt.get(f, torch.int32), device=DEV) for f in fields}
    p = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    ctx.playout(n, p(board), p(rng), per_seq, p(timer), p(eff), trust, nq, depth, p(acts),
                *(p(out.get(f)) for f in pc.FIELDS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items()}


@pytest.mark.parametrize("shape,mode,many", peek_cases.spill_params(device=True))
def test_playout_untrusted_and_spill_gpu(shape, mode, many):
    """Case 7: hand-written boards, trust_eff = 0 and no mask given, through
    Context.playout: the general kernels, and the spill pass for the virtual
    envs one of whose plies outgrows the LDS lists.  many: more spilling
    virtual envs than the spill pass has waves."""
    R, C, k, sm = shape
    n = peek_cases.MANY_SPILLS[shape][1] if many else peek_cases.envs_of(shape)
    b, words, acts = pc.adversarial_case(shape, mode, n)
    env = _env(shape, n)
    board, rng, d_acts = _dev(b), _dev(words), _dev(acts)
    fields = tuple(f for f in pc.FIELDS if f != "out_timer")
    s0 = env.ctx.spills()
    got = _ctx_playout(env.ctx, n, env.mask_words, shape, board, rng, 1, None, None, 0, d_acts, fields)
    want = oracle_playout(b, words, None, MOVES, k, sm, acts)
    assert_playout_equal(got, want, f"{shape} {mode}", fields)
    assert env.status() == 0
    if (R, C) in ((20, 20), (10, 10)) and mode != "stripes":
        assert env.ctx.spills() > s0, "the adversarial boards were meant to outgrow the LDS lists"
    if many:
        assert env.ctx.spills() - s0 > peek_cases.SPILL_WAVES
    assert np.array_equal(board.cpu().numpy(), b) and np.array_equal(rng.cpu().numpy().view(np.uint64), words)
    assert np.array_equal(d_acts.cpu().numpy(), acts)
    env.close()


@pytest.mark.parametrize("shape", pc.LINE_SHAPES, ids=pc.case_id)
def test_playout_line_after_ineffective_ply_gpu(shape):
    """Case 7, the boards that already hold a line: trust_eff = 0, an
    ineffective first ply, then an effective one, which still starts from the
    caller's board and has to search all of it for lines; through
    Context.playout with no mask, and through TileMatchVecEnv.playout with the
    mask cache invalid."""
    case = pc.line_case(shape)
    pc.check_line_conditions(shape, case)
    b, words, acts, want, _ = case
    n = b.shape[0]
    env = _env(shape, n)
    fields = tuple(f for f in pc.FIELDS if f != "out_timer")
    got = _ctx_playout(env.ctx, n, env.mask_words, shape, _dev(b), _dev(words), 0, None, None, 0, _dev(acts), fields)
    assert_playout_equal(got, want, str(shape), fields)
    env.board.copy_(_dev(b))
    env.rng.copy_(_dev(words))
    env.invalidate_effective_cache()
    got, _ = _playout(env, acts)
    assert_playout_equal(got, want, str(shape), fields)
    assert env.status() == 0
    env.close()


def test_playout_reduce_gpu():
    """Case 8: Q = 130, planted ties, the lowest q wins; an env of all-ineffective sequences."""
    case = pc.reduce_case()
    pc.check_reduce_conditions(case)
    o, acts, want = case
    env = _env(pc.REDUCE_SHAPE, o.n)
    _load(env, o)
    got, _ = _playout(env, acts)
    assert_playout_equal(got, want, "reduce")
    assert env.status() == 0
    env.close()


class AlignedBand(ec.Band):
    """A Band whose payload starts on an 8-byte boundary whatever the row size
    (out_board has to; three guard rows of a 7x9 board are 378 bytes): 4 front
    guard rows instead of extent_cases.FRONT = 3."""

    FRONT4 = 4

    def __init__(self, n, row_shape, dtype, device="cuda:0"):
        self.n, self.row_shape, self.dtype = int(n), tuple(row_shape), dtype
        rows = self.FRONT4 + self.n + ec.BACK
        self.row_bytes = torch.empty((), dtype=dtype).element_size() * int(np.prod(self.row_shape, dtype=np.int64))
        self.raw = torch.full((rows * self.row_bytes,), ec.FILL, dtype=torch.uint8, device=device)
        self.view = self.raw.view(dtype).view(rows, *self.row_shape)[self.FRONT4:self.FRONT4 + self.n]
        assert self.view.is_contiguous() and self.view.data_ptr() % 8 == 0

    def guards_intact(self):
        lo, hi = self.FRONT4 * self.row_bytes, (self.FRONT4 + self.n) * self.row_bytes
        return bool((self.raw[:lo] == ec.FILL).all().item()) and bool((self.raw[hi:] == ec.FILL).all().item())

    def payload_bytes(self):
        lo, hi = self.FRONT4 * self.row_bytes, (self.FRONT4 + self.n) * self.row_bytes
        return self.raw[lo:hi].cpu().numpy()


EXTENT_SHAPES = [(7, 9, 5, 15), (10, 10, 4, 0), (20, 20, 6, 15)]      # 2N = 126: byte stores; <= 128 cells; 512 cells
EXTENT = [pytest.param(s, n, q, id=f"{pc.case_id(s)}-n{n}-q{q}") for s in EXTENT_SHAPES for n in (1, 3, 9, 65)
          for q in (1, 3)]


@pytest.mark.parametrize("shape,n,nq", EXTENT)
def test_playout_extent(shape, n, nq):
    """Case 9: every array of the call, inputs included, between guard rows
    (tests/extent_cases.py Band); num_moves = 2 and timers 0, 1, 2 in turn, so
    the rows have horizons 2, 1 and 0; D = 3.  Rows 0 .. Q n - 1 equal the
    oracle, every guard byte is intact, every input holds its bytes."""
    R, C, k, sm = shape
    ctx = ec.context(shape)
    A, W = ctx.num_actions, ctx.mask_words
    st = ec.rolled_state(shape, n)
    timers = (np.arange(n) % 3).astype(np.int32)
    rs = np.random.default_rng([*shape, n, nq])
    acts = rs.integers(0, A, (nq, n, 3)).astype(np.int32)
    for i in range(n):                                           # sequence 0 starts with an effective move
        acts[0, i, 0] = np.nonzero(orc.effective_mask(st["board"][i])[0])[0][0]
    rng = np.stack([ec.seed_words(n, 7000 + 100 * q) for q in range(nq)])
    m = nq * n
    b = ec.Bands()
    b.add("board", n, (2, R, C), torch.int8, st["board"])
    b.add("rng", m, (5,), torch.int64, rng.reshape(m, 5))
    b.add("eff", n, (W,), torch.int64, st["eff"])
    b.add("timer", n, (), torch.int32, timers)
    b.add("actions", m, (3,), torch.int32, acts.reshape(m, 3))
    for f in ("ret", "n_new", "n_act", "plies", "out_timer"):
        b.add(f, m, (), torch.int32)
    b.add("flags", m, (), torch.uint8)
    b.add("ply_reward", m, (3,), torch.int32)
    b["out_board"] = AlignedBand(m, (2, R, C), torch.int8)
    b.add("out_rng", m, (5,), torch.int64)
    b.add("out_eff", m, (W,), torch.int64)
    b.add("best_seq", n, (), torch.int32)
    b.add("best_ret", n, (), torch.int32)
    before = b.snapshot("board", "rng", "eff", "timer", "actions")
    what = (shape, n, nq, "playout")
    ctx.playout(n, b.ptr("board"), b.ptr("rng"), 1, b.ptr("timer"), b.ptr("eff"), 1, nq, 3, b.ptr("actions"),
                *b.ptrs(*pc.FIELDS), ec.stream())
    want = oracle_playout(st["board"], rng, timers, ec.MOVES, k, sm, acts)
    torch.cuda.synchronize()
    assert_playout_equal({f: b[f].host() for f in pc.FIELDS}, want, str(what))
    b.check(what, before)
    assert (want["plies"].reshape(-1)[np.tile(timers, nq) == 2] == 0).all()
    assert ctx.status(clear=True) == 0


def test_playout_refusals_and_noops_gpu():
    """Case 10: each refusal of the list, n == 0, and a tmg_create_scan context."""
    from tile_match_gym_amd import _native
    shape = (10, 10, 4, 0)
    o, timer, acts, rng, want, _ = pc.vs_oracle_case(shape, 7)
    env = _env(shape, o.n)
    _load(env, o, timer)
    n, A = o.n, env.num_actions
    d_acts = _dev(acts)
    ret = torch.zeros((pc.Q, n), dtype=torch.int32, device=DEV)
    best = torch.zeros(n, dtype=torch.int32, device=DEV)
    ot = torch.zeros(pc.Q * n, dtype=torch.int32, device=DEV)
    ob = torch.zeros(pc.Q * n * 200 + 8, dtype=torch.int8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ctx=env.ctx, n=n, board=env.board.data_ptr(), rng=env.rng.data_ptr(), timer=env.timer.data_ptr(),
             eff=env.eff.data_ptr(), trust=1, q=pc.Q, d=pc.D, acts=d_acts.data_ptr(), ret=ret.data_ptr(),
             out_board=None, out_timer=None, best_seq=None):
        ctx.playout(n, board, rng, 0, timer, eff, trust, q, d, acts, ret, None, None, None, None, None, out_board,
                    None, out_timer, None, best_seq, None, stream)

    call()
    torch.cuda.synchronize()
    assert np.array_equal(ret.cpu().numpy(), oracle_playout(o.board, o.rng, timer, MOVES, o.k, o.smask, acts)["ret"])
    for kw, msg in ((dict(n=-1), "negative"), (dict(q=0), "sequence"), (dict(d=0), "depth"),
                    (dict(n=2 ** 26 - 8, q=2), "n \\* seqs"), (dict(board=None), "null"), (dict(rng=None), "null"),
                    (dict(acts=None), "null"), (dict(eff=None), "trust_eff"),
                    (dict(timer=None, out_timer=ot.data_ptr()), "out_timer needs timer"),
                    (dict(ret=None, best_seq=best.data_ptr()), "need ret"),
                    (dict(out_board=ob.data_ptr() + 1), "8-byte aligned")):
        with pytest.raises(_native.TmgError, match=msg):
            call(**kw)
    call(eff=None, trust=0)
    call(out_board=ob.data_ptr())
    ret.fill_(-7)
    call(n=0, board=None, rng=None, acts=None, eff=None)             # n == 0: a no-op
    torch.cuda.synchronize()
    assert bool((ret == -7).all())
    scan = _native.scan_context(0, 10, 10)
    with pytest.raises(_native.TmgError, match="tmg_create_scan"):
        call(ctx=scan)
    # the Python layer's own checks
    with pytest.raises(ValueError, match="actions must be"):
        env.playout(d_acts.to(torch.int64))
    with pytest.raises(ValueError, match="actions must be"):
        env.playout(d_acts[:, :2])
    with pytest.raises(ValueError, match="rng must be"):
        env.playout(d_acts, rng=torch.zeros((n, 4), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="unknown playout output"):
        env.playout(d_acts, outputs=("reward",))
    with pytest.raises(ValueError, match="not both"):
        env.playout(d_acts, rng=env.rng, seed=3)
    with pytest.raises(ValueError, match="final=True needs the horizon"):
        env.playout(d_acts, final=True, horizon=False)
    padded = d_acts.clone()
    padded[2, 1, 0] = -1
    before = _host(env, "timer").copy()
    with pytest.raises(ValueError, match="start with an action"):
        env.step_best_sequence(padded)
    assert np.array_equal(_host(env, "timer"), before)               # nothing was stepped
    assert env.status() == 0
    env.close()


def test_playout_seeded_words_and_2d_actions():
    """seed=E is fresh_rng(Q, E, first_env); an (N, D) tensor is Q = 1 with the envs' own words."""
    shape = (10, 10, 4, 14)
    o, timer, acts, rng, _, _ = pc.vs_oracle_case(shape, 7)
    env = _env(shape, o.n)
    _load(env, o, timer)
    words = env.fresh_rng(pc.Q, 77, 5).cpu().numpy().view(np.uint64)
    out = env.playout(_dev(acts), seed=77, first_env=5, outputs=("ret", "plies"))
    want = oracle_playout(o.board, words, timer, MOVES, o.k, o.smask, acts)
    assert np.array_equal(out["ret"].cpu().numpy(), want["ret"]) and np.array_equal(out["plies"].cpu().numpy(), want["plies"])
    out = env.playout(_dev(acts[0]), outputs=("ret",))
    want = oracle_playout(o.board, o.rng, timer, MOVES, o.k, o.smask, acts[:1])
    assert out["ret"].shape == (1, o.n) and np.array_equal(out["ret"].cpu().numpy(), want["ret"])
    # horizon=False: the timers are not passed on, env 0 (two moves left) plays all D plies and nothing is DONE
    out = env.playout(_dev(acts), rng=_dev(rng), outputs=("ret", "plies", "flags"), horizon=False)
    want = oracle_playout(o.board, rng, None, MOVES, o.k, o.smask, acts)
    for f in ("ret", "plies", "flags"):
        assert np.array_equal(out[f].cpu().numpy(), want[f]), f
    assert (want["plies"][[0, 1, 4], 0] == pc.D).all() and not (want["flags"] & pc.FLAG_DONE).any()
    assert env.status() == 0
    env.close()


def test_playout_facade():
    """Case 11: TileMatchEnv.playout on one env is row 0 of the batch form, the
    env left as it was; step_best_sequence plays the oracle's best first action."""
    from tile_match_gym_amd.tile_match_env import TileMatchEnv
    moves = 10
    env = TileMatchEnv(8, 8, 4, moves, [], ["vertical_laser", "horizontal_laser", "bomb"], seed=5, device=DEV)
    env.reset()
    board, words = env.board.board.copy(), env.board.rng_words.copy()
    b8, timer = board.astype(np.int8)[None], np.array([env.timer], np.int32)
    rs = np.random.default_rng(2)
    seqs = np.stack([pc.greedy_walk(b8[0], words, 4, 14, 4, rs), rs.integers(0, env.num_actions, 4), [3, -1, -1, -1]])
    got = env.playout(seqs)
    want = oracle_playout(b8, words[None], timer, moves, 4, 14, seqs[:, None, :].astype(np.int32))
    assert np.array_equal(got["ret"], want["ret"][:, 0]) and np.array_equal(got["plies"], want["plies"][:, 0])
    assert np.array_equal(got["ply_reward"], want["ply_reward"][:, 0])
    assert np.array_equal(got["board"], want["out_board"].astype(np.int32))
    assert np.array_equal(got["rng_words"], want["out_rng"])
    assert np.array_equal(got["shuffled"], (want["flags"][:, 0] & pc.FLAG_SHUFFLED) != 0)
    assert not got["done"].any()
    assert np.array_equal(env.board.board, board) and np.array_equal(env.board.rng_words, words)
    env.close()
    # the batch form: 6 steps of the shooting planner against OracleBatch driven by the oracle's best sequence
    shape = (10, 10, 4, 14)
    R, C, k, sm = shape
    n, nq, depth = 8, 6, 3
    venv = _env(shape, n, num_moves=4)
    o = orc.OracleBatch(R, C, k, sm, 4, venv.rng_words().copy())
    venv.reset()
    o.reset()
    for t in range(6):
        acts = rs.integers(0, o.A, (nq, n, depth)).astype(np.int32)
        for i in range(n):
            acts[t % nq, i] = pc.greedy_walk(o.board[i], o.rng[i], k, sm, depth, rs)
        want = oracle_playout(o.board, o.rng, o.timer, 4, k, sm, acts)
        best = venv.step_best_sequence(_dev(acts))
        venv.join()
        first = acts[want["best_seq"], np.arange(n), 0]
        o.step(first, autoreset=True)
        assert np.array_equal(venv.actions.cpu().numpy(), first), t
        assert np.array_equal(best.cpu().numpy(), want["best_ret"]), t
        for f in STATE + ("reward", "flags"):
            assert np.array_equal(_host(venv, f), getattr(o, f)), (t, f)
    assert venv.status() == 0
    venv.close()
