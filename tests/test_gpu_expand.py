"""tmg_expand_count / tmg_expand on the MI355X: the successor states of every
effective action against the oracle's children (tests/expand_cases.py
oracle_expand: numpy placement, OracleBatch.step on the copies).  Boards are
compared as bytes and counts as integers; nothing here has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import expand_cases
import peek_cases
from adversarial import adversarial_boards
from deep_rollouts import specials
from expand_cases import assert_expand_equal, oracle_expand, pack_mask, unpack_mask
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE = expand_cases.STATE
ROW_FIELDS = [f for f in expand_cases.FIELDS if f != "first_child"]
FILL64 = 0x5A5A5A5A5A5A5A5A


@functools.lru_cache(maxsize=None)
def _rolled(shape, steps, n=None, num_moves=30):
    """The oracle state the tests expand (shared, never changed: users copy)."""
    n = n or expand_cases.envs_of(shape)
    return peek_cases.rolled_batch(shape, range(500, 500 + n), steps=steps, num_moves=num_moves)


def _env(shape, n, num_moves=30, **kw):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, sm = shape
    cl, co = specials(sm)
    return TileMatchVecEnv(n, R, C, k, num_moves, cl, co, seeds=range(500, 500 + n), device=DEV, **kw)


def _load(env, o, timer=None):
    env.load_state_dict({"board": o.board, "rng": o.rng, "timer": o.timer if timer is None else timer, "eff": o.eff,
                         "eff_valid": True, "config": env.config()})


def _words(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(DEV)


def _host(env, f):
    if f == "rng":
        return env.rng_words()
    v = getattr(env, f).cpu().numpy()
    return v.view(np.uint64) if f == "eff" else v


def _arrays(env, exp):
    """An Expansion as the dict oracle_expand returns."""
    torch.cuda.synchronize()
    out = {f: getattr(exp, f).cpu().numpy() for f in ("first_child", "parent", "action") + expand_cases.OUTPUTS}
    if exp.env is None:
        assert exp.count == 0
        out.update(board=np.zeros((0, 2, env.num_rows, env.num_cols), np.int8), rng=np.zeros((0, 5), np.uint64),
                   timer=np.zeros(0, np.int32), eff=np.zeros((0, env.mask_words), np.uint64))
    else:
        assert exp.env.num_envs == exp.count and exp.env.autoreset_mode == "none"
        out.update({f: _host(exp.env, f) for f in STATE})
    return out


class Raw:
    """Child buffers with a sentinel fill for the C call itself (Context.expand)."""

    def __init__(self, env, m):
        kw = dict(device=DEV)
        self.board = torch.full((m, 2, env.num_rows, env.num_cols), -7, dtype=torch.int8, **kw)
        self.rng = torch.full((m, 5), FILL64, dtype=torch.int64, **kw)
        self.timer, self.action, self.reward, self.n_new, self.n_act = (
            torch.full((m,), -7, dtype=torch.int32, **kw) for _ in range(5))
        self.eff = torch.full((m, env.mask_words), FILL64, dtype=torch.int64, **kw)
        self.parent = torch.full((m,), -7, dtype=torch.int64, **kw)
        self.flags = torch.full((m,), 0x55, dtype=torch.uint8, **kw)

    def ptrs(self):
        return [t.data_ptr() for t in (self.board, self.rng, self.timer, self.eff, self.parent, self.action,
                                       self.reward, self.n_new, self.n_act, self.flags)]

    def host(self):
        torch.cuda.synchronize()
        out = {f: getattr(self, f).cpu().numpy() for f in ROW_FIELDS}
        out["rng"], out["eff"] = out["rng"].view(np.uint64), out["eff"].view(np.uint64)
        return out

    def untouched(self):
        h = self.host()
        return all((h[f] == -7).all() for f in ("board", "timer", "action", "reward", "n_new", "n_act", "parent")) \
            and (h["rng"] == FILL64).all() and (h["eff"] == FILL64).all() and (h["flags"] == 0x55).all()


def _count(env, sel_words=None):
    first = torch.full((env.num_envs + 1,), -7, dtype=torch.int64, device=DEV)
    env.ctx.expand_count(env.num_envs, env.timer.data_ptr(), env.eff.data_ptr(),
                         sel_words.data_ptr() if sel_words is not None else None, first.data_ptr(), env._stream())
    return first


def _raw_expand(env, first, raw, m, sel_words=None, trust=1, ptrs=None):
    env.ctx.expand(env.num_envs, env.board.data_ptr(), env.rng.data_ptr(), env.timer.data_ptr(), env.eff.data_ptr(),
                   sel_words.data_ptr() if sel_words is not None else None, trust, first.data_ptr(), m,
                   *(ptrs or raw.ptrs()), env._stream())


@pytest.mark.parametrize("shape", expand_cases.DEVICE_SHAPES, ids=expand_cases.case_id)
def test_expand_vs_oracle_gpu(shape):
    """After a reset and after 7 uniform-random steps, with the envs' own RNG
    words and with words of other seeds; the parents stay as they were."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k, sm = shape
    n = expand_cases.envs_of(shape)
    env = _env(shape, n)
    other = batch_rng_words(range(7000, 7000 + n))
    for steps in (0, 7):
        o = _rolled(shape, steps)
        _load(env, o)
        for rng in (None, other):
            want = oracle_expand(o.board, o.rng if rng is None else rng, o.timer, o.eff, None, k, sm, 30)
            exp = env.expand(rng=None if rng is None else _words(rng))
            assert exp.count == want["first_child"][n] and exp.count >= 2 * n
            assert_expand_equal(_arrays(env, exp), want, f"{shape} steps={steps} own={rng is None}")
        for f in STATE:
            assert np.array_equal(_host(env, f), getattr(o, f)), f
    assert env.status() == 0
    env.close()


def test_expand_horizon():
    """3x5, num_moves = 8: the children of timer-7 parents are done and have a
    zero mask; timer-8 parents (finished, autoreset off) have none."""
    shape = (3, 5, 2, 0)
    R, C, k, sm = shape
    n, moves = 5, 8
    o = _rolled(shape, 3, n, moves)
    env = _env(shape, n, moves, autoreset=False)
    for timers in ([7] * n, [8] * n, [3, 7, 8, 8, 3]):
        t = np.array(timers, np.int32)
        _load(env, o, timer=t)
        want = oracle_expand(o.board, o.rng, t, o.eff, None, k, sm, moves)
        exp = env.expand()
        got = _arrays(env, exp)
        assert_expand_equal(got, want, str(timers))
        last = t[got["parent"]] == 7
        assert (got["flags"][last] & expand_cases.FLAG_DONE).all() and not got["eff"][last].any()
        assert not (got["flags"][~last] & expand_cases.FLAG_DONE).any()
        if min(timers) == 8:
            assert exp.count == 0 and exp.env is None and not got["first_child"].any()
            raw = Raw(env, 4)
            _raw_expand(env, exp.first_child, raw, 0)               # m = 0: nothing is written
            assert raw.untouched()
        else:
            assert last.any()
    assert env.status() == 0
    env.close()


def test_expand_select():
    shape = (10, 10, 4, 14)
    R, C, k, sm = shape
    o = _rolled(shape, 7)
    n = o.n
    env = _env(shape, n, autoreset=False)
    _load(env, o)
    effm = unpack_mask(o.eff, o.A)
    # a random selection that also names ineffective actions: those give no child
    sel = np.random.default_rng(9).random((n, o.A)) < 0.5
    assert (sel & ~effm).any() and (sel & effm).any()
    want = oracle_expand(o.board, o.rng, o.timer, o.eff, sel, k, sm, 30)
    assert_expand_equal(_arrays(env, env.expand(select=torch.from_numpy(sel).to(DEV))), want, "random select")
    # the C call: select words with bits at and above A are ignored
    words = pack_mask(sel)
    words[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(o.A % 64)
    d_words = _words(words)
    first = _count(env, d_words)
    torch.cuda.synchronize()
    assert np.array_equal(first.cpu().numpy(), want["first_child"])
    m = int(want["first_child"][n])
    raw = Raw(env, m)
    _raw_expand(env, first, raw, m, d_words)
    assert_expand_equal(raw.host(), want, "select words", ROW_FIELDS)
    # one action per env: the children are a step of a copy of the batch
    rs = np.random.default_rng(3)
    a = np.array([rs.choice(np.nonzero(effm[i])[0]) for i in range(n)], np.int32)
    hot = np.zeros((n, o.A), bool)
    hot[np.arange(n), a] = True
    exp = env.expand(select=torch.from_numpy(hot).to(DEV))
    got = _arrays(env, exp)
    twin = _env(shape, n, autoreset=False)
    _load(twin, o)
    twin.step(torch.from_numpy(a).to(DEV))
    assert exp.count == n and np.array_equal(got["action"], a) and np.array_equal(got["parent"], np.arange(n))
    for f in STATE:
        assert np.array_equal(got[f], _host(twin, f)), f
    for f in expand_cases.OUTPUTS:
        assert np.array_equal(got[f], getattr(twin, f).cpu().numpy()), f
    assert env.status() == 0 and twin.status() == 0
    twin.close()
    env.close()


def test_expand_m_prefix_and_tail():
    """m below the total: a prefix, the rows past it keep their fill.  m above
    it: the tail rows are steps after done, whose boards nobody touches."""
    shape = (7, 9, 10, 15)
    R, C, k, sm = shape
    o = _rolled(shape, 7)
    n = o.n
    env = _env(shape, n, autoreset=False)
    _load(env, o)
    want = oracle_expand(o.board, o.rng, o.timer, o.eff, None, k, sm, 30)
    total = int(want["first_child"][n])
    first = _count(env)
    raw = Raw(env, total)
    _raw_expand(env, first, raw, total - 3)
    got = raw.host()
    assert_expand_equal({f: got[f][:total - 3] for f in ROW_FIELDS}, {f: want[f][:total - 3] for f in ROW_FIELDS},
                        "prefix", ROW_FIELDS)
    assert (got["board"][total - 3:] == -7).all() and (got["timer"][total - 3:] == -7).all()
    assert (got["rng"][total - 3:] == FILL64).all() and (got["flags"][total - 3:] == 0x55).all()
    assert (got["action"][total - 3:] == -7).all() and (got["parent"][total - 3:] == -7).all()
    exp = env.expand(max_children=total - 3)
    assert exp.count == total - 3 and int(exp.first_child[n]) == total
    assert np.array_equal(exp.action.cpu().numpy(), want["action"][:total - 3])
    assert env.status() == 0
    raw = Raw(env, total + 5)
    _raw_expand(env, first, raw, total + 5)
    got = raw.host()
    assert_expand_equal({f: got[f][:total] for f in ROW_FIELDS}, want, "head", ROW_FIELDS)
    assert (got["flags"][total:] == expand_cases.FLAG_ERROR).all() and (got["parent"][total:] == -1).all()
    assert (got["timer"][total:] == 30).all() and (got["action"][total:] == 0).all()
    assert not got["eff"][total:].any() and not got["reward"][total:].any()
    assert (got["board"][total:] == -7).all() and (got["rng"][total:] == FILL64).all()
    from tile_match_gym_amd import _native
    assert env.status(clear=True) == _native.STATUS_CALLER
    env.close()


@pytest.mark.parametrize("shape", [(10, 10, 4, 14), (20, 20, 6, 15)], ids=expand_cases.case_id)
def test_expand_untrusted_and_spill(shape):
    """Hand-written boards, the mask from compute_effective(), trust_eff = 0:
    the general kernels run and the children's steps go through the spill tier."""
    R, C, k, sm = shape
    n = expand_cases.envs_of(shape) - 1
    b = adversarial_boards(n, R, C, k, sm, 11, "laser_sea")
    env = _env(shape, n, autoreset=False)
    env.board.copy_(torch.from_numpy(b).to(DEV))
    env.invalidate_effective_cache()
    eff = pack_mask(np.stack([orc.effective_mask(x)[0] for x in b]))
    words = env.rng_words().copy()
    s0 = env.ctx.spills()
    exp = env.expand()
    got = _arrays(env, exp)
    assert np.array_equal(_host(env, "eff"), eff)
    want = oracle_expand(b, words, np.zeros(n, np.int32), eff, None, k, sm, 30)
    assert exp.count > n
    assert_expand_equal(got, want, f"{shape} laser_sea")
    assert env.ctx.spills() > s0, "the adversarial boards were meant to outgrow the LDS lists"
    assert env.status() == 0
    assert np.array_equal(_host(env, "board"), b) and np.array_equal(env.rng_words(), words)
    env.close()


def test_expand_lane_route():
    """10x10 k4, 3 072 envs straight after reset: more than TMG_LANE_MIN_ENVS
    children, so their step is the lane-per-board kernel's."""
    shape = (10, 10, 4, 0)
    R, C, k, sm = shape
    n = 3072
    o = peek_cases.rolled_batch(shape, range(500, 500 + n), steps=0)
    env = _env(shape, n, autoreset=False)
    _load(env, o)
    exp = env.expand()
    assert exp.count >= 131072
    want = oracle_expand(o.board, o.rng, o.timer, o.eff, None, k, sm, 30, threads=16)
    assert exp.count == 140443 and np.diff(want["first_child"]).min() == 23 and np.diff(want["first_child"]).max() == 70
    assert_expand_equal(_arrays(env, exp), want, "lane route")
    assert env.status() == 0
    env.close()


@pytest.mark.parametrize("select", [False, True], ids=["all", "select"])
def test_expand_count_large(select):
    """The scan alone over 100 003 random mask rows (98 workgroup tiles)."""
    shape = (10, 10, 4, 0)
    env = _env(shape, 1)
    n, A, W = 100003, env.num_actions, env.mask_words
    rs = np.random.default_rng(77)
    eff = rs.integers(0, 2 ** 64, (n, W), dtype=np.uint64)
    sel = rs.integers(0, 2 ** 64, (n, W), dtype=np.uint64) if select else None
    timer = rs.integers(0, 60, n).astype(np.int32)
    first = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    d_eff, d_sel, d_timer = _words(eff), _words(sel) if select else None, torch.from_numpy(timer).to(DEV)
    env.ctx.expand_count(n, d_timer.data_ptr(), d_eff.data_ptr(), d_sel.data_ptr() if select else None,
                         first.data_ptr(), env._stream())
    torch.cuda.synchronize()
    counts = unpack_mask(eff & sel if select else eff, A).sum(axis=1) * (timer < 30)
    assert np.array_equal(first.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    env.close()


def test_expand_two_plies():
    """The children are an env: expanding them gives the oracle expanded twice,
    and peeking at them the grandchildren's rewards."""
    shape = (3, 5, 2, 0)
    R, C, k, sm = shape
    o = _rolled(shape, 7)
    env = _env(shape, o.n, autoreset=False)
    _load(env, o)
    w1 = oracle_expand(o.board, o.rng, o.timer, o.eff, None, k, sm, 30)
    w2 = oracle_expand(w1["board"], w1["rng"], w1["timer"], w1["eff"], None, k, sm, 30)
    exp = env.expand()
    exp2 = exp.env.expand()
    assert exp2.count > exp.count > o.n
    assert_expand_equal(_arrays(exp.env, exp2), w2, "second ply")
    assert_expand_equal(_arrays(env, exp), w1, "first ply")            # the children were only read
    peek = exp.env.peek(outputs=("reward",))["reward"]
    torch.cuda.synchronize()
    assert np.array_equal(peek.cpu().numpy()[w2["parent"], w2["action"]], w2["reward"])
    assert env.status() == 0
    exp2.env.close()
    exp.env.close()
    env.close()


def test_expand_refusals():
    """Each refused call raises TmgError with a message and launches nothing."""
    from tile_match_gym_amd import _native
    shape = (3, 5, 2, 0)
    o = _rolled(shape, 7)
    env = _env(shape, o.n, autoreset=False)
    _load(env, o)
    first = _count(env)
    torch.cuda.synchronize()
    total = int(first[o.n])
    raw = Raw(env, total + 1)
    good = raw.ptrs()
    scan = _native.scan_context(0, 3, 5)
    with pytest.raises(_native.TmgError, match="tmg_create_scan"):
        scan.expand(env.num_envs, env.board.data_ptr(), env.rng.data_ptr(), env.timer.data_ptr(), env.eff.data_ptr(),
                    None, 1, first.data_ptr(), total, *good, env._stream())
    with pytest.raises(_native.TmgError, match="tmg_create_scan"):
        scan.expand_count(env.num_envs, env.timer.data_ptr(), env.eff.data_ptr(), None, first.data_ptr(), env._stream())
    no_action = list(good)
    no_action[5] = None
    with pytest.raises(_native.TmgError, match="null child buffer"):
        _raw_expand(env, first, raw, total, ptrs=no_action)
    odd = list(good)
    odd[0] += 2                                                      # a child_board view offset by 2 bytes
    with pytest.raises(_native.TmgError, match="8-byte aligned"):
        _raw_expand(env, first, raw, total, ptrs=odd)
    with pytest.raises(_native.TmgError, match="negative"):
        _raw_expand(env, first, raw, -1)
    with pytest.raises(_native.TmgError, match="null first_child"):
        env.ctx.expand_count(env.num_envs, env.timer.data_ptr(), env.eff.data_ptr(), None, None, env._stream())
    assert raw.untouched()
    # a mis-sized first_child never reaches the C call (it cannot check it)
    with pytest.raises(ValueError, match="first_child"):
        env.expand_rows(first[:-1].contiguous(), total, env.rng)
    with pytest.raises(ValueError, match="select"):
        env.expand(select=torch.ones((o.n, env.num_actions + 1), dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="rng"):
        env.expand(rng=env.rng[:-1].contiguous())
    assert env.status() == 0
    env.close()


def test_facade_expand():
    """TileMatchEnv.expand() on 6x6 k3 with a bomb against oracle_expand of its mirror state."""
    from tile_match_gym_amd.tile_match_env import TileMatchEnv
    env = TileMatchEnv(6, 6, 3, 9, [], ["bomb"], seed=21)
    env.reset()
    rs = np.random.default_rng(4)
    for _ in range(3):
        env.step(int(rs.integers(0, env.num_actions)))
    b = env.board.board.astype(np.int8)[None]
    words = env.board.rng_words.copy()[None]
    eff = pack_mask(orc.effective_mask(b[0])[0][None])
    want = oracle_expand(b, words, np.array([env.timer], np.int32), eff, None, 3, 8, 9)
    got = env.expand()
    assert len(got["action"]) == want["first_child"][1] > 0
    assert np.array_equal(got["action"], want["action"]) and np.array_equal(got["board"], want["board"])
    assert got["board"].dtype == np.int32
    assert np.array_equal(got["rng_words"], want["rng"]) and np.array_equal(got["reward"], want["reward"])
    assert np.array_equal(got["num_new_specials"], want["n_new"])
    assert np.array_equal(got["num_specials_activated"], want["n_act"])
    assert np.array_equal(got["is_combination_match"], (want["flags"] & 2) != 0)
    assert np.array_equal(got["shuffled"], (want["flags"] & 4) != 0) and not got["done"].any()
    assert np.array_equal(env.board.board.astype(np.int8)[None], b) and np.array_equal(env.board.rng_words[None], words)
    env.close()
