"""tmg_seed on the MI355X: the PCG64 words of every stream seeded on the device
against numpy's own np.random.PCG64(...) state (tests/seed_cases.py), exactly;
then the Python surface that seeds through it (TileMatchVecEnv's seed / seeds,
set_seed, reset(seed=), TileMatchVectorEnv.reset(seed=), fresh_rng, and the
seed= of rollout / step_rollout_greedy / peek)."""
import numpy as np
import pytest
import torch

import seed_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
PAD = 70                                   # rows behind the m seeded ones: more than a wave of them
SIZES = (1, 63, 64, 65, 257)               # one lane; the wave tail; a full wave; the block tail; a second block's tail
ALL = ("ret", "plies", "flags", "total")


@pytest.fixture(scope="module")
def ctx():
    from tile_match_gym_amd import _native
    c = _native.Context(0, 10, 10, 4, 0, 30)
    yield c
    c.close()


def _stores():
    from tile_match_gym_amd import _native
    return (("default", 0), ("direct", _native.SEED_STORE_DIRECT), ("staged", _native.SEED_STORE_STAGED))


def _seed(c, m, mode=0, seeds=None, rows=None, **kw):
    """Context.seed into a sentinel-filled buffer of m + PAD rows; the whole buffer as uint64."""
    buf = torch.full((max(m, 0) + PAD if rows is None else rows, 5), SENTINEL, dtype=torch.int64, device=DEV)
    d = None if seeds is None else torch.from_numpy(np.ascontiguousarray(seeds).view(np.int64)).to(DEV)
    c.seed(m, buf.data_ptr(), 0, mode=mode, seeds=None if d is None else d.data_ptr(), **kw)
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("m", SIZES)
def test_seed_cases_gpu(ctx, m):
    """Every case of the table with every store variant; the rows behind m keep the sentinel."""
    table = sc.cases(m)
    for store, bits in _stores():
        for name, call, want in table:
            call = dict(call)
            got = _seed(ctx, m, call.pop("mode") | bits, **call)
            assert np.array_equal(got[:m], want), (name, store)
            assert (got[m:] == SENTINEL).all(), (name, store)


def test_known_answers_gpu(ctx):
    for call, want in sc.KNOWN:
        call = dict(call)
        got = _seed(ctx, 1, call.pop("mode"), **call)
        assert [int(x) for x in got[0]] == list(want)


def test_edges_empty_and_scan_context_gpu(ctx):
    from tile_match_gym_amd import _native
    for name, m, call, want in sc.EDGES:
        call = dict(call)
        got = _seed(ctx, m, call.pop("mode"), **call)
        assert np.array_equal(got[:m], want()) and (got[m:] == SENTINEL).all(), name
    assert (_seed(ctx, 0, base=3) == SENTINEL).all()                    # m == 0 writes nothing
    scan = _native.scan_context(0, 3, 5)                                 # any context serves
    got = _seed(scan, 65, base=2 ** 64 - 3)
    assert np.array_equal(got[:65], sc.numpy_rows(range(2 ** 64 - 3, 2 ** 64 + 62))) and (got[65:] == SENTINEL).all()


def test_refusals_gpu(ctx):
    from tile_match_gym_amd import _native
    L = ctx._L
    buf = torch.full((8, 5), SENTINEL, dtype=torch.int64, device=DEV)
    for name, m, call in sc.REFUSED:
        call = dict(dict(mode=0, seed_words=1, base=0, key0=0, key1=0, period=0, rng=buf.data_ptr()), **call)
        base = call["base"]
        rc = L.tmg_seed(ctx.handle, m, call["mode"], None, call["seed_words"], base & sc.M64, base >> 64, call["key0"],
                        call["key1"], call["period"], call["rng"], None)
        assert rc < 0 and L.tmg_last_error(), name
        with pytest.raises(_native.TmgError):
            _native.check(rc, L)
    seeds = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(_native.TmgError, match="seeds must be NULL"):
        ctx.seed(4, buf.data_ptr(), 0, mode=_native.SEED_SPAWN, seeds=seeds.data_ptr())
    assert L.tmg_seed(None, 4, 0, None, 1, 0, 0, 0, 0, 0, buf.data_ptr(), None) < 0       # null context
    with pytest.raises(ValueError):
        ctx.seed(4, buf.data_ptr(), 0, base=2 ** 128)
    with pytest.raises(ValueError):
        ctx.seed(4, buf.data_ptr(), 0, base=-1)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint64) == SENTINEL).all()         # no refused call wrote


def _vec(n, **kw):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    return TileMatchVecEnv(n, 10, 10, 4, 30, device=DEV, **kw)


def test_vec_env_seeds_on_device_gpu():
    from tile_match_gym_amd.seeding import batch_rng_words
    n, base = 64, 2 ** 32 - 10
    want = batch_rng_words(range(base, base + n))
    env = _vec(n, seed=base)
    assert np.array_equal(env.rng_words(), want)
    # a list, an ndarray and a tensor of seeds, one of them >= 2^64; then one >= 2^128 (numpy's to seed)
    small = [int(s) for s in np.random.default_rng(1).integers(0, 2 ** 63, n)]
    wide = list(small)
    wide[5] = 2 ** 64 + 17
    huge = list(wide)
    huge[9] = 2 ** 128 + 3
    for seeds, ref in ((small, small), (np.array(small, np.int64), small), (np.array(small, np.uint64), small),
                       (torch.tensor(small), small), (torch.tensor(small, device=DEV), small), (wide, wide),
                       (tuple(wide), wide), (np.array(wide, dtype=object), wide), (huge, huge),
                       ((s for s in small), small)):
        e = _vec(n, seeds=seeds)
        assert np.array_equal(e.rng_words(), batch_rng_words(ref)), type(seeds)
        e.close()
    # set_seed and reset(seed=) re-seed the same way
    env.set_seed(wide)
    assert np.array_equal(env.rng_words(), batch_rng_words(wide))
    env.set_seed(huge)
    assert np.array_equal(env.rng_words(), batch_rng_words(huge))
    env.set_seed(range(7, 7 + n))
    assert np.array_equal(env.rng_words(), batch_rng_words(range(7, 7 + n)))
    twin = _vec(n, seed=2 ** 64 - 5)
    assert np.array_equal(twin.rng_words(), batch_rng_words(range(2 ** 64 - 5, 2 ** 64 - 5 + n)))
    env.reset(seed=2 ** 64 - 5)
    twin.reset()
    assert np.array_equal(env.rng_words(), twin.rng_words())
    assert torch.equal(env.board, twin.board)
    for bad in ([1] * (n - 1) + [-1], np.full(n, -2), range(-1, n - 1)):
        with pytest.raises(ValueError):
            env.set_seed(bad)
    with pytest.raises(ValueError):
        env.set_seed(range(n + 1))
    with pytest.raises(ValueError):
        _vec(n, seeds=[-1] * n)
    env.close()
    twin.close()


def test_vector_env_reset_seeds_gpu():
    from tile_match_gym_amd.seeding import batch_rng_words
    from tile_match_gym_amd.vector import TileMatchVectorEnv
    n = 16
    venv = TileMatchVectorEnv(n, 10, 10, 4, 30, seed=3, device=DEV)
    ref = _vec(n, seed=0)
    seeds = [2 ** 40 + 3 * i for i in range(n)]
    seeds[2] = 2 ** 100 + 1
    for seed, want in ((seeds, seeds), (np.arange(50, 50 + n), range(50, 50 + n)), (2 ** 32 - 4, range(2 ** 32 - 4, 2 ** 32 - 4 + n))):
        obs, _ = venv.reset(seed=seed)
        ref.set_seed(want)
        assert np.array_equal(ref.rng_words(), batch_rng_words(want))
        ref.reset()
        assert np.array_equal(venv.vec.rng_words(), ref.rng_words())
        assert torch.equal(obs["board"].to(torch.int8), ref.board)
    venv.close()
    ref.close()


def _spawn_words(entropy, samples, n, first_env):
    return np.stack([sc.spawn_rows(entropy, [(s, first_env + i) for i in range(n)]) for s in range(samples)])


@pytest.mark.parametrize("shape", [(8, 8, 3), (10, 10, 4)], ids=["8x8k3", "10x10k4"])
def test_rollout_and_peek_seed_gpu(shape):
    """seed=E draws the words of SeedSequence(E, spawn_key=(s, first_env + i)) on the device."""
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k = shape
    n = 8
    env = TileMatchVecEnv(n, R, C, k, 30, seeds=range(500, 500 + n), device=DEV)
    env.reset()
    W = _spawn_words(9, 2, n, 100)
    fresh = env.fresh_rng(2, 9, first_env=100)
    torch.cuda.synchronize()
    assert fresh.shape == (2, n, 5) and fresh.dtype == torch.int64
    assert np.array_equal(fresh.cpu().numpy().view(np.uint64), W)
    Wd = torch.from_numpy(W.view(np.int64)).to(DEV)
    got = {f: v.clone() for f, v in env.rollout(2, samples=2, seed=9, first_env=100, outputs=ALL, best=True).items()}
    want = env.rollout(2, 2, rng=Wd, first_env=100, outputs=ALL, best=True)
    for f in want:
        assert torch.equal(got[f], want[f]), f
    assert int(want["ret"].sum()) > 0
    # peek: one sample, key (0, i)
    P0 = torch.from_numpy(_spawn_words(9, 1, n, 0)[0].view(np.int64)).to(DEV)
    names = ("reward", "n_new", "n_act", "flags")
    got = {f: v.clone() for f, v in env.peek(seed=9, outputs=names, best=True).items()}
    want = env.peek(rng=P0, outputs=names, best=True)
    for f in want:
        assert torch.equal(got[f], want[f]), f
    # the rollout-greedy step with a seed plays the action its rollout picks
    twin = TileMatchVecEnv(n, R, C, k, 30, seeds=range(500, 500 + n), device=DEV)
    twin.reset()
    best = env.rollout(2, 2, rng=Wd, first_env=100, outputs=(), best=True)["best_action"].clone()
    total = twin.step_rollout_greedy(2, 2, first_env=100, seed=9)
    twin.join()
    assert torch.equal(twin.actions, best) and total.shape == (n,)
    # rng and seed together, and more samples than one without either
    with pytest.raises(ValueError):
        env.rollout(2, 2, rng=Wd, seed=9)
    with pytest.raises(ValueError):
        env.step_rollout_greedy(2, 2, rng=Wd, seed=9)
    with pytest.raises(ValueError):
        env.peek(rng=P0, seed=9)
    with pytest.raises(ValueError):
        env.rollout(2, 2)
    assert env.status() == 0 and twin.status() == 0
    env.close()
    twin.close()
