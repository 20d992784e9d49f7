"""tmg_seed's arithmetic on the host (CPU): emu_seed of tools/wave_emu runs
csrc/tmg_seed.h's per-stream function, the one the device kernel runs, over
every row, and refuses what tmg_seed refuses (the same seed_refusal).  Every
expected row is numpy's own PCG64 state; equality is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seed_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    return emu, emu.load()


def test_known_answers(emu_lib):
    emu, L = emu_lib
    for call, want in sc.KNOWN:
        got = emu.seed(L, 1, **call)
        assert [int(x) for x in got[0]] == list(want), call
        # and numpy agrees with the stated words
    assert np.array_equal(sc.words(12345), np.array(sc.KNOWN[0][1], np.uint64))
    assert np.array_equal(sc.words(np.random.SeedSequence(7, spawn_key=(3, 2 ** 32 + 1))),
                          np.array(sc.KNOWN[1][1], np.uint64))


def test_int_array_forms(emu_lib):
    """64-bit seeds around the one / two word boundary, 128-bit seeds as lo / hi pairs."""
    emu, L = emu_lib
    got = emu.seed(L, len(sc.SEEDS64), sc.SEED_INT, seeds=sc.pack(sc.SEEDS64, 1), seed_words=1)
    assert np.array_equal(got, sc.numpy_rows(sc.SEEDS64))
    got = emu.seed(L, len(sc.SEEDS128), sc.SEED_INT, seeds=sc.pack(sc.SEEDS128, 2), seed_words=2)
    assert np.array_equal(got, sc.numpy_rows(sc.SEEDS128))
    # a 64-bit seed passed as a pair is the same seed
    got = emu.seed(L, len(sc.SEEDS64), sc.SEED_INT, seeds=sc.pack(sc.SEEDS64, 2), seed_words=2)
    assert np.array_equal(got, sc.numpy_rows(sc.SEEDS64))


@pytest.mark.parametrize("base", sc.RANGE_BASES)
def test_range_form_carries(emu_lib, base):
    """base + j crosses 2^32 (a second entropy word) and 2^64 (the carry into the high half)."""
    emu, L = emu_lib
    assert np.array_equal(emu.seed(L, 8, sc.SEED_INT, base=base), sc.numpy_rows(range(base, base + 8)))


@pytest.mark.parametrize("key0", sc.SPAWN_KEY0)
@pytest.mark.parametrize("entropy", sc.SPAWN_ENTROPY)
def test_spawn_one_element(emu_lib, entropy, key0):
    """Key (key0 + j,): from 2^32 - 2 the element turns from one word into two inside the batch."""
    emu, L = emu_lib
    got = emu.seed(L, 5, sc.SEED_SPAWN, base=entropy, key0=key0)
    assert np.array_equal(got, sc.spawn_rows(entropy, [(key0 + j,) for j in range(5)]))


def test_spawn_two_elements(emu_lib):
    emu, L = emu_lib
    k0, k1 = 2 ** 33, 2 ** 32 - 2
    for e in sc.SPAWN_ENTROPY:
        got = emu.seed(L, 10, sc.SEED_SPAWN, base=e, key0=k0, key1=k1, period=3)
        assert np.array_equal(got, sc.spawn_rows(e, [(k0 + j // 3, k1 + j % 3) for j in range(10)])), e


def test_spawn_form_is_seedsequence_spawn(emu_lib):
    emu, L = emu_lib
    for e in sc.SPAWN_ENTROPY:
        want = sc.numpy_rows(np.random.SeedSequence(e).spawn(6))
        assert np.array_equal(emu.seed(L, 6, sc.SEED_SPAWN, base=e), want), e


@pytest.mark.parametrize("m", (1, 63, 64, 65, 257))
def test_every_case_at_the_device_sizes(emu_lib, m):
    """The case table the device test runs, on the host."""
    emu, L = emu_lib
    for name, call, want in sc.cases(m):
        assert np.array_equal(emu.seed(L, m, **call), want), name


def test_refusals_and_edges(emu_lib):
    emu, L = emu_lib
    rng = np.zeros((8, 5), np.uint64)
    for name, m, call in sc.REFUSED:
        call = dict(dict(mode=0, seeds=None, seed_words=1, base=0, key0=0, key1=0, period=0, rng=rng), **call)
        base, out = call.pop("base"), call.pop("rng")
        rc = L.emu_seed(m, call["mode"], None, call["seed_words"], base & sc.M64, base >> 64, call["key0"],
                        call["key1"], call["period"], out.ctypes.data if out is not None else None)
        assert rc < 0, name
    assert not rng.any()
    seeds = np.zeros(4, np.uint64)
    assert L.emu_seed(4, sc.SEED_SPAWN, seeds.ctypes.data, 1, 0, 0, 0, 0, 0, rng.ctypes.data) < 0   # spawn form + array
    assert L.emu_seed(0, 0, None, 1, 0, 0, 0, 0, 0, rng.ctypes.data) == 0 and not rng.any()          # m == 0
    for name, m, call, want in sc.EDGES:
        assert np.array_equal(emu.seed(L, m, **call), want()), name
    # the store-variant bits change nothing on the host
    assert np.array_equal(emu.seed(L, 3, sc.SEED_INT | 0x100, base=5), emu.seed(L, 3, sc.SEED_INT | 0x200, base=5))


def test_pack_seeds_classifies():
    """seeding.pack_seeds: what goes to the device and how, what stays with numpy."""
    from tile_match_gym_amd.seeding import pack_seeds
    assert pack_seeds(range(5, 9)) == ("range", 5, 4)
    assert pack_seeds(range(0)) == ("range", 0, 0)
    kind, a = pack_seeds([3, 2 ** 64 - 1])
    assert kind == "array" and a.dtype == np.uint64 and a.tolist() == [3, 2 ** 64 - 1]
    kind, a = pack_seeds((3, 2 ** 64 + 2, np.int64(7)))
    assert kind == "array" and a.tolist() == [[3, 0], [2, 1], [7, 0]]
    kind, a = pack_seeds(np.array([1, 2, 3], np.int32))
    assert kind == "array" and a.dtype == np.uint64 and a.tolist() == [1, 2, 3]
    kind, a = pack_seeds(range(0, 6, 2))
    assert kind == "array" and a.tolist() == [0, 2, 4]
    assert pack_seeds([1, 2 ** 128]) is None                    # numpy's to seed
    assert pack_seeds(range(2 ** 128 - 1, 2 ** 128 + 1)) is None
    assert pack_seeds(s for s in (1, 2)) is None                # any other iterable: untouched
    assert pack_seeds([1, 2.0]) is None
    for bad in ([1, -1], np.array([-3]), range(-2, 2)):
        with pytest.raises(ValueError):
            pack_seeds(bad)
