"""Shared cases of the tmg_seed tests (tests/test_seed_emulated.py on the host
emulator, tests/test_gpu_seed.py on the device): every expected row is numpy's
own np.random.PCG64(...) state (seeding.rng_words_from_generator), compared
exactly.  A case is (name, call, want): `call` the keyword arguments of
emu.seed / Context.seed but for m and the buffers (seeds as a host uint64
array), `want(m)` the (m, 5) uint64 rows numpy gives."""
import numpy as np

from tile_match_gym_amd.seeding import rng_words_from_generator

SEED_INT, SEED_SPAWN = 0, 1
M64 = (1 << 64) - 1

# the two answers the issue states (np.random.default_rng(12345) and
# SeedSequence(7, spawn_key=(3, 2**32 + 1))): state lo, hi, inc lo, hi, buffer
KNOWN = (
    (dict(mode=SEED_INT, base=12345),
     (0x9199b0d09775add5, 0x1905e0335aae9634, 0x7d761f2d4027fae7, 0xc9c7353e6e2b1f28, 0)),
    (dict(mode=SEED_SPAWN, base=7, key0=3, key1=2 ** 32 + 1, period=1),
     (0x7a9bf0d38577167d, 0x2a256a3616d58d2e, 0xa47f34bcc81ffeab, 0x8e53078d3a8cd582, 0)),
)

SEEDS64 = (0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63 - 1, 2 ** 64 - 1)
SEEDS128 = (2 ** 64, 2 ** 96 + 3, 2 ** 128 - 1)
RANGE_BASES = (2 ** 32 - 3, 2 ** 64 - 3)
SPAWN_ENTROPY = (0, 5, 2 ** 64 + 1, 2 ** 127 + 9)
SPAWN_KEY0 = (0, 2 ** 32 - 2)


def words(x) -> np.ndarray:
    """numpy's PCG64 state words for a seed (an int or a SeedSequence)."""
    return rng_words_from_generator(np.random.PCG64(x))


def numpy_rows(seeds) -> np.ndarray:
    return np.stack([words(s) for s in seeds]) if len(seeds) else np.zeros((0, 5), np.uint64)


def pack(seeds, seed_words):
    if seed_words == 1:
        return np.array(seeds, dtype=np.uint64)
    return np.array([[s & M64, s >> 64] for s in seeds], dtype=np.uint64)


def cycle(values, m):
    return [values[j % len(values)] for j in range(m)]


def spawn_rows(entropy, keys) -> np.ndarray:
    return numpy_rows([np.random.SeedSequence(entropy, spawn_key=key) for key in keys])


def cases(m):
    """The issue's cases at m rows (the array forms repeat their seeds cyclically)."""
    out = []
    s64, s128 = cycle(SEEDS64, m), cycle(SEEDS128 + SEEDS64[:3], m)
    out.append(("int64", dict(mode=SEED_INT, seeds=pack(s64, 1), seed_words=1), numpy_rows(s64)))
    out.append(("int128", dict(mode=SEED_INT, seeds=pack(s128, 2), seed_words=2), numpy_rows(s128)))
    for b in RANGE_BASES:
        out.append((f"range{b:#x}", dict(mode=SEED_INT, base=b), numpy_rows(range(b, b + m))))
    for e in SPAWN_ENTROPY:
        for k0 in SPAWN_KEY0:
            out.append((f"spawn{e:#x}+{k0:#x}", dict(mode=SEED_SPAWN, base=e, key0=k0),
                        spawn_rows(e, [(k0 + j,) for j in range(m)])))
    e, k0, k1, period = 2 ** 64 + 1, 2 ** 33, 2 ** 32 - 2, 3
    out.append(("spawn2", dict(mode=SEED_SPAWN, base=e, key0=k0, key1=k1, period=period),
                spawn_rows(e, [(k0 + j // period, k1 + j % period) for j in range(m)])))
    return out


# (name, m, call): every call tmg_seed must refuse with a negative return.
# "rng" None stands for the null output pointer.
REFUSED = (
    ("seed_words0", 4, dict(seed_words=0)),
    ("seed_words3", 4, dict(seed_words=3)),
    ("null_rng", 4, dict(rng=None)),
    ("negative_m", -1, dict()),
    ("negative_period", 4, dict(mode=SEED_SPAWN, period=-1)),
    ("mode2", 4, dict(mode=2)),
    ("mode-1", 4, dict(mode=-1)),
    ("both_stores", 4, dict(mode=0x300)),
    ("key0_wraps", 4, dict(mode=SEED_SPAWN, key0=2 ** 64 - 3)),
    ("key0_wraps_period", 7, dict(mode=SEED_SPAWN, key0=2 ** 64 - 2, period=3)),
    ("key1_wraps_period", 7, dict(mode=SEED_SPAWN, key1=2 ** 64 - 2, period=3)),
    ("key1_wraps_short", 3, dict(mode=SEED_SPAWN, key1=2 ** 64 - 2, period=5)),
    ("base_wraps", 2, dict(mode=SEED_INT, base=2 ** 128 - 1)),
)
# the same edges, one short of wrapping: accepted
EDGES = (
    ("key0_edge", 3, dict(mode=SEED_SPAWN, base=1, key0=2 ** 64 - 3),
     lambda: spawn_rows(1, [(2 ** 64 - 3 + j,) for j in range(3)])),
    ("key_edge_period", 6, dict(mode=SEED_SPAWN, base=1, key0=2 ** 64 - 2, key1=2 ** 64 - 3, period=3),
     lambda: spawn_rows(1, [(2 ** 64 - 2 + j // 3, 2 ** 64 - 3 + j % 3) for j in range(6)])),
    ("base_edge", 2, dict(mode=SEED_INT, base=2 ** 128 - 2), lambda: numpy_rows([2 ** 128 - 2, 2 ** 128 - 1])),
)
