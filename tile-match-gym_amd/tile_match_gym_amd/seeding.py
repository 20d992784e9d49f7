"""Per-env RNG state: numpy Generator(PCG64) packed as 5 uint64 words.

The reference drives all board randomness from ONE ``np.random.default_rng(seed)``
per env (tile_match_env.py:49-51, set_seed :79-82).  The device keeps that
stream bit-exactly; its state per env is

    words[0:2] = 128-bit LCG state (lo, hi)
    words[2:4] = 128-bit increment (lo, hi)
    words[4]   = has_uint32 << 32 | uinteger   (numpy's persistent 32-bit half-word buffer)

Seeding uses numpy's own SeedSequence -> PCG64 (numpy, not reference code).
"""
from __future__ import annotations

import numpy as np

_M64 = (1 << 64) - 1


def rng_words_from_generator(gen) -> np.ndarray:
    bg = gen.bit_generator if isinstance(gen, np.random.Generator) else gen
    st = bg.state
    if st.get("bit_generator") != "PCG64":
        raise ValueError(f"only PCG64 generators are supported, got {st.get('bit_generator')}")
    s, inc = st["state"]["state"], st["state"]["inc"]
    return np.array([s & _M64, s >> 64, inc & _M64, inc >> 64,
                     (int(st["has_uint32"]) << 32) | int(st["uinteger"])], dtype=np.uint64)


def rng_words_from_seed(seed) -> np.ndarray:
    """== np.random.default_rng(seed) state (tile_match_env.py:49)."""
    return rng_words_from_generator(np.random.PCG64(seed))


def generator_from_words(words) -> np.random.Generator:
    w = [int(x) for x in np.asarray(words, dtype=np.uint64)]
    bg = np.random.PCG64()
    bg.state = {"bit_generator": "PCG64",
                "state": {"state": w[0] | (w[1] << 64), "inc": w[2] | (w[3] << 64)},
                "has_uint32": (w[4] >> 32) & 1, "uinteger": w[4] & 0xFFFFFFFF}
    return np.random.Generator(bg)


def pack_seeds(seeds):
    """How the device seeds `seeds` (tmg_seed, include/tmg.h), or None when only
    the host can (batch_rng_words):

        ("range", base, m)   consecutive ints base .. base + m - 1, nothing to upload
        ("array", a)         a: uint64 (m,) for seeds below 2^64, else (m, 2) lo / hi

    Taken: a range of step 1, and a list / tuple / integer ndarray (torch
    tensors: pass their .cpu().numpy()) of non-negative ints below 2^128.  A
    negative seed raises ValueError, as np.random.default_rng does.  Anything
    else — a seed of 2^128 or more, a non-integer element, any other iterable,
    which is left untouched — gives None."""
    if isinstance(seeds, range):
        if len(seeds) == 0:
            return "range", 0, 0
        if seeds.step != 1:
            seeds = list(seeds)
        elif seeds.start < 0:
            raise ValueError("seeds must be non-negative")
        elif seeds.stop > 1 << 128:
            return None
        else:
            return "range", seeds.start, len(seeds)
    if isinstance(seeds, np.ndarray) and seeds.dtype.kind in "iu":
        if seeds.ndim != 1:
            return None
        if seeds.size and seeds.min() < 0:
            raise ValueError("seeds must be non-negative")
        return "array", np.ascontiguousarray(seeds.astype(np.uint64))
    if isinstance(seeds, np.ndarray) and seeds.dtype == object and seeds.ndim == 1:
        seeds = seeds.tolist()
    if not isinstance(seeds, (list, tuple)):
        return None
    if not all(isinstance(s, (int, np.integer)) and not isinstance(s, (bool, np.bool_)) for s in seeds):
        return None
    vals = [int(s) for s in seeds]
    if vals and min(vals) < 0:
        raise ValueError("seeds must be non-negative")
    top = max(vals, default=0)
    if top < 1 << 64:
        return "array", np.array(vals, dtype=np.uint64)
    if top < 1 << 128:
        return "array", np.array([[v & _M64, v >> 64] for v in vals], dtype=np.uint64)
    return None


def batch_rng_words(seeds) -> np.ndarray:
    """(N,5) uint64 state words for a sequence of integer seeds."""
    seeds = list(seeds)
    out = np.empty((len(seeds), 5), dtype=np.uint64)
    for i, s in enumerate(seeds):
        out[i] = rng_words_from_seed(int(s))
    return out
