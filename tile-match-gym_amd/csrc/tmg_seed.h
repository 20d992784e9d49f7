// tmg_seed.h — numpy's SeedSequence -> PCG64 seeding of one stream, bit-exact,
// as one __host__ __device__ function: the seed kernel (tmg_aux.hip), the host
// wave emulator and a plain host program run the same code.
//
// np.random.default_rng(seed) is PCG64(SeedSequence(seed)) (tile_match_env.py:49,
// set_seed :79-82).  SeedSequence (numpy/random/bit_generator.pyx) turns the
// entropy and the spawn key into little-endian uint32 words (0 is one word,
// else the minimal count), hashes them into a pool of four uint32 and
// generates four uint64 from the pool; PCG64 takes them as initstate (v0:v1)
// and initseq (v2:v3) of pcg_setseq_128_srandom.
//
// Assembled words: the entropy's, and with a spawn key the entropy zero-padded
// to four words followed by each key element's one or two words.  The pool's
// first pass hashes words 0..3 with missing ones as 0, so of all lengths only
// a key element's word count changes the result.  Up to 128 bits of entropy
// and two key elements below 2^64: at most eight words, all in registers.
#pragma once
#include <stdint.h>

#include "pcg64.h"

namespace tmg {

// SeedSequence's hashmix with its running multiplier (INIT_A / MULT_A, and
// INIT_B / MULT_B for generate_state; XSHIFT = 16)
__host__ __device__ __forceinline__ uint32_t seed_hashmix(uint32_t v, uint32_t &hash_const, uint32_t mult) {
    v ^= hash_const;
    hash_const *= mult;
    v *= hash_const;
    return v ^ (v >> 16);
}

__host__ __device__ __forceinline__ uint32_t seed_mix(uint32_t x, uint32_t y) {
    const uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
    return r ^ (r >> 16);
}

// The five rng words (state lo / hi, inc lo / hi, empty half-word buffer) of
// PCG64(SeedSequence(ent, spawn_key=key[:nkey])), nkey in 0..2.
__host__ __device__ inline void seed_pcg64(U128 ent, int nkey, uint64_t key0, uint64_t key1, uint64_t out[5]) {
    uint32_t pool[4] = {(uint32_t)ent.lo, (uint32_t)(ent.lo >> 32), (uint32_t)ent.hi, (uint32_t)(ent.hi >> 32)};
    uint32_t hc = 0x43b0d7e5u;
    for (int i = 0; i < 4; i++) pool[i] = seed_hashmix(pool[i], hc, 0x931e8875u);
    for (int src = 0; src < 4; src++)
        for (int dst = 0; dst < 4; dst++)
            if (dst != src) pool[dst] = seed_mix(pool[dst], seed_hashmix(pool[src], hc, 0x931e8875u));
    // the words beyond the fourth: the key elements', low word first
    for (int e = 0; e < 2; e++) {
        const uint64_t key = e ? key1 : key0;
        for (int h = 0; h < 2; h++) {
            if (e >= nkey || (h && !(key >> 32))) continue;
            const uint32_t word = (uint32_t)(h ? key >> 32 : key);
            for (int dst = 0; dst < 4; dst++) pool[dst] = seed_mix(pool[dst], seed_hashmix(word, hc, 0x931e8875u));
        }
    }
    // generate_state(4, uint64)
    uint32_t g[8];
    hc = 0x8b51f9ddu;
    for (int i = 0; i < 8; i++) g[i] = seed_hashmix(pool[i & 3], hc, 0x58f38dedu);
    const U128 initstate{g[2] | (uint64_t)g[3] << 32, g[0] | (uint64_t)g[1] << 32};     // v0 << 64 | v1
    const U128 initseq{g[6] | (uint64_t)g[7] << 32, g[4] | (uint64_t)g[5] << 32};       // v2 << 64 | v3
    // pcg_setseq_128_srandom_r: state = 0, step, += initstate, step
    const U128 A{PCG_A_LO, PCG_A_HI};
    const U128 inc{(initseq.lo << 1) | 1ULL, (initseq.hi << 1) | (initseq.lo >> 63)};
    U128 s = inc;                                                                        // 0 * A + inc
    s = add128(s, initstate);
    s = add128(mul128(s, A), inc);
    out[0] = s.lo;
    out[1] = s.hi;
    out[2] = inc.lo;
    out[3] = inc.hi;
    out[4] = 0;
}

// tmg_seed's row j (include/tmg.h): which stream it is.
struct SeedArgs {
    int64_t m;
    int spawn;                 // TMG_SEED_SPAWN
    const uint64_t *seeds;     // TMG_SEED_INT: [m] or [m][2]; null: base + j
    int seed_words;
    uint64_t base_lo, base_hi;
    uint64_t key0, key1;
    int64_t period;
    uint64_t *rng;             // [m][5]
};

__host__ __device__ inline void seed_row(const SeedArgs &a, int64_t j, uint64_t out[5]) {
    if (a.spawn) {
        const U128 ent{a.base_lo, a.base_hi};
        if (a.period > 0) seed_pcg64(ent, 2, a.key0 + (uint64_t)(j / a.period), a.key1 + (uint64_t)(j % a.period), out);
        else seed_pcg64(ent, 1, a.key0 + (uint64_t)j, 0, out);
    } else if (a.seeds) {
        const U128 ent = a.seed_words == 2 ? U128{a.seeds[2 * j], a.seeds[2 * j + 1]} : U128{a.seeds[j], 0};
        seed_pcg64(ent, 0, 0, 0, out);
    } else {
        seed_pcg64(add128(U128{a.base_lo, a.base_hi}, U128{(uint64_t)j, 0}), 0, 0, 0, out);
    }
}

// mode bits of tmg_seed (include/tmg.h: TMG_SEED_SPAWN, TMG_SEED_STORE_*)
constexpr int kSeedSpawn = 1, kSeedStoreDirect = 0x100, kSeedStoreStaged = 0x200;

// Why tmg_seed refuses a call (null: it does not), *code its return value.
// Host: the library and the host emulator refuse alike.
inline const char *seed_refusal(int64_t m, int mode, const uint64_t *seeds, int seed_words, uint64_t base_lo,
                                uint64_t base_hi, uint64_t key0, uint64_t key1, int64_t period, const uint64_t *rng,
                                int *code) {
    const int store = mode & (kSeedStoreDirect | kSeedStoreStaged), kind = mode ^ store;
    *code = -2;
    if (m < 0) return "negative batch size";
    if ((kind != 0 && kind != kSeedSpawn) || store == (kSeedStoreDirect | kSeedStoreStaged)) return "unknown seed mode";
    if (seed_words != 1 && seed_words != 2) return "seed_words must be 1 or 2";
    if (period < 0) return "negative period";
    if (m > (1LL << 31)) return "m is more than one launch holds (2^31 streams)";
    if (kind == kSeedSpawn && seeds) return "TMG_SEED_SPAWN takes its entropy from base: seeds must be NULL";
    if (m > 0) {
        const uint64_t last = (uint64_t)(m - 1);
        if (kind == kSeedSpawn) {
            const uint64_t last0 = period > 0 ? last / (uint64_t)period : last;
            const uint64_t last1 = period > 0 ? (m < period ? last : (uint64_t)period - 1) : 0;
            if (key0 + last0 < key0 || key1 + last1 < key1) return "a spawn key element would pass 2^64";
        } else if (!seeds && base_hi == ~0ULL && base_lo + last < base_lo) {
            return "base + m would pass 2^128";
        }
    }
    *code = -1;
    if (!rng) return "null rng buffer";
    *code = 0;
    return nullptr;
}

}  // namespace tmg
