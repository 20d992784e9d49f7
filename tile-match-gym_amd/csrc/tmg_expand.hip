// tmg_expand.hip — tmg_expand_count / tmg_expand: the successor states of
// every effective action, as rows a step kernel can run on.  Two kernels, both
// plain HBM streaming with no LDS, and neither plays a move: the moves are the
// library's own step kernels, run by tmg_capi.hip on the rows written here
// (a wave that plays an env's ~43 moves one after another
// lost to "step on copies" twice, §7.10 / §7.11).  Include after tmg_board.hip
// (wg_env, rdlane64, popc_below).  Every kernel is a template, so the file can
// be included by any translation unit; TU 12 of tmg_kernels.hip launches them.
//
// expand_count_kernel<PHASE>: first_child[i] = children of envs 0..i-1, an
// exclusive prefix sum in int64 over all n envs, in three launches of one-wave
// workgroups with first_child itself as the only workspace.  A workgroup owns
// a tile of kExpandTile consecutive envs (lane l: envs l, l + 64, ... of it).
//   phase 0: the tile's child count into its first slot, first_child[tile * T];
//   phase 1: one workgroup turns those slots into exclusive tile offsets, 64
//            at a time, and writes the total to first_child[n];
//   phase 2: each tile reads its offset, counts again and writes the slot of
//            every env of it (its first slot gets the value it already holds).
// Every sum is taken in a fixed order, so the result does not depend on the
// schedule.  A tile holds < 2^20 children and 64 tiles < 2^26: the wave scans
// are 32-bit, the running offsets 64-bit.
//
// expand_gather_kernel<ND, PACK>: one wave per parent env (peek's frame
// without the moves).  The board is read from HBM once, lane l keeping dwords
// l, l + 64, ... of it (peek_dwords: ND = 1 up to 128 cells, 4 up to 512); the
// mask row sits in one register per lane; the timer and first_child[e] are
// wave-uniform.  The env's children are consecutive rows of every child
// array, so with PACK the wave writes each array as one run: the board bytes
// of all the env's children are the parent's board repeated, and lane l of
// pass p stores dword (64 p + l) mod nd of it, fetched from the lane that
// holds it (ds_bpermute) — 50 dwords per 10x10 board would leave 14 lanes of a
// one-child store idle, 8 dwords per 4x4 board 56.  The RNG words, the mask
// rows, the timers and the parents leave the same way, and the actions as one
// store per mask word (lane b: the action of bit b, at the rank of that bit).
// Without PACK the wave walks the children and writes one row per pass
// (TMG_EXPAND_PACK, measured in DESIGN.md §7.14).  Boards of more than 128
// cells fill whole stores already and go child by child either way, as do
// boards whose 2N bytes are no multiple of 4: their child rows start on 2-byte
// boundaries and are written as 2-byte halves (load_board / store_board take
// bytes for the same reason; the parent is read as bytes here too).
// Rows [first_child[n], m) belong to no env: a grid-stride loop of the same
// launch gives them timer = num_moves, action 0, parent -1 and a zero mask, so
// the step that follows treats them as steps after done and reads nothing else.
#pragma once

namespace tmg {

#ifndef TMG_EXPAND_PACK
#define TMG_EXPAND_PACK 1
#endif
constexpr bool kExpandPack = TMG_EXPAND_PACK != 0;
constexpr int kExpandTile = 1024;        // envs per workgroup of the count kernels: 16 per lane

struct ExpandCountArgs {
    int64_t n;
    int W, A, num_moves;
    const int32_t *timer;
    const uint64_t *eff;
    const uint64_t *select;              // [n][W] or null
    int64_t *first_child;                // [n + 1]
};

struct ExpandArgs {
    int64_t n, m;
    int N, W, A, num_moves;
    const int8_t *board;
    const uint64_t *rng;
    const int32_t *timer;
    const uint64_t *eff;
    const uint64_t *select;              // [n][W] or null
    const int64_t *first_child;          // [n + 1]
    int8_t *child_board;
    uint64_t *child_rng;
    int32_t *child_timer;
    uint64_t *child_eff;
    int64_t *child_parent;               // or null
    int32_t *child_action;
};

// the bits of mask word w that name an action (w < W, so at least one)
__device__ __forceinline__ uint64_t expand_word_bits(int A, int w) {
    const int left = A - 64 * w;
    return left >= 64 ? ~0ULL : (1ULL << left) - 1ULL;
}

// children of env i: its effective (and selected) actions, none once it is finished
__device__ __forceinline__ int expand_children(const ExpandCountArgs &a, int64_t i) {
    if (a.timer[i] >= a.num_moves) return 0;
    int c = 0;
    for (int w = 0; w < a.W; w++) {
        uint64_t x = a.eff[i * a.W + w] & expand_word_bits(a.A, w);
        if (a.select) x &= a.select[i * a.W + w];
        c += __popcll(x);
    }
    return c;
}

// inclusive sum over the lanes up to this one (log-step, ds_bpermute)
__device__ __forceinline__ int expand_wave_scan(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __builtin_amdgcn_ds_bpermute(((lane - d) & 63) << 2, v);
        if (lane >= d) v += t;
    }
    return v;
}

template <int PHASE>
__global__ __launch_bounds__(64) void expand_count_kernel(ExpandCountArgs a) {
    const int lane = threadIdx.x & 63;
    if constexpr (PHASE == 1) {
        const int64_t tiles = (a.n + kExpandTile - 1) / kExpandTile;
        int64_t run = 0;
        for (int64_t t0 = 0; t0 < tiles; t0 += 64) {
            const int64_t t = t0 + lane;
            const int v = t < tiles ? (int)a.first_child[t * kExpandTile] : 0;
            const int incl = expand_wave_scan(v, lane);
            if (t < tiles) a.first_child[t * kExpandTile] = run + (incl - v);
            run += __builtin_amdgcn_readlane(incl, 63);
        }
        if (lane == 0) a.first_child[a.n] = run;
    } else {
        const int64_t base = (int64_t)blockIdx.x * kExpandTile;
        if (base >= a.n) return;
        int64_t run = 0;
        if constexpr (PHASE == 2) run = a.first_child[base];      // read by every lane before any of them writes it
        int mine = 0;
        for (int j = 0; j < kExpandTile && base + j < a.n; j += 64) {
            const int64_t i = base + j + lane;
            const int c = i < a.n ? expand_children(a, i) : 0;
            if constexpr (PHASE == 0) {
                mine += c;
            } else {
                const int incl = expand_wave_scan(c, lane);
                if (i < a.n) a.first_child[i] = run + (incl - c);
                run += __builtin_amdgcn_readlane(incl, 63);
            }
        }
        if constexpr (PHASE == 0) {
            const int tot = __builtin_amdgcn_readlane(expand_wave_scan(mine, lane), 63);
            if (lane == 0) a.first_child[base] = tot;
        }
    }
}

__device__ __forceinline__ uint64_t expand_bperm64(int src, uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// dst[q] = the word lane q mod period holds, for q in [0, words): whole coalesced passes
__device__ __forceinline__ void expand_fill64(uint64_t *__restrict__ dst, int words, int period, uint64_t v,
                                              int lane) {
    int r = lane % period;
    const int step = 64 % period;
    for (int q0 = 0; q0 < words; q0 += 64) {
        const uint64_t x = expand_bperm64(r, v);
        if (q0 + lane < words) dst[q0 + lane] = x;
        r += step;
        if (r >= period) r -= period;
    }
}

template <int ND, bool PACK>
__global__ __launch_bounds__(64) void expand_gather_kernel(ExpandArgs a) {
    const int lane = threadIdx.x & 63;
    const int N = a.N, W = a.W;
    {   // the rows past the last child
        int64_t total = a.first_child[a.n];
        if (total < 0) total = 0;
        for (int64_t c = total + (int64_t)blockIdx.x * 64 + lane; c < a.m; c += (int64_t)gridDim.x * 64) {
            a.child_timer[c] = a.num_moves;
            a.child_action[c] = 0;
            if (a.child_parent) a.child_parent[c] = -1;
            for (int w = 0; w < W; w++) a.child_eff[c * W + w] = 0ULL;
        }
    }
    const int64_t e = wg_env();
    if (e >= a.n) return;
    const int64_t c0 = a.first_child[e];
    const int t0 = a.timer[e];
    if (t0 >= a.num_moves || c0 < 0 || c0 >= a.m) return;          // wave-uniform
    uint64_t effrow = 0ULL, selrow = 0ULL, rngw = 0ULL;
    if (lane < W) {
        effrow = a.eff[e * W + lane];
        selrow = effrow & expand_word_bits(a.A, lane);
        if (a.select) selrow &= a.select[e * W + lane];
    }
    if (lane < 5) rngw = a.rng[e * 5 + lane];
    // the board, once: whole dwords (the last one of an odd N is zero-filled)
    const int nb = 2 * N, nd = (nb + 3) >> 2;
    const bool wide = (nb & 3) == 0;
    const int8_t *gb = a.board + e * nb;
    uint32_t keep[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) {
        const int d = i * 64 + lane;
        keep[i] = 0u;
        if (d < nd) {
            if (wide) {
                keep[i] = reinterpret_cast<const uint32_t *>(gb)[d];
            } else {
                for (int b = 0; b < 4; b++)
                    if (4 * d + b < nb) keep[i] |= (uint32_t)(uint8_t)gb[4 * d + b] << (8 * b);
            }
        }
    }
    // the actions, a mask word at a time: bit b's child sits at the rank of b
    int cnt = 0;
    for (int wi = 0; wi < W; wi++) {
        const uint64_t mw = rdlane64(selrow, wi);
        const int64_t c = c0 + cnt + popc_below(mw);
        if (((mw >> lane) & 1ULL) && c < a.m) a.child_action[c] = wi * 64 + lane;
        cnt += __popcll(mw);
    }
    const int lim = (int)(a.m - c0 < (int64_t)cnt ? a.m - c0 : (int64_t)cnt);   // rows of this env below m
    if (lim <= 0) return;
    if (PACK && wide && ND == 1) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(a.child_board + c0 * nb);
        const int words = lim * nd;
        int r = lane % nd;
        const int step = 64 % nd;
        for (int q0 = 0; q0 < words; q0 += 64) {
            const uint32_t x = (uint32_t)__builtin_amdgcn_ds_bpermute(r << 2, (int)keep[0]);
            if (q0 + lane < words) dst[q0 + lane] = x;
            r += step;
            if (r >= nd) r -= nd;
        }
    } else if (wide) {
        for (int j = 0; j < lim; j++) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(a.child_board + (c0 + j) * nb);
#pragma unroll
            for (int i = 0; i < ND; i++) {
                const int d = i * 64 + lane;
                if (d < nd) dst[d] = keep[i];
            }
        }
    } else {
        for (int j = 0; j < lim; j++) {
            uint16_t *dst = reinterpret_cast<uint16_t *>(a.child_board + (c0 + j) * nb);
#pragma unroll
            for (int i = 0; i < ND; i++) {
                const int h = 2 * (i * 64 + lane);                  // N halves per row
                if (h < N) dst[h] = (uint16_t)keep[i];
                if (h + 1 < N) dst[h + 1] = (uint16_t)(keep[i] >> 16);
            }
        }
    }
    if (PACK) {
        expand_fill64(a.child_rng + c0 * 5, lim * 5, 5, rngw, lane);
        expand_fill64(a.child_eff + c0 * W, lim * W, W, effrow, lane);
        for (int j = lane; j < lim; j += 64) {
            a.child_timer[c0 + j] = t0;
            if (a.child_parent) a.child_parent[c0 + j] = e;
        }
    } else {
        for (int j = 0; j < lim; j++) {
            const int64_t c = c0 + j;
            if (lane < 5) a.child_rng[c * 5 + lane] = rngw;
            if (lane < W) a.child_eff[c * W + lane] = effrow;
            if (lane == 0) {
                a.child_timer[c] = t0;
                if (a.child_parent) a.child_parent[c] = e;
            }
        }
    }
}

}  // namespace tmg
