// tmg_kernels.hip — kernel instantiations and their host launchers
// (tmg_launch.h).  Compiled once per translation unit, TMG_TU = 1..15, so the
// heavy template instantiations build in parallel; each TU registers only its
// own kernels.
#include <hip/hip_runtime.h>

#include "tmg_board.hip"
#include "tmg_dispatch.h"
#include "tmg_launch.h"
#if TMG_TU == 1
#if TMG_COVER
// the lane kernel's sites, counted per lane: each lane is an env of its own
#define TMG_LANE_COVER_PTR 1
#define TMG_LANE_COVER(g, site)                                                                         \
    do {                                                                                                \
        if ((g).cover) atomicAdd((g).cover + (tmg::CV_LANE_STEP + (site)), 1ULL);                       \
    } while (0)
#endif
#include "tmg_lane.h"
#endif
#if TMG_TU == 6
#include "tmg_aux.hip"      // non-template kernels: one TU only
#endif

#if TMG_TU == 12
#include "tmg_expand.hip"   // tmg_expand's count / scan and gather kernels
#endif

#ifndef TMG_TU
#error "compile tmg_kernels.hip with -DTMG_TU=1..15"
#endif

namespace tmg {

namespace {

// The launchers the ladders of tmg_dispatch.h call: each member enqueues the
// one instantiation the ladder picked.
struct StepLaunch {
    dim3 grid;
    hipStream_t s;
    const Params &P;
    const StepArgs &a;
    template <int MAXN, bool GEN, int NB, bool CODD, int FIX>
    void step() {
        const size_t lds = sizeof(Ws<MAXN, GEN>);
        hipLaunchKernelGGL((step_kernel<MAXN, GEN, NB, CODD, FIX>), grid, dim3(64), lds, s, P, a.n, a.board, a.rng,
                           a.timer, a.actions, a.reward, a.n_new, a.n_act, a.flags, a.eff, a.trust_eff, a.autoreset);
    }
    template <int FIX>
    void step_plain() {
        const size_t lds = sizeof(Ws<128, false>);
        const PlainHot H{(int32_t)a.n, (int32_t)(grid.x >> 3), P.num_moves - 1, a.autoreset, a.actions, a.timer, a.eff,
                         a.reward, a.n_new, a.n_act, a.flags, a.board, a.rng};
        hipLaunchKernelGGL((plain_step_kernel<FIX>), grid, dim3(64), lds, s, H, P);
    }
};

template <int MAXN>
void spill_one(hipStream_t s, const Params &P, const StepArgs &a) {
    const size_t lds = sizeof(Ws<MAXN, false>);
    hipLaunchKernelGGL((spill_kernel<MAXN>), dim3(kSpillWaves), dim3(64), lds, s, P, a.n, a.board, a.rng, a.timer,
                       a.actions, a.reward, a.n_new, a.n_act, a.flags, a.eff, a.trust_eff, a.autoreset);
}

struct ResetLaunch {
    dim3 grid;
    hipStream_t s;
    const Params &P;
    int64_t n;
    int8_t *board;
    uint64_t *rng;
    int32_t *timer;
    uint64_t *eff;
    const uint8_t *env_mask;
    int mask_bits, epw;
    template <int MAXN, int NB, bool CODD, int FIX>
    void reset() {
        const size_t lds = sizeof(Ws<MAXN, false>);
        hipLaunchKernelGGL((reset_kernel<MAXN, NB, CODD, FIX>), grid, dim3(64), lds, s, P, n, board, rng, timer, eff,
                           env_mask, mask_bits, epw);
    }
};

struct EffectiveLaunch {
    dim3 grid;
    hipStream_t s;
    const Params &P;
    int64_t n;
    const int8_t *board;
    uint64_t *eff;
    template <int MAXN>
    void effective() {
        hipLaunchKernelGGL(effective_kernel<MAXN>, grid, dim3(64), sizeof(Ws<MAXN, false>), s, P, n, board, eff);
    }
};

struct PeekLaunch {
    dim3 grid;
    hipStream_t s;
    const Params &P;
    const PeekArgs &a;
    template <int MAXN, bool GEN, int NB, bool CODD>
    void peek() {
        const size_t lds = sizeof(Ws<MAXN, GEN>);
        hipLaunchKernelGGL((peek_kernel<MAXN, GEN, NB, CODD>), grid, dim3(64), lds, s, P, a.n, a.board, a.rng, a.eff,
                           a.trust_eff, a.reward, a.n_new, a.n_act, a.flags, a.best_action, a.best_reward);
    }
};

template <int MAXN>
void peek_spill_one(hipStream_t s, const Params &P, const PeekArgs &a) {
    const size_t lds = sizeof(Ws<MAXN, false>);
    hipLaunchKernelGGL((peek_spill_kernel<MAXN>), dim3(kSpillWaves), dim3(64), lds, s, P, a.n, a.board, a.rng, a.eff,
                       a.trust_eff, a.reward, a.n_new, a.n_act, a.flags, a.best_action, a.best_reward);
}

// tmg_rollout takes peek's dispatch (peek_ladder): peek<...>() launches the
// rollout kernel of the same instantiation
struct RollLaunch {
    dim3 grid;
    hipStream_t s;
    const Params &P;
    const RollArgs &a;
    template <int MAXN, bool GEN, int NB, bool CODD>
    void peek() {
        const size_t lds = sizeof(Ws<MAXN, GEN>);
        hipLaunchKernelGGL((rollout_kernel<MAXN, GEN, NB, CODD>), grid, dim3(64), lds, s, P, a);
    }
};

template <int MAXN>
void rollout_spill_one(hipStream_t s, const Params &P, const RollArgs &a) {
    const size_t lds = sizeof(Ws<MAXN, false>);
    hipLaunchKernelGGL((rollout_spill_kernel<MAXN>), dim3(kSpillWaves), dim3(64), lds, s, P, a);
}

// tmg_playout takes peek's dispatch too: peek<...>() launches the playout
// kernel of the same instantiation
struct PlayLaunch {
    dim3 grid;
    hipStream_t s;
    const Params &P;
    const PlayArgs &a;
    template <int MAXN, bool GEN, int NB, bool CODD>
    void peek() {
        const size_t lds = sizeof(Ws<MAXN, GEN>);
        hipLaunchKernelGGL((playout_kernel<MAXN, GEN, NB, CODD>), grid, dim3(64), lds, s, P, a);
    }
};

template <int MAXN>
void playout_spill_one(hipStream_t s, const Params &P, const PlayArgs &a) {
    const size_t lds = sizeof(Ws<MAXN, false>);
    hipLaunchKernelGGL((playout_spill_kernel<MAXN>), dim3(kSpillWaves), dim3(64), lds, s, P, a);
}

// tmg_trace: the two general non-bitboard kernels and their spill tier
template <int MAXN>
void trace_one(dim3 grid, hipStream_t s, const Params &P, const TraceArgs &a) {
    const size_t lds = sizeof(Ws<MAXN, true>);
    hipLaunchKernelGGL((trace_kernel<MAXN>), grid, dim3(64), lds, s, P, a);
}
template <int MAXN>
void trace_spill_one(hipStream_t s, const Params &P, const TraceArgs &a) {
    const size_t lds = sizeof(Ws<MAXN, false>);
    hipLaunchKernelGGL((trace_spill_kernel<MAXN>), dim3(kSpillWaves), dim3(64), lds, s, P, a);
}

}  // namespace

#if TMG_TU == 15
void launch_trace(int maxn, dim3 grid, hipStream_t s, const Params &P, const TraceArgs &a) {
    if (maxn == 128) trace_one<128>(grid, s, P, a);
    else trace_one<512>(grid, s, P, a);
}
void launch_trace_spill(int maxn, hipStream_t s, const Params &P, const TraceArgs &a) {
    if (maxn == 128) trace_spill_one<128>(s, P, a);
    else trace_spill_one<512>(s, P, a);
}
#endif

#if TMG_TU == 13
void launch_playout_lean(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PlayArgs &a) {
    PlayLaunch l{grid, s, P, a};
    peek_lean_ladder(P, maxn, sb, l);
}
void launch_playout_spill128(hipStream_t s, const Params &P, const PlayArgs &a) { playout_spill_one<128>(s, P, a); }
void launch_playout_spill512(hipStream_t s, const Params &P, const PlayArgs &a) { playout_spill_one<512>(s, P, a); }
#endif

#if TMG_TU == 14
void launch_playout_gen(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PlayArgs &a) {
    PlayLaunch l{grid, s, P, a};
    peek_gen_ladder(P, maxn, sb, l);
}
#endif

#if TMG_TU == 10
void launch_rollout_lean(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const RollArgs &a) {
    RollLaunch l{grid, s, P, a};
    peek_lean_ladder(P, maxn, sb, l);
}
void launch_rollout_spill128(hipStream_t s, const Params &P, const RollArgs &a) { rollout_spill_one<128>(s, P, a); }
void launch_rollout_spill512(hipStream_t s, const Params &P, const RollArgs &a) { rollout_spill_one<512>(s, P, a); }
#endif

#if TMG_TU == 11
void launch_rollout_gen(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const RollArgs &a) {
    RollLaunch l{grid, s, P, a};
    peek_gen_ladder(P, maxn, sb, l);
}
#endif

#if TMG_TU == 12
void launch_expand_count(hipStream_t s, const ExpandCountArgs &a) {
    const unsigned tiles = (unsigned)((a.n + kExpandTile - 1) / kExpandTile);
    if (tiles) hipLaunchKernelGGL(expand_count_kernel<0>, dim3(tiles), dim3(64), 0, s, a);
    hipLaunchKernelGGL(expand_count_kernel<1>, dim3(1), dim3(64), 0, s, a);
    if (tiles) hipLaunchKernelGGL(expand_count_kernel<2>, dim3(tiles), dim3(64), 0, s, a);
}
void launch_expand_gather(int maxn, hipStream_t s, const ExpandArgs &a) {
    const dim3 grid = env_grid(a.n);
    if (maxn == 128) hipLaunchKernelGGL((expand_gather_kernel<1, kExpandPack>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((expand_gather_kernel<4, kExpandPack>), grid, dim3(64), 0, s, a);
}
#endif

#if TMG_TU == 8
void launch_peek_lean(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PeekArgs &a) {
    PeekLaunch l{grid, s, P, a};
    peek_lean_ladder(P, maxn, sb, l);
}
void launch_peek_spill128(hipStream_t s, const Params &P, const PeekArgs &a) { peek_spill_one<128>(s, P, a); }
void launch_peek_spill512(hipStream_t s, const Params &P, const PeekArgs &a) { peek_spill_one<512>(s, P, a); }
#endif

#if TMG_TU == 9
void launch_peek_gen(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PeekArgs &a) {
    PeekLaunch l{grid, s, P, a};
    peek_gen_ladder(P, maxn, sb, l);
}
#endif

#if TMG_TU == 1
// The lane-per-board lean step (tmg_lane.h): EPW envs per one-wave
// workgroup (lane i < EPW = env EPW * group + i), the groups in wg_env's
// XCD-blocked order.  Each lane keeps kLaneScratch bytes of LDS for a
// shuffle's index array (the rare path).  EPW is 64, or 32 for a launch of
// fewer than kLaneSmallEnvs envs (tmg_dispatch.h).
#ifndef TMG_LANE_WPE
#define TMG_LANE_WPE 0          // amdgpu_waves_per_eu(WPE, WPE) when > 0 (A/B)
#endif
#ifndef TMG_LANE_LDS
#define TMG_LANE_LDS 0          // extra LDS bytes per workgroup (A/B: caps workgroups per CU)
#endif
template <int R, int C, int K, int EPW>
__global__ __launch_bounds__(64)
#if TMG_LANE_WPE > 0
__attribute__((amdgpu_waves_per_eu(TMG_LANE_WPE, TMG_LANE_WPE)))
#endif
void lane_step_kernel(Params P_, int64_t n, int8_t *__restrict__ board, uint64_t *__restrict__ rng,
                      int32_t *__restrict__ timer, int32_t *__restrict__ actions, int32_t *__restrict__ reward,
                      int32_t *__restrict__ n_new, int32_t *__restrict__ n_act, uint8_t *__restrict__ flags,
                      uint64_t *__restrict__ eff, int autoreset) {
    __shared__ uint8_t scratch[EPW * kLaneScratch + TMG_LANE_LDS];
    const Params &P = TMG_KERNARG_PARAMS(P_);
    const int lane = threadIdx.x & 63;
    const int64_t e = wg_env() * EPW + lane;
    if (lane >= EPW || e >= n) return;
    static_assert(CV_LANE_STEP + lane::LC_COUNT <= CV_COUNT &&
                      CV_LANE_REJECT_REDRAW - CV_LANE_STEP == lane::LC_REJECT_REDRAW,
                  "CV_LANE_* follow tmg_lane.h's LC_* order");
#if TMG_COVER
    const lane::StepIO io{board, rng, timer, actions, reward, n_new, n_act, flags, eff,
                          P.num_moves, autoreset, P.sample, P.pol_key, P.pol_first, P.pol_t, P.cover};
#else
    const lane::StepIO io{board, rng, timer, actions, reward, n_new, n_act, flags, eff,
                          P.num_moves, autoreset, P.sample, P.pol_key, P.pol_first, P.pol_t};
#endif
    const uint32_t st = lane::step_env<lane::Board<R, C, K>>(io, e, scratch + lane * kLaneScratch);
    if (st & lane::LS_INTERNAL) P.status[0] = 1u;
    if (st & lane::LS_CALLER) P.status[2] = 1u;
}

template <int K, int EPW>
void lane_one(hipStream_t s, const Params &P, const StepArgs &a) {
    const dim3 grid = env_grid((a.n + EPW - 1) / EPW);
    int32_t *act = const_cast<int32_t *>(a.actions);            // the policy writes its draws back
    hipLaunchKernelGGL((lane_step_kernel<10, 10, K, EPW>), grid, dim3(64), 0, s, P, a.n, a.board, a.rng, a.timer,
                       act, a.reward, a.n_new, a.n_act, a.flags, a.eff, a.autoreset);
}

void launch_step_lane(hipStream_t s, const Params &P, const StepArgs &a) {
    const bool small = a.n < kLaneSmallEnvs;
    if (P.k == 4) small ? lane_one<4, 32>(s, P, a) : lane_one<4, 64>(s, P, a);
    else small ? lane_one<5, 32>(s, P, a) : lane_one<5, 64>(s, P, a);
}

void launch_step_lean128(bool sb, bool plain, dim3 grid, hipStream_t s, const Params &P, const StepArgs &a) {
    StepLaunch l{grid, s, P, a};
    step_lean128_ladder(P, sb, l, plain);
}
#endif

#if TMG_TU == 2
void launch_step_gen128_even(bool sb, dim3 grid, hipStream_t s, const Params &P, const StepArgs &a) {
    StepLaunch l{grid, s, P, a};
    step_gen128_even_ladder(P, sb, l);
}
#endif

#if TMG_TU == 7
void launch_spill128(hipStream_t s, const Params &P, const StepArgs &a) { spill_one<128>(s, P, a); }
void launch_spill512(hipStream_t s, const Params &P, const StepArgs &a) { spill_one<512>(s, P, a); }
#endif

#if TMG_TU == 3
void launch_step_gen128_odd(dim3 grid, hipStream_t s, const Params &P, const StepArgs &a) {
    StepLaunch l{grid, s, P, a};
    step_gen128_odd_ladder(P, l);
}
#endif

#if TMG_TU == 4
void launch_step512(bool gen, dim3 grid, hipStream_t s, const Params &P, const StepArgs &a) {
    StepLaunch l{grid, s, P, a};
    step512_ladder(P, gen, l);
}

void launch_reset512(dim3 grid, hipStream_t s, const Params &P, int64_t n, int8_t *board, uint64_t *rng,
                     int32_t *timer, uint64_t *eff, const uint8_t *env_mask, int mask_bits, int epw) {
    ResetLaunch l{grid, s, P, n, board, rng, timer, eff, env_mask, mask_bits, epw};
    reset512_ladder(P, l);
}
void launch_effective512(dim3 grid, hipStream_t s, const Params &P, int64_t n, const int8_t *board, uint64_t *eff) {
    EffectiveLaunch l{grid, s, P, n, board, eff};
    effective512_ladder(l);
}
#endif

#if TMG_TU == 5
void launch_reset128(bool sb, dim3 grid, hipStream_t s, const Params &P, int64_t n, int8_t *board, uint64_t *rng,
                     int32_t *timer, uint64_t *eff, const uint8_t *env_mask, int mask_bits, int epw) {
    ResetLaunch l{grid, s, P, n, board, rng, timer, eff, env_mask, mask_bits, epw};
    reset128_ladder(P, sb, l);
}
void launch_effective128(dim3 grid, hipStream_t s, const Params &P, int64_t n, const int8_t *board, uint64_t *eff) {
    EffectiveLaunch l{grid, s, P, n, board, eff};
    effective128_ladder(l);
}
#endif

#if TMG_TU == 6
void launch_onehot(hipStream_t s, int64_t n, int N, int k, int nsel, int4 sel, const int8_t *board, void *out,
                   int dtype) {
    const int64_t cells = n * N;
    const dim3 grid((unsigned)((cells + 255) / 256)), block(256);
    switch (dtype) {
    case 0: hipLaunchKernelGGL(onehot_kernel<float>, grid, block, 0, s, n, N, k, nsel, sel, board, (float *)out); break;
    case 1: hipLaunchKernelGGL(onehot_kernel<uint8_t>, grid, block, 0, s, n, N, k, nsel, sel, board, (uint8_t *)out); break;
    default: hipLaunchKernelGGL(onehot_kernel<int32_t>, grid, block, 0, s, n, N, k, nsel, sel, board, (int32_t *)out); break;
    }
}
void launch_sample_effective(hipStream_t s, int64_t n, int W, int A, const uint64_t *eff, uint64_t key,
                             int64_t first_env, int32_t t, int32_t *actions) {
    constexpr int BS = TMG_SAMPLE_BS;
    const dim3 grid((unsigned)((n + BS - 1) / BS)), block(BS);
    hipLaunchKernelGGL((sample_effective_kernel<BS, TMG_SAMPLE_LDS != 0>), grid, block, 0, s, n, W, A, eff, key,
                       first_env, t, actions);
}
void launch_count_states(int R, int C, int k, uint64_t total, uint64_t per, uint64_t threads,
                         unsigned long long *counts) {
    const CountGeo G = make_count_geo(R, C, k);
    hipLaunchKernelGGL(count_states_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, G, total, per,
                       counts);
}
void launch_seed(hipStream_t s, const SeedArgs &a, int store) {
    constexpr int BS = TMG_SEED_BS;
    const dim3 grid((unsigned)((a.m + BS - 1) / BS)), block(BS);
    const bool stage = store ? store == 2 : TMG_SEED_LDS != 0;
    if (stage) hipLaunchKernelGGL((seed_kernel<BS, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((seed_kernel<BS, false>), grid, block, 0, s, a);
}
void launch_rollout_reduce(hipStream_t s, int64_t n, int A, int samples, const int32_t *ret, int32_t *total,
                           int32_t *best_action, int32_t *best_total) {
    hipLaunchKernelGGL(rollout_reduce_kernel, env_grid(n), dim3(64), 0, s, n, A, samples, ret, total, best_action,
                       best_total);
}
void launch_playout_reduce(hipStream_t s, int64_t n, int seqs, const int32_t *ret, int32_t *best_seq,
                           int32_t *best_ret) {
    hipLaunchKernelGGL(playout_reduce_kernel, env_grid(n), dim3(64), 0, s, n, seqs, ret, best_seq, best_ret);
}
#endif

}  // namespace tmg
