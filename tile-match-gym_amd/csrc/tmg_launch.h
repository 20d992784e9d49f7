// tmg_launch.h — host-side launchers of the kernels, one group per
// translation unit of tmg_kernels.hip (compiled once per TMG_TU value, in
// parallel), called by tmg_capi.hip.  Each launcher enqueues its kernel(s) on
// `s` and returns nothing; tmg_capi checks hipGetLastError afterwards.  Which
// group a call goes to (route_step, step_group) and which instantiation a
// group launches (the *_ladder functions) is decided in tmg_dispatch.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace tmg {

struct Params;

struct StepArgs {
    int64_t n;
    int8_t *board;
    uint64_t *rng;
    int32_t *timer;
    const int32_t *actions;
    int32_t *reward, *n_new, *n_act;
    uint8_t *flags;
    uint64_t *eff;
    int trust_eff, autoreset;
};

// one wave per env: grid padded to 8 equal XCD blocks (wg_env0)
dim3 env_grid(int64_t n);

// TU 1 — lean step kernels (no specials, cached mask trusted), <= 128 cells;
// sb: scalar-bitboard variants (C <= 63); plain: StepRoute::plain (tmg_dispatch.h)
void launch_step_lean128(bool sb, bool plain, dim3 grid, hipStream_t s, const Params &P, const StepArgs &a);
// and the lane-per-board lean step (tmg_lane.h) for the shapes lane_shape
// (tmg_dispatch.h) accepts; its autoreset codes are the deferred ones (0, 2, 4)
void launch_step_lane(hipStream_t s, const Params &P, const StepArgs &a);
constexpr int kLaneScratch = 128;      // LDS bytes per lane (a shuffle's index array, N <= 128)
// TU 2 / 3 — general <= 128-cell step kernels, C even / odd (the
// non-bitboard one lives in TU 2)
void launch_step_gen128_even(bool sb, dim3 grid, hipStream_t s, const Params &P, const StepArgs &a);
void launch_step_gen128_odd(dim3 grid, hipStream_t s, const Params &P, const StepArgs &a);
// TU 4 — 512-cell kernels
void launch_step512(bool gen, dim3 grid, hipStream_t s, const Params &P, const StepArgs &a);
// TU 7 — the spill tier (steps whose cascade outgrew the LDS lists)
void launch_spill128(hipStream_t s, const Params &P, const StepArgs &a);
void launch_spill512(hipStream_t s, const Params &P, const StepArgs &a);
void launch_reset512(dim3 grid, hipStream_t s, const Params &P, int64_t n, int8_t *board, uint64_t *rng,
                     int32_t *timer, uint64_t *eff, const uint8_t *env_mask, int mask_bits, int epw);
void launch_effective512(dim3 grid, hipStream_t s, const Params &P, int64_t n, const int8_t *board, uint64_t *eff);
// TU 5 — <= 128-cell reset / effective kernels
void launch_reset128(bool sb, dim3 grid, hipStream_t s, const Params &P, int64_t n, int8_t *board, uint64_t *rng,
                     int32_t *timer, uint64_t *eff, const uint8_t *env_mask, int mask_bits, int epw);
void launch_effective128(dim3 grid, hipStream_t s, const Params &P, int64_t n, const int8_t *board, uint64_t *eff);
// TU 6 — the callers either side (tmg_aux.hip)
void launch_onehot(hipStream_t s, int64_t n, int N, int k, int nsel, int4 sel, const int8_t *board, void *out,
                   int dtype);
void launch_sample_effective(hipStream_t s, int64_t n, int W, int A, const uint64_t *eff, uint64_t key,
                             int64_t first_env, int32_t t, int32_t *actions);
void launch_count_states(int R, int C, int k, uint64_t total, uint64_t per, uint64_t threads,
                         unsigned long long *counts);
// tmg_seed (tmg_seed.h); store: 0 the default variant, 1 direct, 2 staged
struct SeedArgs;
void launch_seed(hipStream_t s, const SeedArgs &a, int store);

// tmg_peek (tmg_peek.hip): every action's outcome, no state written
struct PeekArgs {
    int64_t n;
    const int8_t *board;
    const uint64_t *rng;
    const uint64_t *eff;
    int trust_eff;
    int32_t *reward, *n_new, *n_act;
    uint8_t *flags;
    int32_t *best_action, *best_reward;
};
// TU 8 — lean peek kernels (both families), and the peek spill tier
void launch_peek_lean(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PeekArgs &a);
void launch_peek_spill128(hipStream_t s, const Params &P, const PeekArgs &a);
void launch_peek_spill512(hipStream_t s, const Params &P, const PeekArgs &a);
// TU 9 — general peek kernels (both families)
void launch_peek_gen(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PeekArgs &a);

// tmg_rollout (tmg_rollout.hip): every action's policy rollout, no state
// written.  grid: env_grid(n * samples), one wave per virtual env
struct RollArgs;
// TU 10 — lean rollout kernels (both families), and the rollout spill tier
void launch_rollout_lean(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const RollArgs &a);
void launch_rollout_spill128(hipStream_t s, const Params &P, const RollArgs &a);
void launch_rollout_spill512(hipStream_t s, const Params &P, const RollArgs &a);
// TU 11 — general rollout kernels (both families)
void launch_rollout_gen(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const RollArgs &a);
// TU 6 — the sums over the samples (tmg_aux.hip)
void launch_rollout_reduce(hipStream_t s, int64_t n, int A, int samples, const int32_t *ret, int32_t *total,
                           int32_t *best_action, int32_t *best_total);

// tmg_playout (tmg_playout.hip): given action sequences played on copies of
// every env.  grid: env_grid(n * seqs), one wave per virtual env
struct PlayArgs;
// TU 13 — lean playout kernels (both families), and the playout spill tier
void launch_playout_lean(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PlayArgs &a);
void launch_playout_spill128(hipStream_t s, const Params &P, const PlayArgs &a);
void launch_playout_spill512(hipStream_t s, const Params &P, const PlayArgs &a);
// TU 14 — general playout kernels (both families)
void launch_playout_gen(int maxn, bool sb, dim3 grid, hipStream_t s, const Params &P, const PlayArgs &a);
// TU 6 — the best sequence per env (tmg_aux.hip)
void launch_playout_reduce(hipStream_t s, int64_t n, int seqs, const int32_t *ret, int32_t *best_seq,
                           int32_t *best_ret);

// tmg_trace (tmg_trace.hip): one move's cascade stage by stage on copies of
// every env.  grid: env_grid(n * seqs), one wave per virtual env
struct TraceArgs;
// TU 15 — the general non-bitboard trace kernels (128 / 512 cells) and their spill tier
void launch_trace(int maxn, dim3 grid, hipStream_t s, const Params &P, const TraceArgs &a);
void launch_trace_spill(int maxn, hipStream_t s, const Params &P, const TraceArgs &a);

// tmg_expand_count / tmg_expand (tmg_expand.hip): the child rows of every
// effective action, counted and placed on the device; the moves themselves
// are a step launch on those rows (tmg_capi.hip)
struct ExpandCountArgs;
struct ExpandArgs;
// TU 12 — the count / scan launches (n == 0: first_child[0] = 0 only) and the
// gather, one wave per parent env
void launch_expand_count(hipStream_t s, const ExpandCountArgs &a);
void launch_expand_gather(int maxn, hipStream_t s, const ExpandArgs &a);

// bytes of one spill-kernel wave's worst-case global-memory lists
size_t spill_ws_bytes(int maxn);

}  // namespace tmg
