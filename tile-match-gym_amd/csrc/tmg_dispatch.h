// tmg_dispatch.h — which kernel instantiation runs for a call: the one
// statement of the rule, shared by libtmg.so (tmg_capi.hip decides the route,
// each translation unit of tmg_kernels.hip walks its own ladder) and by the
// host wave emulator (tools/wave_emu), which runs the same route and ladders
// on fibers.  Host code only, nothing of the HIP runtime: plain functions of
// Params, and ladders templated over a launcher object that knows how to start
// (or record) step<MAXN, GEN, NB, CODD, FIX>(), reset<MAXN, NB, CODD, FIX>()
// and effective<MAXN>().  Include after tmg_board.hip (Params, shape_fix, the
// kFix* constants, sb_planes).
#pragma once
#include <stdint.h>

namespace tmg {

// ------------------------------------------------------------------ knobs
// Each overridable with -D for an A/B build (scripts/build_ab.sh).

// The lane-per-board kernel (tmg_lane.h) takes the lean steps of the shapes
// it is built for (lane_shape), unless a fused output (one-hot, vector-env
// outputs) is asked for, when its lanes are busy: the in-kernel policy (every
// move effective) or a launch of >= kLaneMinEnvs envs.  With given actions on
// smaller launches the wave-per-board kernels are faster (a lane's wave runs
// as long as its longest cascade, and at c2's 65 536 envs there is one such
// wave per SIMD: DESIGN.md §7.7).
#ifndef TMG_LANE
#define TMG_LANE 1
#endif
#ifndef TMG_LANE_MIN_ENVS
#define TMG_LANE_MIN_ENVS 131072
#endif
constexpr bool kLaneKernel = TMG_LANE != 0;
constexpr int64_t kLaneMinEnvs = TMG_LANE_MIN_ENVS;
// A lane wave lasts as long as its longest cascade, so a launch too small to
// give each SIMD two waves of 64 takes 32 envs per wave (c2's 21 845-env group
// launches: c2-eff +4.5 %; at c4's 43 690 the 64-env waves are 4.5 % faster,
// profiles/r06/s12/).
#ifndef TMG_LANE_SMALL
#define TMG_LANE_SMALL 32768
#endif
constexpr int64_t kLaneSmallEnvs = TMG_LANE_SMALL;    // launches below this many envs: 32 envs per wave
// After a lane step the masked reset takes 2 envs per wave, not 8: the block
// storms (a whole env group's regeneration) dominate its time there (c2-eff
// 5.45 vs 5.19, c4-eff 9.9 vs 9.45 x 10^8 on one box; 1 / 4 in between,
// profiles/r06/s13/).
#ifndef TMG_LANE_RESET_EPW
#define TMG_LANE_RESET_EPW 2
#endif
constexpr int kLaneResetEnvs = TMG_LANE_RESET_EPW;
// Envs per wave of a masked reset_kernel launch (the deferred autoreset after a
// general step; 29 of 30 find no finished env).  10x10 boards: 1 / 2 / 4 / 8 /
// 16 measured c3 6.97 / 7.10 / 7.19 / 7.17 / 7.15 x 10^8; 20x20 boards, whose
// regenerations are long: 2 (4 made the storm 4 % slower).
constexpr int kMaskedResetEnvs128 = 8;
constexpr int kMaskedResetEnvs512 = 2;
// The general kernels (low occupancy, long waves) take the policy's draw from
// the sampler kernel ahead of them; the lean ones sample in their own
// prologue.  1: the general kernels sample in-kernel too (A/B).
#ifndef TMG_GEN_SAMPLE
#define TMG_GEN_SAMPLE 0
#endif
constexpr bool kGenSampleInKernel = TMG_GEN_SAMPLE != 0;

// ------------------------------------------------------------------ route
// the kernel family of a board: <= 128 cells or <= 512
inline int shape_maxn(const Params &P) { return P.N <= 128 ? 128 : 512; }
// the scalar-bitboard kernels (tmg_sb.hip): <= 128 cells, a row fits a word
inline bool shape_sb(const Params &P) { return P.N <= 128 && P.C <= 63; }
// the shapes lane_step_kernel is instantiated for
inline bool lane_shape(const Params &P) {
    return P.smask == 0 && P.R == 10 && P.C == 10 && (P.k == 4 || P.k == 5);
}
// whether a fused output (one-hot, vector-env outputs) is asked for
inline bool fused_output(const Params &P) {
    return P.oh || P.vo_term || P.vo_mask || P.vo_left || P.vo_final || P.vo_obs;
}

// The lean kernels take a step when no special can exist (none enabled) and
// the cached mask came from this library's own step / reset of the current
// boards; the general kernels take every other, with the spill tier behind.
inline bool lean_step(const Params &P, int trust_eff) { return P.smask == 0 && trust_eff; }

// whether P is the shape a FIX instantiation was compiled for
template <int FIX>
bool is_shape(const Params &P) {
    const int sm = (FIX & 255) == kFixAnySpecials ? kFixAnySpecials : P.smask;
    return shape_fix(P.R, P.C, P.k, sm) == FIX;
}

// The plain step kernel (plain_step_kernel, tmg_board.hip) takes the c2-shape
// lean steps with given actions and no fused output: c2 and the c4 shard.  It
// addresses an env's rows by 32-bit byte offsets, so the launch may hold at
// most kPlainMaxEnvs envs: the widest rows are the board's 2 N bytes, the RNG
// state's 40 and the mask's 8 W.
constexpr int64_t kPlainMaxEnvs = 1 << 23;
constexpr int64_t plain_max_offset(int R, int C) {      // the largest byte offset of a row's end, any array
    const int64_t N = R * C, W = (2 * N - R - C + 63) / 64;
    const int64_t row = 2 * N > 40 ? (2 * N > 8 * W ? 2 * N : 8 * W) : (40 > 8 * W ? 40 : 8 * W);
    return kPlainMaxEnvs * row;
}
static_assert(plain_max_offset(kFixC2 >> 24, (kFixC2 >> 16) & 255) < (1LL << 31),
              "every env's byte offset (e * 2N, e * 40, e * 8W, e * 4) stays below 2^31");
inline bool plain_step(const Params &P, int trust_eff, int64_t n) {
    return is_shape<kFixC2>(P) && lean_step(P, trust_eff) && !P.sample && !fused_output(P) && n <= kPlainMaxEnvs;
}

// Envs per wave of a reset_kernel launch: a masked reset (the deferred
// autoreset after a step; most find no finished env) takes several, a full one
// 1.  override > 0: the caller's own count for a masked launch.
inline int reset_envs_per_wave(int maxn, bool masked, int override = 0) {
    return !masked ? 1 : override ? override : maxn == 128 ? kMaskedResetEnvs128 : kMaskedResetEnvs512;
}

// Whether the sampler kernel draws the policy's actions ahead of the step
// (the step then runs with P.sample = 0).
inline bool sample_ahead(const Params &P, int trust_eff) {
    return P.sample && !kGenSampleInKernel && !lean_step(P, trust_eff);
}

struct StepRoute {
    bool lean;              // lean_step: the lean kernels, not the general ones
    bool lane;             // the lane-per-board kernel instead of the wave-per-board ladder
    bool plain;             // plain_step: the ladder's plain instantiation of the c2 kernel (never with lane)
    bool deferred;          // finished boards are left to a reset launch masked by FL_RESET
    bool spill;             // spill_kernel follows (the general kernels: steps that ran out of LDS lists)
    int kernel_autoreset;   // the kernel's code (step_env): 0 none, 1 / 3 inline, 2 / 4 deferred
    int reset_epw;          // envs per wave of the deferred reset (0: none)
};

// mode: 0 none, 1 same step, 2 next step (tmg_plan_config); n: envs of the
// launch; have_lane: the caller has the lane kernel (the library; not the
// emulator).  The general and 512-cell kernels, and the lane kernel, leave
// finished boards to a masked reset launch, which runs at several times their
// occupancy; only the 128-cell lean kernels regenerate inline.
inline StepRoute route_step(const Params &P, int maxn, int trust_eff, int mode, int64_t n, bool have_lane) {
    StepRoute r;
    r.lean = lean_step(P, trust_eff);
    r.lane = have_lane && kLaneKernel && r.lean && maxn == 128 && lane_shape(P) && !fused_output(P) &&
             (P.sample || n >= kLaneMinEnvs);
    r.plain = !r.lane && maxn == 128 && plain_step(P, trust_eff, n);
    r.deferred = mode && (maxn == 512 || !r.lean || r.lane);
    r.spill = !r.lean;
    r.kernel_autoreset = mode == 0 ? 0 : mode == 1 ? (r.deferred ? 2 : 1) : (r.deferred ? 4 : 3);
    r.reset_epw = r.deferred ? reset_envs_per_wave(maxn, true, r.lane ? kLaneResetEnvs : 0) : 0;
    return r;
}

// The wave-per-board step kernels live in four groups, one translation unit
// of tmg_kernels.hip each (tmg_launch.h).
enum class StepGroup { Lean128, Gen128Even, Gen128Odd, Step512 };
inline StepGroup step_group(const Params &P, int maxn, bool sb, bool lean) {
    if (maxn != 128) return StepGroup::Step512;
    if (lean) return StepGroup::Lean128;
    return sb && (P.C & 1) ? StepGroup::Gen128Odd : StepGroup::Gen128Even;
}

// ---------------------------------------------------------------- ladders
// One per launcher group; each calls exactly one member of the launcher, and
// names only its own group's instantiations.

// scalar-bitboard step variants: NB colour planes (sb_planes(k))
template <bool GEN, bool CODD, class L>
void step_sb_ladder(const Params &P, L &l) {
    switch (sb_planes(P.k)) {
    case 1: l.template step<128, GEN, 1, CODD, kNoFix>(); break;
    case 2: l.template step<128, GEN, 2, CODD, kNoFix>(); break;
    case 3: l.template step<128, GEN, 3, CODD, kNoFix>(); break;
    default: l.template step<128, GEN, 4, CODD, kNoFix>(); break;
    }
}

// plain: StepRoute::plain; step_plain<FIX>() starts plain_step_kernel<FIX>,
// the plain form of step<128, false, 2, false, FIX>
template <class L>
void step_lean128_ladder(const Params &P, bool sb, L &l, bool plain = false) {
    if (!sb) l.template step<128, false, 0, false, kNoFix>();
    else if (is_shape<kFixC2>(P) && plain) l.template step_plain<kFixC2>();
    else if (is_shape<kFixC2>(P)) l.template step<128, false, 2, false, kFixC2>();
    else if (P.C & 1) step_sb_ladder<false, true>(P, l);
    else step_sb_ladder<false, false>(P, l);
}

// C even, and the non-bitboard general kernel
template <class L>
void step_gen128_even_ladder(const Params &P, bool sb, L &l) {
    if (!sb) l.template step<128, true, 0, false, kNoFix>();
    else if (is_shape<kFixC3>(P)) l.template step<128, true, 2, false, kFixC3>();
    else step_sb_ladder<true, false>(P, l);
}

template <class L>
void step_gen128_odd_ladder(const Params &P, L &l) {
    step_sb_ladder<true, true>(P, l);
}

template <class L>
void step512_ladder(const Params &P, bool gen, L &l) {
    if (!gen) l.template step<512, false, 0, false, kNoFix>();
    else if (is_shape<kFixC5>(P)) l.template step<512, true, 0, false, kFixC5>();
    else l.template step<512, true, 0, false, kNoFix>();
}

template <bool CODD, class L>
void reset_sb_ladder(const Params &P, L &l) {
    switch (sb_planes(P.k)) {
    case 1: l.template reset<128, 1, CODD, kNoFix>(); break;
    case 2: l.template reset<128, 2, CODD, kNoFix>(); break;
    case 3: l.template reset<128, 3, CODD, kNoFix>(); break;
    default: l.template reset<128, 4, CODD, kNoFix>(); break;
    }
}

template <class L>
void reset128_ladder(const Params &P, bool sb, L &l) {
    if (!sb) l.template reset<128, 0, false, kNoFix>();
    else if (is_shape<kFixReset10>(P)) l.template reset<128, 2, false, kFixReset10>();
    else if (P.C & 1) reset_sb_ladder<true>(P, l);
    else reset_sb_ladder<false>(P, l);
}

// NB = colour bit-planes of the row-plane generate (bp_generate)
template <class L>
void reset512_ladder(const Params &P, L &l) {
    if (is_shape<kFixReset20>(P)) { l.template reset<512, 3, false, kFixReset20>(); return; }
    switch (sb_planes(P.k)) {
    case 1: l.template reset<512, 1, false, kNoFix>(); break;
    case 2: l.template reset<512, 2, false, kNoFix>(); break;
    case 3: l.template reset<512, 3, false, kNoFix>(); break;
    default: l.template reset<512, 4, false, kNoFix>(); break;
    }
}

// tmg_peek (tmg_peek.hip): the route rule of a step (lean_step, shape_sb,
// shape_maxn, sb_planes, C odd), generic instantiations only, in two launcher
// groups: the lean kernels, and the general ones with the spill tier behind.
// peek<MAXN, GEN, NB, CODD>()
template <bool GEN, bool CODD, class L>
void peek_sb_ladder(const Params &P, L &l) {
    switch (sb_planes(P.k)) {
    case 1: l.template peek<128, GEN, 1, CODD>(); break;
    case 2: l.template peek<128, GEN, 2, CODD>(); break;
    case 3: l.template peek<128, GEN, 3, CODD>(); break;
    default: l.template peek<128, GEN, 4, CODD>(); break;
    }
}
template <bool GEN, class L>
void peek_group_ladder(const Params &P, int maxn, bool sb, L &l) {
    if (maxn != 128) l.template peek<512, GEN, 0, false>();
    else if (!sb) l.template peek<128, GEN, 0, false>();
    else if (P.C & 1) peek_sb_ladder<GEN, true>(P, l);
    else peek_sb_ladder<GEN, false>(P, l);
}
template <class L>
void peek_lean_ladder(const Params &P, int maxn, bool sb, L &l) { peek_group_ladder<false>(P, maxn, sb, l); }
template <class L>
void peek_gen_ladder(const Params &P, int maxn, bool sb, L &l) { peek_group_ladder<true>(P, maxn, sb, l); }

template <class L>
void effective128_ladder(L &l) { l.template effective<128>(); }
template <class L>
void effective512_ladder(L &l) { l.template effective<512>(); }

// The whole rule for a caller that holds every group at once (the emulator;
// the library's groups sit behind the launch_* functions of tmg_launch.h).
template <class L>
void step_ladder(const Params &P, int maxn, bool sb, bool lean, L &l, bool plain = false) {
    switch (step_group(P, maxn, sb, lean)) {
    case StepGroup::Lean128: step_lean128_ladder(P, sb, l, plain); break;
    case StepGroup::Gen128Even: step_gen128_even_ladder(P, sb, l); break;
    case StepGroup::Gen128Odd: step_gen128_odd_ladder(P, l); break;
    case StepGroup::Step512: step512_ladder(P, !lean, l); break;
    }
}
template <class L>
void reset_ladder(const Params &P, int maxn, bool sb, L &l) {
    if (maxn == 128) reset128_ladder(P, sb, l);
    else reset512_ladder(P, l);
}
// lean: lean_step(P, trust_eff); the general kernels are followed by the peek spill pass
template <class L>
void peek_ladder(const Params &P, int maxn, bool sb, bool lean, L &l) {
    if (lean) peek_lean_ladder(P, maxn, sb, l);
    else peek_gen_ladder(P, maxn, sb, l);
}
template <class L>
void effective_ladder(int maxn, L &l) {
    if (maxn == 128) effective128_ladder(l);
    else effective512_ladder(l);
}

}  // namespace tmg
