// tmg_rollout.hip — tmg_rollout: the simulation step of a Monte-Carlo planner.
// For every env i, sample s and action a: play a on a copy of the board with
// a copy of the RNG words rng[s][i], then continue with the examples' policy
// (uniform over the effective actions, tmg_sample_effective's draw) until the
// horizon, and report the summed eliminations.  Included by tmg_board.hip after
// tmg_peek.hip, whose layout this file keeps: one wave per *virtual env*
// v = s * n + i (board / mask / timer row i, RNG and output row v), the board
// in LDS with a pristine copy in registers, the mask walked word by word, lane
// j keeping the outcome of action 64 * w + j, one coalesced store per output
// array per word.  The per-action body is a ply loop: every move leaves the
// final board's mask in w.effw, the next action is drawn from it in-wave, and
// the RNG stream runs on from ply to ply.
#pragma once

// tmg_sample_effective's pick for one mask row (sample_action with the 32-bit
// draw h given): the r-th set bit, r = h * count >> 32; -1 when no bit is set.
// effrow: lane i holds mask word i (W <= 64).
__device__ __forceinline__ int sample_action_h(const Params &P, uint64_t effrow, uint32_t h, int lane) {
    const int W = P.W;
    const int pc = __popcll(effrow);                    // 0 on lanes >= W
    int count = 0;
    for (int j = 0; j < W; j++) count += __builtin_amdgcn_readlane(pc, j);
    if (count == 0) return -1;
    int r = (int)(((uint64_t)h * (uint64_t)count) >> 32);
    int j = 0;
    for (; j < W - 1; j++) {
        const int c = __builtin_amdgcn_readlane(pc, j);
        if (r < c) break;
        r -= c;
    }
    const uint64_t x = rdlane64(effrow, j);
    const bool hit = ((x >> lane) & 1ULL) && popc_below(x) == r;
    return j * 64 + __ffsll((unsigned long long)__ballot(hit)) - 1;
}

// The call's arguments (by value to the kernels, after Params).  The policy's
// key / first_env / t travel in Params::pol_key / pol_first / pol_t.
struct RollArgs {
    int64_t n;                    // real envs; the launch covers n * samples virtual envs
    int samples, depth;
    const int8_t *board;          // [n]
    const uint64_t *rng;          // [samples][n][5]
    const int32_t *timer;         // [n] or null (no horizon)
    const uint64_t *eff;          // [n][W] (trust_eff != 0)
    int trust_eff;
    int32_t *ret, *plies;         // [samples][n][A], each or null
    uint8_t *flags;               // [samples][n][A] or null
};

// one mask word's outcomes: lane j holds action base + j of virtual env v
__device__ __forceinline__ void roll_store_word(const Params &P, const RollArgs &a, int lane, int64_t v, int base, int r,
                                                int np, int fl) {
    const int act = base + lane;
    if (act < P.A) {
        const int64_t o = v * P.A + act;
        if (a.ret) a.ret[o] = r;
        if (a.plies) a.plies[o] = np;
        if (a.flags) a.flags[o] = (uint8_t)fl;
    }
}

// Every action's rollout of virtual env v.  Template parameters as peek_env;
// returns the ST_* bits for the sticky status word.  TIER_MAIN with GEN: the
// first ply whose cascade outgrows the LDS lists queues v for
// rollout_spill_kernel and abandons it (outputs written so far are rewritten
// there).
template <int MAXN, bool GEN, int SBNB, bool CODD, int TIER = TIER_MAIN, class WS = Ws<MAXN, GEN>,
          class L = WsSerial<MAXN>>
__device__ __forceinline__ uint32_t rollout_env(const Params &P, const RollArgs &a, WS &w, int lane, int64_t v,
                                                L *lists) {
    constexpr int ND = peek_dwords<MAXN>();
    const int N = P.N, W = P.W;
    const int s = (int)(v / a.n);
    const int64_t e = v - (int64_t)s * a.n;
    // the horizon: the episode ends when the timer reaches num_moves (tile_match_env.py:100-101)
    int H = a.depth;
    if (a.timer) H = min(H, P.num_moves - __builtin_amdgcn_readfirstlane(a.timer[e]));
    if (H <= 0) {                                  // a finished env
        for (int wi = 0; wi < W; wi++) roll_store_word(P, a, lane, v, wi * 64, 0, 0, 0);
        return 0;
    }
    const int8_t *gb = a.board + e * 2 * N;
    uint64_t effrow = 0ULL;
    if (a.trust_eff && lane < W) effrow = a.eff[e * W + lane];
    constexpr bool RP = SBNB > 0 && !GEN;
    bool rowp = false;
    if constexpr (RP) rowp = rp_shape(P);
    load_board(P, w, lane, gb);
    if constexpr (TIER == TIER_SPILL) COVER(CV_ROLL_SPILL_RUN);
    WSYNC();
    const int nd = (2 * N + 3) >> 2;               // the pristine copy, as peek_env keeps it
    uint32_t keep[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) {
        const int d = i * 64 + lane;
        keep[i] = d < nd ? reinterpret_cast<const uint32_t *>(w.brd)[d] : 0u;
    }
    if constexpr (!GEN) {                                                   // lean variant precondition (step_env)
        bool ok = true;
        for (int p = lane; p < N; p += 64) ok &= w.brd[N + p] == 1;
        if (__ballot(!ok) != 0ULL) {
            for (int wi = 0; wi < W; wi++) roll_store_word(P, a, lane, v, wi * 64, 0, 0, FL_ERR);
            return ST_INTERNAL;
        }
    }
    if (!a.trust_eff) {                            // the mask of the board as it stands (it may hold a line)
        scan_effective(P, w, lane, make_cells<MAXN / 64>(P, lane), false);
        WSYNC();
        effrow = lane < W ? w.effw[lane] : 0ULL;
    }
    // As peek_env: the lean kernels rebuild this lane's jump-table row and cell
    // coordinates per move through an opaque lane index (kept live across the
    // moves they spill) and reload the RNG words per action; the general
    // kernels keep all of it.  An action's RNG words stay live across its plies.
    constexpr bool RELOAD = !GEN;
    Rng g0{};
    LaneJump J0{};
    Cells<MAXN / 64> cl0{};
    const uint64_t *rv = a.rng + v * 5;
    if constexpr (!RELOAD) {
        g0 = load_rng(rv);
        J0 = load_jump(P, lane, g0, rowp);
        cl0 = make_cells<MAXN / 64>(P, lane);
    }
    const uint64_t gid = (uint64_t)(P.pol_first + e);
    uint32_t st = 0;
    for (int wi = 0; wi < W; wi++) {
        uint64_t m = rdlane64(effrow, wi);
        int kr = 0, kp = 0, kf = 0;                // lane j: the outcome of action 64 * wi + j
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const int a0 = wi * 64 + j;
            const uint64_t key = P.pol_key + (uint64_t)s * (uint64_t)P.A + (uint64_t)a0;
            Rng g = g0;
            if constexpr (RELOAD) g = load_rng(rv + (loop_lane(lane) >> 6));   // lane < 64: cache hits after the first action
            WSYNC();                               // the move before is done with the board
#pragma unroll
            for (int i = 0; i < ND; i++) {
                const int d = i * 64 + lane;
                if (d < nd) reinterpret_cast<uint32_t *>(w.brd)[d] = keep[i];
            }
            int act = a0, tot = 0, fl = 0, np = 0;
            for (int d = 0; d < H; d++) {
                if (d > 0) {
                    // the policy's draw from the mask the ply before left (its
                    // move ended on a wave barrier)
                    const uint64_t row = lane < W ? w.effw[lane] : 0ULL;
                    const uint32_t h = (uint32_t)policy_draw(key, gid, P.pol_t + d);
                    act = __builtin_amdgcn_readfirstlane(sample_action_h(P, row, h, lane));
                    if (act < 0) { fl |= FL_ERR; break; }                   // unreachable: a move leaves a playable board
                    COVER(CV_ROLL_PLY);
                }
                LaneJump J = J0;
                Cells<MAXN / 64> cl = cl0;
                if constexpr (RELOAD) {
                    const int ll = loop_lane(lane);
                    J = load_jump(P, ll, g, rowp);
                    cl = make_cells<MAXN / 64>(P, ll);
                }
                if constexpr (GEN) {
                    for (int p = lane; p < N; p += 64) w.mark[p] = 0;
                }
                WSYNC();
                int flags = 0, nn = 0, na = 0, elim;
                int r1, c1, r2, c2;
                action_coords(P.R, P.C, act, r1, c1, r2, c2);
                const int p1 = r1 * P.C + c1, p2 = r2 * P.C + c2;
                // plies >= 1 run on a line-free board this file's moves left:
                // the bounded first line search applies whatever trust_eff is
                if constexpr (RP) {
                    if (rowp) elim = rp_move<SBNB, CODD>(P, w, lane, J, g, cl, p1, p2, flags);
                    else elim = sb_move<SBNB, CODD>(P, w, lane, J, g, cl, p1, p2, flags, e);
                } else elim = board_move<MAXN, GEN, SBNB, CODD, TIER>(P, w, lane, J, g, cl, p1, p2, flags, nn, na, e, lists,
                                                                     d > 0 || a.trust_eff != 0);
                if constexpr (GEN) {
                    if (flags & FL_OVF) {
                        // as peek_env: the queue holds every virtual env of the
                        // launch and WsSerialBig cannot run out
                        if constexpr (TIER == TIER_MAIN) {
                            if (queue_env(P.spill, lane, v)) { COVER(CV_ROLL_SPILL); return st; }
                        }
                        flags = (flags & ~FL_OVF) | FL_ERR;
                    }
                }
                tot += elim;
                fl |= flags;
                np++;
                if (flags & FL_ERR) break;         // a safety cap: the rollout stops here
            }
            if (H < a.depth) COVER(CV_ROLL_HORIZON);
            if (fl & FL_ERR) st |= ST_INTERNAL;
            if (lane == j) { kr = tot; kp = np; kf = fl; }
        }
        roll_store_word(P, a, lane, v, wi * 64, kr, kp, kf);
    }
    return st;
}

// Occupancy.  Lean: 5 / 4 waves per SIMD (96 VGPRs with 164 B of scratch / 128 with 32 B)
// measured 20.2 / 17.5 ms per c2 launch at depth 4; general: 5 / 4 measured 206.7 / 220.5 ms at c3.
#ifndef TMG_ROLL_LEAN_WAVES
#define TMG_ROLL_LEAN_WAVES 4
#endif
#ifndef TMG_ROLL_GEN_WAVES
#define TMG_ROLL_GEN_WAVES 5
#endif
#ifndef TMG_ROLL_512_WAVES
#define TMG_ROLL_512_WAVES TMG_PEEK_512_WAVES
#endif
constexpr int kRollLean128Waves = TMG_ROLL_LEAN_WAVES;   // rollout_kernel<128, false>
constexpr int kRollGen128Waves = TMG_ROLL_GEN_WAVES;     // rollout_kernel<128, true>
constexpr int kRoll512Waves = TMG_ROLL_512_WAVES;        // rollout_kernel<512, *>

// tmg_rollout over a batch, one wave per virtual env: peek's instantiations
template <int MAXN, bool GEN, int SBNB = 0, bool CODD = false>
__global__ __launch_bounds__(64, MAXN == 128 ? (GEN ? kRollGen128Waves : kRollLean128Waves) : kRoll512Waves) void rollout_kernel(
    Params P_, RollArgs a) {
    TMG_SMEM_DECL(smem);
    using WS = Ws<MAXN, GEN>;
    const Params &P = TMG_KERNARG_PARAMS(P_);
    const int lane = threadIdx.x & 63;
    WS &w = *reinterpret_cast<WS *>(smem);
    const int64_t v = wg_env();
    if (v >= a.n * a.samples) return;
    WsSerial<MAXN> *lists = nullptr;
    if constexpr (GEN) lists = &w.s;
    const uint32_t st = rollout_env<MAXN, GEN, SBNB, CODD, TIER_MAIN, WS, WsSerial<MAXN>>(P, a, w, lane, v, lists);
    note_status(P, lane, st);
}

// every rollout of the virtual envs rollout_kernel<*, true> queued (spill_drain)
template <int MAXN>
__global__ __launch_bounds__(64, 8) void rollout_spill_kernel(Params P, RollArgs a) {
    spill_drain<MAXN>(P, a.n * a.samples, [&](Ws<MAXN, false> &w, int lane, int64_t v, WsSerialBig<MAXN> *lists) {
        return rollout_env<MAXN, true, 0, false, TIER_SPILL, Ws<MAXN, false>, WsSerialBig<MAXN>>(P, a, w, lane, v, lists);
    });
}
