// tmg_playout.hip — tmg_playout: play given action sequences on copies of
// every env, the evaluation step of a shooting planner (random shooting, CEM,
// beam refinement, the replay of a recorded trajectory).  Row (q, i) is what
// successive tmg_step(autoreset = 0) calls with actions[q][i][0], [1], ...
// leave and report on a one-env copy of env i.  Included by tmg_board.hip
// after tmg_rollout.hip, whose layout this file keeps: one wave per *virtual
// env* v = q * n + i (board / mask / timer row i, actions and output row v),
// the board in LDS from the first ply to the last, the RNG words live across
// the plies, every move leaving the mask of its final board in w.effw.  There
// is one sequence per wave, so no per-action walk and no pristine copy to
// restore; what a rollout has not is the ineffective move (a ply like any
// other that changes nothing but the timer: the step kernels' quick exit,
// tested on the mask row of the board as it stands) and the final state,
// written out of LDS and registers once, after the last ply.
#pragma once

// The call's arguments (by value to the kernels, after Params).
struct PlayArgs {
    int64_t n;                    // real envs; the launch covers n * seqs virtual envs
    int seqs, depth;
    const int8_t *board;          // [n]
    const uint64_t *rng;          // [n][5], or [seqs][n][5] (rng_per_seq != 0)
    int rng_per_seq;
    const int32_t *timer;         // [n] or null (no horizon)
    const uint64_t *eff;          // [n][W] (trust_eff != 0)
    int trust_eff;
    const int32_t *actions;       // [seqs][n][depth]
    int32_t *ret, *n_new, *n_act, *plies;   // [seqs][n], each or null
    uint8_t *flags;               // [seqs][n] or null
    int32_t *ply_reward;          // [seqs][n][depth] or null
    int8_t *out_board;            // [seqs][n] final states, each or null
    uint64_t *out_rng;
    int32_t *out_timer;
    uint64_t *out_eff;
};

// Virtual env v's outputs: the sums and flags from lane 0, ply_reward's
// entries from ply np on zeroed, the final state from LDS (the board), `row`
// (lane i: mask word i; all zero when `zero`) and g.
template <class WS>
__device__ __forceinline__ void playout_store(const Params &P, const PlayArgs &a, const WS &w, int lane, int64_t v,
                                              int tot, int tn, int ta, int np, int fl, int t1, uint64_t row, bool zero,
                                              const Rng &g) {
    if (lane == 0) {
        if (a.ret) a.ret[v] = tot;
        if (a.n_new) a.n_new[v] = tn;
        if (a.n_act) a.n_act[v] = ta;
        if (a.plies) a.plies[v] = np;
        if (a.flags) a.flags[v] = (uint8_t)fl;
        if (a.out_timer) a.out_timer[v] = t1;
    }
    if (a.ply_reward) {
        for (int d = np + lane; d < a.depth; d += 64) a.ply_reward[v * a.depth + d] = 0;
    }
    if (a.out_board) store_board(P, w, lane, a.out_board + v * 2 * P.N);
    if (a.out_rng) store_rng(a.out_rng + v * 5, g, lane);
    if (a.out_eff && lane < P.W) a.out_eff[v * P.W + lane] = zero ? 0ULL : row;
}

// The sequence of virtual env v.  Template parameters as peek_env; returns the
// ST_* bits for the sticky status word.  TIER_MAIN with GEN: the first ply
// whose cascade outgrows the LDS lists queues v for playout_spill_kernel and
// abandons it (nothing but ply_reward entries has been written, and those are
// rewritten there).
template <int MAXN, bool GEN, int SBNB, bool CODD, int TIER = TIER_MAIN, class WS = Ws<MAXN, GEN>,
          class L = WsSerial<MAXN>>
__device__ __forceinline__ uint32_t playout_env(const Params &P, const PlayArgs &a, WS &w, int lane, int64_t v,
                                                L *lists) {
    const int N = P.N, W = P.W, D = a.depth;
    const int q = (int)(v / a.n);
    const int64_t e = v - (int64_t)q * a.n;
    // the horizon: the episode ends when the timer reaches num_moves (tile_match_env.py:100-101)
    const int t0 = a.timer ? __builtin_amdgcn_readfirstlane(a.timer[e]) : 0;
    int H = D;
    if (a.timer) H = min(H, P.num_moves - t0);
    const int8_t *gb = a.board + e * 2 * N;
    const uint64_t *rv = a.rng + (a.rng_per_seq ? v : e) * 5;
    const int32_t *av = a.actions + v * D;
    // the mask row of the board as it stands: lane i holds word i
    uint64_t row = 0ULL;
    if (a.trust_eff && lane < W) row = a.eff[e * W + lane];
    constexpr bool RP = SBNB > 0 && !GEN;
    bool rowp = false;
    if constexpr (RP) rowp = rp_shape(P);
    load_board(P, w, lane, gb);
    WSYNC();
    Rng g = load_rng(rv);
    if (H <= 0) {                                  // a finished env: its parent's state, a zero mask
        playout_store(P, a, w, lane, v, 0, 0, 0, 0, 0, t0, 0ULL, true, g);
        return 0;
    }
    if constexpr (!GEN) {                                                   // lean variant precondition (step_env)
        bool ok = true;
        for (int p = lane; p < N; p += 64) ok &= w.brd[N + p] == 1;
        if (__ballot(!ok) != 0ULL) {
            playout_store(P, a, w, lane, v, 0, 0, 0, 0, FL_ERR, t0, row, false, g);
            return ST_INTERNAL;
        }
    }
    if (!a.trust_eff) {                            // the mask of the board as it stands (it may hold a line)
        scan_effective(P, w, lane, make_cells<MAXN / 64>(P, lane), false);
        WSYNC();
        row = lane < W ? w.effw[lane] : 0ULL;
    }
    // As rollout_env: the lean kernels rebuild this lane's jump-table row and
    // cell coordinates per move through an opaque lane index; the general
    // kernels keep them.  The RNG words stay live across the plies.
    constexpr bool RELOAD = !GEN;
    LaneJump J0{};
    Cells<MAXN / 64> cl0{};
    if constexpr (!RELOAD) {
        J0 = load_jump(P, lane, g, rowp);
        cl0 = make_cells<MAXN / 64>(P, lane);
    }
    uint32_t st = 0;
    int tot = 0, tn = 0, ta = 0, fl = 0, np = 0;
    // the board is line-free: the caller says so (trust_eff), or a move of this
    // sequence left it.  An ineffective ply plays no move, so after any number
    // of them an untrusted board is still the caller's and may hold a line.
    bool clean = a.trust_eff != 0;
    for (int d = 0; d < H; d++) {
        const int act = __builtin_amdgcn_readfirstlane(av[d]);
        if (act < 0) break;                        // padding: the sequence ends here, quietly
        if (act >= P.A) {                          // what a bad action is to a step: the ply is not played
            fl |= FL_ERR;
            st |= ST_CALLER;
            break;
        }
        int flags = 0, nn = 0, na = 0, elim = 0;
        // board.py:352-353 via the mask of the current board: the row taken in
        // the frame at ply 0, then the one the move before left (its move
        // ended on a wave barrier).  A clear bit is the step kernels' quick
        // exit: no move, the ply counted.
        if ((rdlane64(row, act >> 6) >> (act & 63)) & 1ULL) {
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
            int r1, c1, r2, c2;
            action_coords(P.R, P.C, act, r1, c1, r2, c2);
            const int p1 = r1 * P.C + c1, p2 = r2 * P.C + c2;
            // on a line-free board the bounded first line search applies
            if constexpr (RP) {
                if (rowp) elim = rp_move<SBNB, CODD>(P, w, lane, J, g, cl, p1, p2, flags);
                else elim = sb_move<SBNB, CODD>(P, w, lane, J, g, cl, p1, p2, flags, e);
            } else elim = board_move<MAXN, GEN, SBNB, CODD, TIER>(P, w, lane, J, g, cl, p1, p2, flags, nn, na, e, lists,
                                                                 clean);
            if constexpr (GEN) {
                if (flags & FL_OVF) {
                    // as rollout_env: the queue holds every virtual env of the
                    // launch and WsSerialBig cannot run out
                    if constexpr (TIER == TIER_MAIN) {
                        if (queue_env(P.spill, lane, v)) return st;
                    }
                    flags = (flags & ~FL_OVF) | FL_ERR;
                }
            }
            row = lane < W ? w.effw[lane] : 0ULL;
            clean = true;
        }
        if (a.ply_reward && lane == 0) a.ply_reward[v * D + d] = elim;
        tot += elim;
        tn += nn;
        ta += na;
        fl |= flags;
        np++;
        if (flags & FL_ERR) { st |= ST_INTERNAL; break; }   // a safety cap: the sequence stops here
    }
    // tile_match_env.py:100-101, 119-120: the sequence that reaches num_moves is done, its mask zero
    const bool done = a.timer && np > 0 && t0 + np >= P.num_moves;
    if (done) fl |= FL_DONE;
    playout_store(P, a, w, lane, v, tot, tn, ta, np, fl, t0 + np, row, done, g);
    return st;
}

// Occupancy: rollout's values, kept after one A/B at 4 096 envs.  Lean: 4 / 5 waves per SIMD
// measured 6.67 / 8.99 ms per c2 launch of 256 masked sequences of depth 4; general: 5 / 4 measured 21.5 / 21.7 ms
// at c3 (uniform sequences: 6.63 / 6.33 ms, the other way round; within 5 % everywhere).
#ifndef TMG_PLAY_LEAN_WAVES
#define TMG_PLAY_LEAN_WAVES TMG_ROLL_LEAN_WAVES
#endif
#ifndef TMG_PLAY_GEN_WAVES
#define TMG_PLAY_GEN_WAVES TMG_ROLL_GEN_WAVES
#endif
#ifndef TMG_PLAY_512_WAVES
#define TMG_PLAY_512_WAVES TMG_ROLL_512_WAVES
#endif
constexpr int kPlayLean128Waves = TMG_PLAY_LEAN_WAVES;   // playout_kernel<128, false>
constexpr int kPlayGen128Waves = TMG_PLAY_GEN_WAVES;     // playout_kernel<128, true>
constexpr int kPlay512Waves = TMG_PLAY_512_WAVES;        // playout_kernel<512, *>

// tmg_playout over a batch, one wave per virtual env: peek's instantiations
template <int MAXN, bool GEN, int SBNB = 0, bool CODD = false>
__global__ __launch_bounds__(64, MAXN == 128 ? (GEN ? kPlayGen128Waves : kPlayLean128Waves) : kPlay512Waves) void playout_kernel(
    Params P_, PlayArgs a) {
    TMG_SMEM_DECL(smem);
    using WS = Ws<MAXN, GEN>;
    const Params &P = TMG_KERNARG_PARAMS(P_);
    const int lane = threadIdx.x & 63;
    WS &w = *reinterpret_cast<WS *>(smem);
    const int64_t v = wg_env();
    if (v >= a.n * a.seqs) return;
    WsSerial<MAXN> *lists = nullptr;
    if constexpr (GEN) lists = &w.s;
    const uint32_t st = playout_env<MAXN, GEN, SBNB, CODD, TIER_MAIN, WS, WsSerial<MAXN>>(P, a, w, lane, v, lists);
    note_status(P, lane, st);
}

// every sequence of the virtual envs playout_kernel<*, true> queued (spill_drain)
template <int MAXN>
__global__ __launch_bounds__(64, 8) void playout_spill_kernel(Params P, PlayArgs a) {
    spill_drain<MAXN>(P, a.n * a.seqs, [&](Ws<MAXN, false> &w, int lane, int64_t v, WsSerialBig<MAXN> *lists) {
        return playout_env<MAXN, true, 0, false, TIER_SPILL, Ws<MAXN, false>, WsSerialBig<MAXN>>(P, a, w, lane, v, lists);
    });
}
