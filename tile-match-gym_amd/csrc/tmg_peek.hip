// tmg_peek.hip — tmg_peek: what a step with each action would report, for all
// A actions of an env at once, without changing the env.  Included by
// tmg_board.hip after step_env: the moves are the ones a step runs (rp_move /
// sb_move / board_move), each on a fresh copy of the board and of the env's
// RNG stream.
//
// One wave per env.  The board is read from HBM once, into LDS, and a pristine
// copy of it stays in registers (lane i: dwords i, i + 64, ... of the LDS
// board); every simulated action restores LDS from them.  The mask row is
// moved out of w.effw into a register per lane first, since every move leaves
// the final board's mask there.  The wave walks the mask one 64-bit word at a
// time, set bits ascending; lane j keeps the outcome of action 64 * w + j (zero
// unless simulated), so a word's outcomes leave with one coalesced store per
// output array.
#pragma once

// dwords of the LDS board a lane keeps: 64 cover <= 128 cells, 256 cover 512
template <int MAXN>
constexpr int peek_dwords() { return MAXN <= 128 ? 1 : 4; }

// one mask word's outcomes: lane j holds action base + j
__device__ __forceinline__ void peek_store_word(const Params &P, int lane, int64_t e, int base, int r, int nn, int na,
                                                int fl, int32_t *__restrict__ reward, int32_t *__restrict__ n_new,
                                                int32_t *__restrict__ n_act, uint8_t *__restrict__ flags_out) {
    const int a = base + lane;
    if (a < P.A) {
        const int64_t o = e * P.A + a;
        if (reward) reward[o] = r;
        if (n_new) n_new[o] = nn;
        if (n_act) n_act[o] = na;
        if (flags_out) flags_out[o] = (uint8_t)fl;
    }
}

// env e's RNG words (wave-uniform) and lane ll's jump-table row: the row of
// output bp_out(ll) for the row-plane cascade (rowp), as step_env loads them
__device__ __forceinline__ void peek_load(const Params &P, const uint64_t *__restrict__ rng, int64_t e, bool rowp,
                                          int ll, Rng &g, LaneJump &J) {
    const uint64_t *rp = rng + e * 5 + (ll >> 6);          // ll < 64: the lane index only keeps the loads per action
    const uint64_t q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3], q4 = rp[4];
    const JumpRow jrow = jump_row_load(P, ll, rowp);       // all nine loads before the first broadcast waits
    g.slo = bcast64(q0); g.shi = bcast64(q1); g.ilo = bcast64(q2); g.ihi = bcast64(q3); g.h = bcast64(q4);
    J = jump_row_finish(jrow, g);
}

// Board.move (board.py:330-395) of every action of env e, each on a copy.
// GEN / SBNB / CODD / TIER / WS / L as step_env; trust_eff as tmg_step.
// Returns the ST_* bits for the sticky status word.  TIER_MAIN with GEN: the
// first action whose cascade outgrows the LDS lists queues the env for
// peek_spill_kernel and abandons it (outputs written so far are rewritten
// there).
template <int MAXN, bool GEN, int SBNB, bool CODD, int TIER = TIER_MAIN, class WS = Ws<MAXN, GEN>,
          class L = WsSerial<MAXN>>
__device__ __forceinline__ uint32_t peek_env(
    const Params &P, WS &w, int lane, int64_t e, const int8_t *__restrict__ board, const uint64_t *__restrict__ rng,
    const uint64_t *__restrict__ eff, int trust_eff, int32_t *__restrict__ reward, int32_t *__restrict__ n_new,
    int32_t *__restrict__ n_act, uint8_t *__restrict__ flags_out, int32_t *__restrict__ best_action,
    int32_t *__restrict__ best_reward, L *lists) {
    constexpr int ND = peek_dwords<MAXN>();
    const int N = P.N, W = P.W;
    const int8_t *gb = board + e * 2 * N;
    // the mask row (trusted) and the board, loaded once per env
    uint64_t effrow = 0ULL;
    if (trust_eff && lane < W) effrow = eff[e * W + lane];
    constexpr bool RP = SBNB > 0 && !GEN;
    bool rowp = false;
    if constexpr (RP) rowp = rp_shape(P);
    load_board(P, w, lane, gb);                    // bytes when 2N is no multiple of 4 (boards then start on odd words)
    if constexpr (TIER == TIER_SPILL) COVER(CV_PEEK_SPILL_RUN);
    WSYNC();
    // the pristine copy: whole dwords of the LDS board (w.brd is dword-aligned
    // and 2 * MAXN long, so the last partial dword of an odd N lies inside it)
    const int nd = (2 * N + 3) >> 2;
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
            for (int wi = 0; wi < W; wi++) peek_store_word(P, lane, e, wi * 64, 0, 0, 0, FL_ERR, reward, n_new, n_act, flags_out);
            if (lane == 0) {
                if (best_action) best_action[e] = 0;
                if (best_reward) best_reward[e] = 0;
            }
            return ST_INTERNAL;
        }
    }
    if (!trust_eff) {                              // the mask of the board as it stands (it may hold a line)
        scan_effective(P, w, lane, make_cells<MAXN / 64>(P, lane), false);
        WSYNC();
        effrow = lane < W ? w.effw[lane] : 0ULL;
    }
    // The lean kernels load per action what a step loads (the RNG words, this
    // lane's jump-table row: cache hits after the first) and rebuild the cell
    // coordinates, through an opaque lane index so that none of it is hoisted:
    // kept live across the moves these ~30 registers cost them more in
    // scratch traffic (c2 4.45 -> 4.20 ms per 65 536 envs).  The general
    // kernels keep them: reloading measured slower there (c3 50.6 -> 54.4 ms).
    constexpr bool RELOAD = !GEN;
    Rng g0{};
    LaneJump J0{};
    Cells<MAXN / 64> cl0{};
    if constexpr (!RELOAD) {
        peek_load(P, rng, e, rowp, lane, g0, J0);
        cl0 = make_cells<MAXN / 64>(P, lane);
    }
    int best_r = 0, best_a = 0;
    uint32_t st = 0;
    for (int wi = 0; wi < W; wi++) {
        uint64_t m = rdlane64(effrow, wi);
        int kr = 0, kn = 0, ka = 0, kf = 0;        // lane j: the outcome of action 64 * wi + j
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const int a = wi * 64 + j;
            Rng g = g0;
            LaneJump J = J0;
            Cells<MAXN / 64> cl = cl0;
            if constexpr (RELOAD) {
                const int ll = loop_lane(lane);
                peek_load(P, rng, e, rowp, ll, g, J);
                cl = make_cells<MAXN / 64>(P, ll);
            }
            WSYNC();                               // the move before is done with the board
#pragma unroll
            for (int i = 0; i < ND; i++) {
                const int d = i * 64 + lane;
                if (d < nd) reinterpret_cast<uint32_t *>(w.brd)[d] = keep[i];
            }
            if constexpr (GEN) {
                for (int p = lane; p < N; p += 64) w.mark[p] = 0;
            }
            WSYNC();
            COVER(CV_PEEK_MOVE);
            int flags = 0, nn = 0, na = 0, elim;
            int r1, c1, r2, c2;
            action_coords(P.R, P.C, a, r1, c1, r2, c2);
            const int p1 = r1 * P.C + c1, p2 = r2 * P.C + c2;
            if constexpr (RP) {
                if (rowp) elim = rp_move<SBNB, CODD>(P, w, lane, J, g, cl, p1, p2, flags);
                else elim = sb_move<SBNB, CODD>(P, w, lane, J, g, cl, p1, p2, flags, e);
            } else elim = board_move<MAXN, GEN, SBNB, CODD, TIER>(P, w, lane, J, g, cl, p1, p2, flags, nn, na, e, lists,
                                                                 trust_eff != 0);
            if constexpr (GEN) {
                if (flags & FL_OVF) {
                    // as step_env: the queue holds every env of the launch and
                    // WsSerialBig cannot run out, so the fall-through is
                    // unreachable; were it reached, the action is an error
                    if constexpr (TIER == TIER_MAIN) {
                        if (queue_env(P.spill, lane, e)) { COVER(CV_PEEK_SPILL); return st; }
                    }
                    flags = (flags & ~FL_OVF) | FL_ERR;
                }
            }
            if (flags & FL_ERR) st |= ST_INTERNAL;
            if (lane == j) { kr = elim; kn = nn; ka = na; kf = flags; }
            if (elim > best_r) { best_r = elim; best_a = a; }       // ascending a: the lowest of maximal reward
        }
        peek_store_word(P, lane, e, wi * 64, kr, kn, ka, kf, reward, n_new, n_act, flags_out);
    }
    if (lane == 0) {
        if (best_action) best_action[e] = best_a;
        if (best_reward) best_reward[e] = best_r;
    }
    return st;
}

// tmg_peek over a batch, one wave per env: the generic instantiations only
template <int MAXN, bool GEN, int SBNB = 0, bool CODD = false>
__global__ __launch_bounds__(64, MAXN == 128 ? (GEN ? kPeekGen128Waves : kPeekLean128Waves) : kPeek512Waves) void peek_kernel(
    Params P_, int64_t n, const int8_t *__restrict__ board, const uint64_t *__restrict__ rng,
    const uint64_t *__restrict__ eff, int trust_eff, int32_t *__restrict__ reward, int32_t *__restrict__ n_new,
    int32_t *__restrict__ n_act, uint8_t *__restrict__ flags_out, int32_t *__restrict__ best_action,
    int32_t *__restrict__ best_reward) {
    TMG_SMEM_DECL(smem);
    using WS = Ws<MAXN, GEN>;
    const Params &P = TMG_KERNARG_PARAMS(P_);
    const int lane = threadIdx.x & 63;
    WS &w = *reinterpret_cast<WS *>(smem);
    const int64_t e = wg_env();
    if (e >= n) return;
    WsSerial<MAXN> *lists = nullptr;
    if constexpr (GEN) lists = &w.s;
    const uint32_t st = peek_env<MAXN, GEN, SBNB, CODD, TIER_MAIN, WS, WsSerial<MAXN>>(
        P, w, lane, e, board, rng, eff, trust_eff, reward, n_new, n_act, flags_out, best_action, best_reward, lists);
    note_status(P, lane, st);
}

// every action of the envs peek_kernel<*, true> queued, and all of those envs' outputs (spill_drain)
template <int MAXN>
__global__ __launch_bounds__(64, 8) void peek_spill_kernel(
    Params P, int64_t n, const int8_t *__restrict__ board, const uint64_t *__restrict__ rng,
    const uint64_t *__restrict__ eff, int trust_eff, int32_t *__restrict__ reward, int32_t *__restrict__ n_new,
    int32_t *__restrict__ n_act, uint8_t *__restrict__ flags_out, int32_t *__restrict__ best_action,
    int32_t *__restrict__ best_reward) {
    spill_drain<MAXN>(P, n, [&](Ws<MAXN, false> &w, int lane, int64_t e, WsSerialBig<MAXN> *lists) {
        return peek_env<MAXN, true, 0, false, TIER_SPILL, Ws<MAXN, false>, WsSerialBig<MAXN>>(
            P, w, lane, e, board, rng, eff, trust_eff, reward, n_new, n_act, flags_out, best_action, best_reward, lists);
    });
}
