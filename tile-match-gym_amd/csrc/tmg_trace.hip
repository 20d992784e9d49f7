// tmg_trace.hip — tmg_trace: one move's cascade stage by stage, on a copy of
// the env.  Row (q, i) is Board.move(actions[q][i]) (board.py:330-395) on a
// copy of board[i] with a copy of rng[i]; between the stages of the move the
// board is written out of LDS into the row's next frame slot.  Included by
// tmg_board.hip after tmg_playout.hip, whose frame this file keeps: one wave
// per virtual env v = q * n + i (board / mask / RNG row i, action and output
// row v), the board loaded into LDS once.
//
// trace_move is board_move's unfused branch with a frame hook after every
// stage: detect, then fast_clear on a board that can hold no special, else the
// lane-0 list machinery (Serial::build_lines / process_lines / resolve), then
// gravity, refill and, after the cascade, ensure_playable.  The fused forms
// (sb_simple_step, simple_step_lds, rp_move, sb_move) never hold the board
// between two stages and are not used, so the general non-bitboard kernels are
// the only instantiations.
#pragma once

enum : int { TR_SWAP = 1, TR_COMBO = 2, TR_CLEAR = 3, TR_FALL = 4, TR_REFILL = 5, TR_SHUFFLE = 6 };
enum : int { FL_STOPPED = 0x10 };                // tmg_trace only
enum : int { TRACE_DONE = 0, TRACE_STOPPED = 1, TRACE_QUEUED = 2 };

// The call's arguments (by value to the kernels, after Params).
struct TraceArgs {
    int64_t n;                    // real envs; the launch covers n * seqs virtual envs
    int seqs;
    const int8_t *board;          // [n]
    const uint64_t *rng;          // [n][5]
    const uint64_t *eff;          // [n][W] (trust_eff != 0)
    int trust_eff;
    const int32_t *actions;       // [seqs][n]
    uint32_t stage_mask;          // bit TR_*: the stage is recorded
    int max_frames, stop;
    int8_t *frames;               // [seqs][n][max_frames][2][R][C] or null
    uint8_t *kind;                // [seqs][n][max_frames] or null
    int32_t *frame_elim;          // [seqs][n][max_frames] or null
    int32_t *n_frames, *reward, *n_new, *n_act;   // [seqs][n], each or null
    uint8_t *flags;               // [seqs][n] or null
    uint64_t *out_rng;            // [seqs][n][5] or null
};

// Virtual env v's sums and flags, once, from lane 0; kind / frame_elim from the
// first unrecorded slot on zeroed; the RNG words as the simulated stages left
// them.
__device__ __forceinline__ void trace_store(const TraceArgs &a, int lane, int64_t v, int nf, int rew, int tn, int ta,
                                            int fl, const Rng &g) {
    if (lane == 0) {
        if (a.n_frames) a.n_frames[v] = nf;
        if (a.reward) a.reward[v] = rew;
        if (a.n_new) a.n_new[v] = tn;
        if (a.n_act) a.n_act[v] = ta;
        if (a.flags) a.flags[v] = (uint8_t)fl;
    }
    const int64_t base = v * a.max_frames;
    for (int f = min(nf, a.max_frames) + lane; f < a.max_frames; f += 64) {
        if (a.kind) a.kind[base + f] = 0;
        if (a.frame_elim) a.frame_elim[base + f] = 0;
    }
    if (a.out_rng) store_rng(a.out_rng + v * 5, g, lane);
}

// The stage `kind` has just run on the LDS board: record it when selected
// (slot nf, while one is left) and count it.  True when the row stops here.
template <class WS>
__device__ __forceinline__ bool trace_frame(const Params &P, const TraceArgs &a, const WS &w, int lane, int64_t v,
                                            int kind, int elim, int &nf) {
    if (!((a.stage_mask >> kind) & 1u)) return false;
    if (nf < a.max_frames) {
        const int64_t slot = v * a.max_frames + nf;
        WSYNC();                                   // the stage's LDS writes, lane 0's included
        if (a.frames) store_board(P, w, lane, a.frames + slot * 2 * P.N);
        if (lane == 0) {
            if (a.kind) a.kind[slot] = (uint8_t)kind;
            if (a.frame_elim) a.frame_elim[slot] = elim;
        }
        WSYNC();                                   // read before the next stage writes the board
    }
    nf++;
    return a.stop != 0 && nf >= a.max_frames;
}

// Board.move of the swap p1 <-> p2 on the LDS board, stage by stage; tot: the
// eliminations of the stages run (without the new specials), flags: FL_COMBO /
// FL_SHUF / FL_OVF / FL_ERR as board_move sets them.  clean as board_move's.
template <int MAXN, int TIER, class WS, class L>
__device__ __forceinline__ int trace_move(const Params &P, const TraceArgs &a, WS &w, int lane, int64_t v,
                                          const LaneJump &J, Rng &g, const Cells<MAXN / 64> &cl, int p1, int p2,
                                          bool clean, L *lists, int &nf, int &tot, int &flags) {
    const auto cells = [&]() {                     // board_move's: rebuilt at <= 128 cells, kept at 512
        if constexpr (MAXN > 128) return cl;
        else return make_cells<MAXN / 64>(P, loop_lane(lane));
    };
    const int N = P.N;
    int lim = P.R - 1;
    if (clean) lim = min(P.R - 1, div_c(P, max(p1, p2)) + 2);
    int8_t *col = w.brd, *typ = w.brd + N;
    if (lane == 0) {                                                        // swap_coords :355
        int8_t x = col[p1]; col[p1] = col[p2]; col[p2] = x;
        x = typ[p1]; typ[p1] = typ[p2]; typ[p2] = x;
        w.sc[SC_NACT] = 0; w.sc[SC_NNEW] = 0; w.sc[SC_ERR] = 0; w.sc[SC_A] = 0;
    }
    WSYNC();
    if (trace_frame(P, a, w, lane, v, TR_SWAP, 0, nf)) return TRACE_STOPPED;
    // gravity and refill, a frame after each
    const auto fall_refill = [&]() -> bool {
        WSYNC();
        gravity(P, w, lane);
        WSYNC();
        if (trace_frame(P, a, w, lane, v, TR_FALL, 0, nf)) return true;
        refill(P, w, lane, J, g);
        return trace_frame(P, a, w, lane, v, TR_REFILL, 0, nf);
    };
    const int t1 = typ[p1], t2 = typ[p2];
    bool ovf = false;
    if (((t1 != 0 && t1 != 1) && (t2 != 0 && t2 != 1)) || t1 < 0 || t2 < 0) {   // :357-364
        flags |= FL_COMBO;
        COVER(CV_COMBO);
        const int nz = count_colour_nonzero(P, w, lane);
        if (lane == 0) {
            w.sc[SC_NZ] = nz;
            Serial<MAXN, L> S(P, w, *lists);
            S.combination(p1, p2);
            w.sc[SC_A] = S.ovf;
        }
        WSYNC();
        ovf = w.sc[SC_A] != 0;
        if (!ovf) {
            const int z = count_type_zero(P, w, lane);
            tot += z;
            if (trace_frame(P, a, w, lane, v, TR_COMBO, z, nf)) return TRACE_STOPPED;
            if (fall_refill()) return TRACE_STOPPED;
        }
        lim = P.R - 1;
    }
    // wave-parallel clear only when no special can exist on the board
    bool fast = false;
    if (P.smask == 0) {
        bool ok = true;
        for (int p = lane; p < N; p += 64) ok &= typ[p] == 1;
        fast = __ballot(!ok) == 0ULL;
    }
    while (!ovf) {                                                          // :367-376
        if (w.sc[SC_ERR]) break;
        Det<MAXN / 64> d;
        const int rs = detect(P, w, lane, cells(), d, lim);
        if (rs < 0) break;
        int z;
        if (fast) {
            COVER(CV_FAST);
            z = fast_clear(P, w, lane, cells(), d, rs);
            lim = min(P.R - 1, rs + 2);
        } else {
            lim = P.R - 1;
            const int nz = count_colour_nonzero(P, w, lane);
            COVER(CV_SERIAL_STEP);
            if (lane == 0) {
                w.sc[SC_NZ] = nz;
                Serial<MAXN, L> S(P, w, *lists);
                S.build_lines(rs);
                if (!S.ovf) S.process_lines();
                if (!S.ovf) S.resolve();
                w.sc[SC_A] = S.ovf;
            }
            WSYNC();
            ovf = w.sc[SC_A] != 0;
            if (ovf) break;
            z = count_type_zero(P, w, lane);
        }
        tot += z;
        if (trace_frame(P, a, w, lane, v, TR_CLEAR, z, nf)) return TRACE_STOPPED;
        if (fall_refill()) return TRACE_STOPPED;
    }
    if (ovf) {
        // the lists ran out: the row is re-run whole on the worst-case lists
        // (the queue holds every virtual env of the launch and WsSerialBig
        // cannot run out, so past TIER_MAIN this is unreachable: an error)
        if constexpr (TIER == TIER_MAIN) {
            if (queue_env(P.spill, lane, v)) return TRACE_QUEUED;
        }
        flags |= FL_ERR;
        return TRACE_DONE;
    }
    if (w.sc[SC_ERR]) flags |= FL_ERR;
    const int fl = ensure_playable(P, w, lane, J, g, cells(), !w.sc[SC_ERR]);   // :381-391
    flags |= fl;
    if (fl & FL_SHUF) {
        if (trace_frame(P, a, w, lane, v, TR_SHUFFLE, 0, nf)) return TRACE_STOPPED;
    }
    return TRACE_DONE;
}

// The traced move of virtual env v; returns the ST_* bits for the sticky status
// word.  TIER_MAIN: a row whose cascade outgrows the LDS lists is queued for
// trace_spill_kernel and abandoned (the frames written so far are rewritten
// there, as every other output is).
template <int MAXN, int TIER = TIER_MAIN, class WS = Ws<MAXN, true>, class L = WsSerial<MAXN>>
__device__ __forceinline__ uint32_t trace_env(const Params &P, const TraceArgs &a, WS &w, int lane, int64_t v,
                                              L *lists) {
    const int N = P.N;
    const int q = (int)(v / a.n);
    const int64_t e = v - (int64_t)q * a.n;
    const int act = __builtin_amdgcn_readfirstlane(a.actions[v]);
    Rng g = load_rng(a.rng + e * 5);
    if (act < 0) {                                 // padding: nothing happens, quietly
        trace_store(a, lane, v, 0, 0, 0, 0, 0, g);
        return 0;
    }
    if (act >= P.A) {                              // what a bad action is to a step
        trace_store(a, lane, v, 0, 0, 0, 0, FL_ERR, g);
        return ST_CALLER;
    }
    // board.py:352-353 through the mask: the caller's row, or the scan of the
    // board as it stands (it may hold a line).  A clear bit is the quick exit.
    if (a.trust_eff) {
        const uint64_t word = bcast64(a.eff[e * P.W + (act >> 6)]);
        if (!((word >> (act & 63)) & 1ULL)) {
            trace_store(a, lane, v, 0, 0, 0, 0, 0, g);
            return 0;
        }
    }
    load_board(P, w, lane, a.board + e * 2 * N);
    if constexpr (TIER == TIER_SPILL) COVER(CV_PEEK_SPILL_RUN);
    WSYNC();
    if (!a.trust_eff) {
        scan_effective(P, w, lane, make_cells<MAXN / 64>(P, lane), false);
        WSYNC();
        const uint64_t word = bcast64(w.effw[act >> 6]);
        if (!((word >> (act & 63)) & 1ULL)) {
            trace_store(a, lane, v, 0, 0, 0, 0, 0, g);
            return 0;
        }
    }
    const LaneJump J = load_jump(P, lane, g);
    const Cells<MAXN / 64> cl = make_cells<MAXN / 64>(P, lane);
    for (int p = lane; p < N; p += 64) w.mark[p] = 0;
    WSYNC();
    int r1, c1, r2, c2;
    action_coords(P.R, P.C, act, r1, c1, r2, c2);
    const int p1 = r1 * P.C + c1, p2 = r2 * P.C + c2;
    int nf = 0, tot = 0, flags = 0;
    const int end = trace_move<MAXN, TIER>(P, a, w, lane, v, J, g, cl, p1, p2, a.trust_eff != 0, lists, nf, tot, flags);
    if (end == TRACE_QUEUED) return 0;
    if (end == TRACE_STOPPED) flags |= FL_STOPPED;
    WSYNC();
    const int nn = w.sc[SC_NNEW], na = w.sc[SC_NACT];
    trace_store(a, lane, v, nf, tot + nn, nn, na, flags, g);                // :378
    return (flags & FL_ERR) ? ST_INTERNAL : 0;
}

// Occupancy, from -Rpass-analysis=kernel-resource-usage (DESIGN.md 3.12's
// register table): the most waves per SIMD at which the kernel needs no
// scratch.  128 cells: 5 waves hold it to 96 VGPRs and 124 B of scratch per
// lane, 4 give 121 VGPRs and none; 512 cells: 4 / 3 waves spill 260 / 104 B,
// 2 give 207 VGPRs and none.
#ifndef TMG_TRACE_128_WAVES
#define TMG_TRACE_128_WAVES 4
#endif
#ifndef TMG_TRACE_512_WAVES
#define TMG_TRACE_512_WAVES 2
#endif
constexpr int kTrace128Waves = TMG_TRACE_128_WAVES;   // trace_kernel<128>
constexpr int kTrace512Waves = TMG_TRACE_512_WAVES;   // trace_kernel<512>

// tmg_trace over a batch, one wave per virtual env: the general non-bitboard kernels
template <int MAXN>
__global__ __launch_bounds__(64, MAXN == 128 ? kTrace128Waves : kTrace512Waves) void trace_kernel(Params P_, TraceArgs a) {
    TMG_SMEM_DECL(smem);
    using WS = Ws<MAXN, true>;
    const Params &P = TMG_KERNARG_PARAMS(P_);
    const int lane = threadIdx.x & 63;
    WS &w = *reinterpret_cast<WS *>(smem);
    const int64_t v = wg_env();
    if (v >= a.n * a.seqs) return;
    const uint32_t st = trace_env<MAXN, TIER_MAIN, WS, WsSerial<MAXN>>(P, a, w, lane, v, &w.s);
    note_status(P, lane, st);
}

// the rows trace_kernel queued, re-run whole (spill_drain)
template <int MAXN>
__global__ __launch_bounds__(64, 8) void trace_spill_kernel(Params P, TraceArgs a) {
    spill_drain<MAXN>(P, a.n * a.seqs, [&](Ws<MAXN, false> &w, int lane, int64_t v, WsSerialBig<MAXN> *lists) {
        return trace_env<MAXN, TIER_SPILL, Ws<MAXN, false>, WsSerialBig<MAXN>>(P, a, w, lane, v, lists);
    });
}
