// tmg_rp.hip — the lean cascade on row bit-planes in registers: the move of a
// board that can hold no special (step_env's lean variant) when R <= 16 and
// C <= kRowScanMaxC.  Included by tmg_board.hip after tmg_sb.hip.
//
// Lane r < R holds row r as NB 32-bit words (RowPlanes, as bp_generate: bit c
// of plane b = bit b of colour - 1 of cell (r, c)) from the load to the
// write-back.  Line detection, the clear set, its perpendicular pass, gravity
// and the refill all run on those words: within a row as shifts of the word,
// across rows as DPP row shifts (R <= 16: one DPP row of 16 lanes), so a
// cascade iteration touches no LDS and the scalar unit only for its ballots
// and the stream position.  The scalar-bitboard path (tmg_sb.hip) keeps every
// other shape, the general kernels and the rare shuffle.
//
// TMG_RP: A/B switch (0: every lean move takes the scalar-bitboard path).
#ifndef TMG_RP
#define TMG_RP 1
#endif
constexpr int kRpMaxR = 16;
__device__ __forceinline__ bool rp_shape(const Params &P) {
    return TMG_RP != 0 && P.R <= kRpMaxR && P.C <= kRowScanMaxC;
}

// DPP row shifts inside one 16-lane row: rp_dn gives lane l the value of lane
// l - N (the row above, N rows up), rp_up the value of lane l + N; a lane whose
// source is outside the DPP row takes `old`.
template <int N>
__device__ __forceinline__ uint32_t rp_dn(uint32_t v, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x110 + N, 0xf, 0xf, false);   // row_shr:N
}
template <int N>
__device__ __forceinline__ uint32_t rp_up(uint32_t v, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x100 + N, 0xf, 0xf, false);   // row_shl:N
}
// OR / AND over the lanes at and after this one in the DPP row (rows at and
// below this one); inclusive sum over the lanes at and before it
__device__ __forceinline__ uint32_t rp_or_below(uint32_t v) {
    v |= rp_up<1>(v, 0u);
    v |= rp_up<2>(v, 0u);
    v |= rp_up<4>(v, 0u);
    v |= rp_up<8>(v, 0u);
    return v;
}
__device__ __forceinline__ uint32_t rp_and_below(uint32_t v) {
    v &= rp_up<1>(v, ~0u);
    v &= rp_up<2>(v, ~0u);
    v &= rp_up<4>(v, ~0u);
    v &= rp_up<8>(v, ~0u);
    return v;
}
__device__ __forceinline__ uint32_t rp_sum_above(uint32_t v) {
    v += rp_dn<1>(v, 0u);
    v += rp_dn<2>(v, 0u);
    v += rp_dn<4>(v, 0u);
    v += rp_dn<8>(v, 0u);
    return v;
}

// row `lane` of the LDS colour plane as planes of colour - 1 (one conversion
// per step).  Bit 7 of every byte set before the subtraction: no borrow
// crosses a byte whatever the byte holds.
template <int NB, class WS>
__device__ __forceinline__ RowPlanes<NB> rp_load(const Params &P, const WS &w, int lane, uint32_t cm) {
    const int rr = lane < P.R ? lane : 0;
    const int nd = (P.C + 3) >> 2;
    uint32_t d[8];
    lds_row(w, rr * P.C, nd, d);
    RowPlanes<NB> pl;
#pragma unroll
    for (int b = 0; b < NB; b++) pl.p[b] = 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j < nd) {
            const uint32_t x = (d[j] | 0x80808080u) - 0x01010101u;
#pragma unroll
            for (int b = 0; b < NB; b++) pl.p[b] |= byte_bits(x, b) << (4 * j);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; b++) pl.p[b] &= cm;
    return pl;
}

// scan_rows (the effective-action mask into w.effw, possible_move) from the
// planes in registers: the scan works on planes of the colour itself (0 =
// outside the board), i.e. the planes of colour - 1 incremented
template <int NB, int NBV, class WS>
__device__ __forceinline__ int rp_scan_nb(const Params &P, WS &w, int lane, const RowPlanes<NB> &pl, uint32_t cm) {
    uint32_t X[NBV];
    uint32_t carry = cm;
#pragma unroll
    for (int b = 0; b < NBV; b++) {
        const uint32_t x = b < NB ? pl.p[b < NB ? b : 0] : 0u;
        X[b] = x ^ carry;
        carry &= x;
    }
    return scan_rows_core<false, NBV>(P, w, lane, lane, true, X, cm, 0u, 0u, 0u, false);
}
// SCAN2: where the colour value needs a plane more than colour - 1 (k = 2, 4,
// 8: NB = sb_planes(k)), the scan runs on the NB planes as they are, the board's
// edge ORed into its D masks (scan_rows_core's EDGE)
template <int NB, bool SCAN2, class WS>
__device__ __forceinline__ int rp_scan(const Params &P, WS &w, int lane, const RowPlanes<NB> &pl, uint32_t cm) {
    constexpr int NB1 = NB < 4 ? NB + 1 : 4;
    if (rs_planes(P.k) == NB) return rp_scan_nb<NB, NB>(P, w, lane, pl, cm);
    if constexpr (SCAN2) {
        COVER(CV_RP_SCAN2);
        return scan_rows_core<false, NB, true>(P, w, lane, lane, true, pl.p, cm, 0u, 0u, 0u, false);
    }
    return rp_scan_nb<NB, NB1>(P, w, lane, pl, cm);
}

// bits [s, s + 28) of the 128-bit string hi:lo (wave-uniform), per lane
__device__ __forceinline__ uint32_t rp_slice(uint64_t lo, uint64_t hi, int s, bool wide) {
    const int sh = s & 63;
    if (!wide) return (uint32_t)(lo >> sh);
    const uint64_t w0 = s < 64 ? lo : hi, w1 = s < 64 ? hi : 0ULL;
    return (uint32_t)(w0 >> sh) | (sh > 32 ? (uint32_t)(w1 << (64 - sh)) : 0u);
}

// TMG_RP_BATCH: A/B switch (0: a jump-ahead batch per cascade iteration, rp_refill;
// 1: one per move, carried through the iterations, RpBatch)
#ifndef TMG_RP_BATCH
#define TMG_RP_BATCH 1
#endif

// TMG_RP_VSHIFT: A/B switch (0: gravity moves every column one row per pass;
// 1: the columns of the first line's vertical runs move three rows in the
// first pass, rp_move)
#ifndef TMG_RP_VSHIFT
#define TMG_RP_VSHIFT 1
#endif
// TMG_RP_SCAN2: A/B switch (0: the final effective-mask scan on planes of the
// colour value, rp_scan_nb; 1: on the cascade's own planes of colour - 1 where
// those are one fewer, rp_scan)
#ifndef TMG_RP_SCAN2
#define TMG_RP_SCAN2 1
#endif
// The two levers are arguments of rp_move (LV), handed over by the lean step
// (step_env) alone: tmg_peek, tmg_rollout and tmg_playout call rp_move without
// them and keep their object code.
// RP_NOLDS (TMG_BP_ROUND, tmg_board.hip): the caller may say that the final
// board is not needed in LDS (an inline regeneration rewrites all of it).
enum : int { RP_VSHIFT = 1, RP_SCAN2 = 2, RP_NOLDS = 4 };
constexpr int kRpLevers = (TMG_RP_VSHIFT ? RP_VSHIFT : 0) | (TMG_RP_SCAN2 ? RP_SCAN2 : 0) | (TMG_BPR_NOLDS ? RP_NOLDS : 0);

// Lemire rejection among the T colours of a refill: exact serial replay, cell
// by cell, from the exact stream position g
template <int NB, class WS>
__device__ __forceinline__ void rp_replay(const Params &P, WS &w, int lane, Rng &g, uint32_t G, int pre, int T,
                                          RowPlanes<NB> &pl) {
    COVER(CV_REJECT);
    COVER(CV_RP_REJECT);
    WFENCE();
    if (lane == 0) {
        Rng r = g;
        for (int i = 0; i < T; i++) w.u.draw[i] = (uint32_t)r_colour(P, r);
        g = r;
    }
    rng_bcast(g);
    WSYNC();
    int at = pre;
    for (uint32_t f = G; f; f &= f - 1u) {
        const int c = __builtin_ctz(f);
        const uint32_t code = w.u.draw[at++] - 1u;
#pragma unroll
        for (int b = 0; b < NB; b++) pl.p[b] |= ((code >> b) & 1u) << c;
    }
    WSYNC();
}

// this lane's slice sl (its colours from bit 0 up, one word per plane) into
// its refill bits G, one run of contiguous cells at a time
template <int NB>
__device__ __forceinline__ void rp_deposit(uint32_t G, uint32_t (&sl)[NB], RowPlanes<NB> &pl) {
    for (uint32_t f = G; f;) {
        const int c = __builtin_ctz(f);
        const int len = __builtin_ctz(~(f >> c));        // f < 2^28: a zero bit above every run
        const uint32_t m = (1u << len) - 1u;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            pl.p[b] |= (sl[b] & m) << c;
            sl[b] >>= len;
        }
        f &= ~(m << c);
    }
}

#if !TMG_RP_BATCH
// The refill (board.py:233-241) of the cells G of this lane's row, T cells in
// all, `pre` of them in the rows above: the next T colours of the env's
// stream in row-major order.  One jump-ahead batch of 64 PCG64 outputs in
// bp_ring_fill's lane order (J holds the jump-table row of output bp_out(lane)),
// turned into one bit-string per plane by ballots; each lane takes its slice
// and deposits it at its refill bits, one run of contiguous cells at a time.
template <int NB, class WS>
__device__ __forceinline__ void rp_refill(const Params &P, WS &w, int lane, const LaneJump &J, Rng &g, uint32_t G, int pre,
                                          int T, RowPlanes<NB> &pl) {
    const uint32_t k = (uint32_t)P.k;
#pragma unroll
    for (int b = 0; b < NB; b++) pl.p[b] &= ~G;
    if (k == 1) return;                                  // rng == 0: numpy draws nothing, every colour is 1
    const int off = (int)(g.h >> 32) & 1;                // draw 0 is the buffered half-word
    const uint64_t mbuf = (uint64_t)(uint32_t)g.h * k;
    const int need = T - off;
    const int n64 = (need + 1) >> 1;
    cover_uniform(P, lane, U128{g.slo, g.shi});
    const U128 sj = jump128(J.Aj, U128{g.slo, g.shi}, J.incG);
    const uint64_t out = xsl_rr(sj);
    const int o = bp_out(lane);
    const uint64_t m0 = (uint64_t)(uint32_t)out * k, m1 = (out >> 32) * k;
    if (P.thr != 0u) {
        const bool rbuf = off && (uint32_t)mbuf < P.thr;
        const bool rej = (o < n64 && (uint32_t)m0 < P.thr) || (2 * o + 1 < need && (uint32_t)m1 < P.thr);
        if (__ballot(rej) != 0ULL || rbuf) {
            rp_replay<NB>(P, w, lane, g, G, pre, T, pl);
            return;
        }
    }
    // codes of colours l and 64 + l of the batch on lane l (bp_ring_fill)
    const uint32_t c0 = (uint32_t)(m0 >> 32), c1 = (uint32_t)(m1 >> 32);
    const uint32_t n0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c0, 0xb1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    const uint32_t n1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c1, 0xb1, 0xf, 0xf, true);
    const bool odd = lane & 1;
    const uint32_t x0 = odd ? n1 : c0, x1 = odd ? c1 : n0;
    const bool wide = T > 64;                            // wave-uniform
    if (wide) COVER(CV_RP_WIDE);
    const uint32_t bcode = (uint32_t)(mbuf >> 32);
    uint32_t sl[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        uint64_t lo = __ballot((x0 >> b) & 1u), hi = 0ULL;
        if (wide) hi = __ballot((x1 >> b) & 1u);
        if (off) {                                       // the buffered half-word goes first
            hi = (hi << 1) | (lo >> 63);
            lo = (lo << 1) | ((bcode >> b) & 1u);
        }
        sl[b] = rp_slice(lo, hi, pre, wide);
    }
    rp_deposit<NB>(G, sl, pl);
    if (n64 > 0) {                                       // the stream position after the last output taken
        const int l = bp_lane(n64 - 1);
        g.slo = rdlane64(sj.lo, l);
        g.shi = rdlane64(sj.hi, l);
        g.h = ((uint64_t)(need & 1) << 32) | (uint32_t)rdlane64(out >> 32, l);
    } else {
        g.h = (uint32_t)g.h;                             // only the buffered half was used
    }
}
#else
// One jump-ahead batch of 64 PCG64 outputs per move, in bp_ring_fill's lane
// order: the next 128 colours of the env's stream (the buffered half-word
// first, when there is one) as one wave-uniform 128-bit string per plane, bit
// i = the i-th colour not yet taken.  Every cascade iteration takes its T
// colours from bit 0 and shifts the strings down by T on the scalar unit
// (Lemire rejections: the index of the first rejected word is kept beside
// them, and an iteration that reaches it replays serially, rp_replay); the
// env's stream position is derived from the count taken, once, when something
// else needs it (rp_sync).
template <int NB>
struct RpBatch {
    U128 sj;                     // per lane: the state after output bp_out(lane) of the batch
    uint64_t lo[NB], hi[NB];     // wave-uniform: the planes of the colours not yet taken
    int rfirst;                  // P.thr != 0: the batch's first Lemire-rejected word, as a colour index (else >= 128)
    int left;                    // colours not yet taken (0: no batch)
    int used;                    // colours taken, the buffered half-word included
    int off;                     // the batch began with the buffered half-word
};

// the strings shifted down by the T colours taken, 1 <= T <= 128 (wave-uniform;
// an iteration clears a line, so T >= 3).  One scalar branch on the common
// T < 64 instead of selects per string: four shifts each.
template <int NB>
__device__ __forceinline__ void rp_advance(RpBatch<NB> &B, int T) {
    if (T < 64) {
#pragma unroll
        for (int b = 0; b < NB; b++) {
            B.lo[b] = (B.lo[b] >> T) | (B.hi[b] << (64 - T));
            B.hi[b] >>= T;
        }
    } else {
#pragma unroll
        for (int b = 0; b < NB; b++) {
            B.lo[b] = T < 128 ? B.hi[b] >> (T - 64) : 0ULL;
            B.hi[b] = 0ULL;
        }
    }
    B.left -= T;
    B.used += T;
}

// a fresh batch from the stream as it stands at g (exact); J: the jump-table
// row of output bp_out(lane)
template <int NB>
__device__ __forceinline__ void rp_batch(const Params &P, int lane, const LaneJump &J, const Rng &g, RpBatch<NB> &B) {
    const uint32_t k = (uint32_t)P.k;
    const int off = (int)(g.h >> 32) & 1;                // colour 0 is the buffered half-word
    const uint64_t mbuf = (uint64_t)(uint32_t)g.h * k;
    cover_uniform(P, lane, U128{g.slo, g.shi});
    B.sj = jump128(J.Aj, U128{g.slo, g.shi}, J.incG);
    const uint64_t out = xsl_rr(B.sj);
    const uint64_t m0 = (uint64_t)(uint32_t)out * k, m1 = (out >> 32) * k;
    // codes of colours l and 64 + l of the batch on lane l (bp_ring_fill); a
    // rejected word is flagged in bit 31 of its code and travels with it
    uint32_t c0 = (uint32_t)(m0 >> 32), c1 = (uint32_t)(m1 >> 32);
    if (P.thr != 0u) {
        c0 |= (uint32_t)m0 < P.thr ? 0x80000000u : 0u;
        c1 |= (uint32_t)m1 < P.thr ? 0x80000000u : 0u;
    }
    const uint32_t n0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c0, 0xb1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    const uint32_t n1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c1, 0xb1, 0xf, 0xf, true);
    const bool odd = lane & 1;
    const uint32_t x0 = odd ? n1 : c0, x1 = odd ? c1 : n0;
    const uint32_t bcode = (uint32_t)(mbuf >> 32);
#pragma unroll
    for (int b = 0; b < NB; b++) {
        uint64_t lo = __ballot((x0 >> b) & 1u), hi = __ballot((x1 >> b) & 1u);
        if (off) {                                       // the buffered half-word goes first
            hi = (hi << 1) | (lo >> 63);
            lo = (lo << 1) | ((bcode >> b) & 1u);
        }
        B.lo[b] = lo;
        B.hi[b] = hi;
    }
    B.rfirst = 2 * 128;
    if (P.thr != 0u) {
        // only the first rejected word matters: the replay that meets it drops the batch
        const uint64_t lo = __ballot((x0 >> 31) != 0u), hi = __ballot((x1 >> 31) != 0u);
        if (lo | hi) B.rfirst = off + (lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(hi));
        if (off && (uint32_t)mbuf < P.thr) B.rfirst = 0;
    }
    B.left = 128;
    B.used = 0;
    B.off = off;
}

// g <- the exact stream position after the colours taken from the batch
// (rp_refill's / bp_ring_state's arithmetic: the state after the last output
// touched, its high half buffered when an odd number of half-words was
// taken); the batch is dropped
template <int NB>
__device__ __forceinline__ void rp_sync(RpBatch<NB> &B, Rng &g) {
    if (B.used > 0) {
        const int need = B.used - B.off;                 // half-words taken from the batch's outputs
        if (need > 0) {
            const int l = bp_lane(((need + 1) >> 1) - 1);
            const U128 s{rdlane64(B.sj.lo, l), rdlane64(B.sj.hi, l)};
            g.slo = s.lo;
            g.shi = s.hi;
            g.h = ((uint64_t)(need & 1) << 32) | (uint32_t)(xsl_rr(s) >> 32);
        } else {
            g.h = (uint32_t)g.h;                         // only the buffered half was used
        }
    }
    B.left = 0;
    B.used = 0;
}

// The refill (board.py:233-241) of the cells G of this lane's row, T cells in
// all, `pre` of them in the rows above: the next T colours of the env's
// stream in row-major order, from the move's batch.  Each lane takes its
// slice of the strings and deposits it at its refill bits.
template <int NB, class WS>
__device__ __forceinline__ void rp_take(const Params &P, WS &w, int lane, RpBatch<NB> &B, Rng &g, uint32_t G, int pre,
                                        int T, RowPlanes<NB> &pl) {
#pragma unroll
    for (int b = 0; b < NB; b++) pl.p[b] &= ~G;
    if (P.k == 1) return;                                // rng == 0: numpy draws nothing, every colour is 1
    if (B.left < T) {
        // the batch has run out (rare: > 128 colours in one move), or a replay
        // dropped it: a fresh one from the exact position, its jump-table row
        // reloaded instead of kept across the cascade.  T <= 128: it fits.
        if (B.used > 0) COVER(CV_RP_REBATCH);
        rp_sync(B, g);
        const LaneJump J = load_jump_bp(P, lane, g);
        rp_batch<NB>(P, lane, J, g, B);
    } else if (B.used > 0) {
        COVER(CV_RP_CARRY);
    }
    if (P.thr != 0u) {
        // a rejected word among the T taken: the words after it shift, so
        // replay from the exact position and drop the batch
        if (B.used + T > B.rfirst) {
            rp_sync(B, g);
            rp_replay<NB>(P, w, lane, g, G, pre, T, pl);
            return;
        }
    }
    const bool wide = T > 64;                            // wave-uniform
    if (wide) COVER(CV_RP_WIDE);
    uint32_t sl[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) sl[b] = rp_slice(B.lo[b], B.hi[b], pre, wide);
    rp_advance(B, T);
    rp_deposit<NB>(G, sl, pl);
}
#endif

// Board.move, board.py:330-395, for a board that can hold no special, on row
// planes — the effectiveness test (:352) is the caller's.  J: the jump-table
// row of output bp_out(lane) (rp_batch).  Returns eliminations; leaves the
// final board in LDS and its effective mask in w.effw.
template <int NB, bool CODD, int LV = 0, class WS>
__device__ __forceinline__ int rp_move(const Params &P, WS &w, int lane, const LaneJump &J, Rng &g,
                                       const Cells<WS::NP> &cl, int p1, int p2, int &flags, bool nolds = false) {
    const int R = P.R, C = P.C;
    if constexpr (!(LV & RP_NOLDS)) nolds = false;
    constexpr bool VSHIFT = (LV & RP_VSHIFT) != 0, SCAN2 = (LV & RP_SCAN2) != 0;
    int8_t *col = w.brd;
#if TMG_RP_BATCH
    // Every move that gets here clears a line (the cached mask said so, or
    // eff_exact did), so its first refill is certain: the move's batch is
    // issued ahead of the swap, where its multiply chain overlaps the LDS round
    // trips below.  J is not used after it.
    RpBatch<NB> B{};
    if (P.k != 1) rp_batch<NB>(P, lane, J, g, B);
#endif
    if (lane == 0) {                                     // swap_coords :355 (types are all 1)
        int8_t x = col[p1]; col[p1] = col[p2]; col[p2] = x;
    }
    WSYNC();
    const uint32_t cm = lane < R ? (1u << C) - 1u : 0u;              // C <= 28
    const uint32_t hml = C >= 3 ? cm >> 2 : 0u;                      // columns <= C-3
    const uint32_t vml = lane >= 2 ? cm : 0u;                        // rows >= 2
    RowPlanes<NB> pl = rp_load<NB>(P, w, lane, cm);
    int elim = 0;
    for (;;) {                                           // :367-376
        // get_colour_lines' first pass (:158-193), as bp_first_line_row
        uint32_t neR = 0u, neU = 0u;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const uint32_t x = pl.p[b];
            neR |= x ^ (x >> 1);
            neU |= x ^ rp_dn<1>(x, 0u);
        }
        const uint32_t eqU = ~neU;                                   // same colour as the cell above (rows >= 1)
        const uint32_t h = ~(neR | (neR >> 1)) & hml;
        const uint32_t v = eqU & rp_dn<1>(eqU, 0u) & vml;
        const uint64_t rows = __ballot((h | v) != 0u);
        if (!rows) break;
        COVER(CV_SB_LEAN);
        const int rs = 63 - __clzll(rows);                           // bottom-most row holding a line
        const uint32_t vv = (uint32_t)__builtin_amdgcn_readlane((int)v, rs);
        // its horizontal runs, and the vertical runs ending in it grown upward
        // while the colour holds (:166-172): row t takes column c iff every
        // row in (t, rs] equals the one above it there
        const uint32_t hh = lane == rs ? h : 0u;
        uint32_t K = hh | (hh << 1) | (hh << 2);
        if (vv) {
            const uint32_t run = rp_up<1>(rp_and_below(lane <= rs ? eqU : ~0u), ~0u);
            const uint32_t kv = lane <= rs ? vv & run : 0u;
#if TMG_COVER
            if (__ballot(lane + 3 <= rs && kv != 0u) != 0ULL) COVER(CV_RP_VLONG);
#endif
            K |= kv;
        }
        // the perpendicular pass (:195-214): horizontal runs of >= 3 through a
        // coord over non-coord cells (sb_perpendicular<HORIZ_ONLY>)
        const uint32_t eqR = ~neR & (cm >> 1);                       // same colour as the right neighbour
        const uint32_t walk = cm & ~K;
        const uint32_t r1 = ((K & eqR) << 1) & walk;
        const uint32_t l1 = (K >> 1) & eqR & walk;
        const uint32_t r2 = ((r1 & eqR) << 1) & walk;
        const uint32_t l2 = (l1 >> 1) & eqR & walk;
        const uint32_t q = K & ((r2 >> 2) | (l2 << 2) | ((r1 >> 1) & (l1 << 1)));
        uint32_t clr = K;
        if (q) {
            for (uint32_t f = ((q & eqR) << 1) & walk; f; f = ((f & eqR) << 1) & walk) clr |= f;
            for (uint32_t f = (q >> 1) & eqR & walk; f; f = (f >> 1) & eqR & walk) clr |= f;
        }
#if TMG_COVER
        if (__ballot(q != 0u) != 0ULL) COVER(CV_RP_PERP);
#endif
        // gravity (:217-231): per pass every column with a hole left moves its
        // rows at and above the lowest one down by one; the row shifted in at
        // the top is a cell to refill (G)
        uint32_t E = clr, G = 0u;
        int pass = 0;
        // VSHIFT: a column of vv holds a run of >= 3 cleared cells ending at row rs and
        // no hole below it (rs is the bottom-most row of any line, and every
        // cleared cell lies in a row <= rs), so the loop's first three passes
        // there all find the lowest hole at row rs: rows <= rs take the row
        // three up, at once.  vv and rs are wave-uniform: no scan over lanes
        // for these columns.  Every other column makes its first pass as in
        // the loop; the loop finishes what E still holds (runs longer than 3,
        // a second hole above a run, two separate holes in a column).
        bool settle = true;
        if (VSHIFT && vv) {
            COVER(CV_RP_PASSES);                         // the loop would have needed >= 3 passes
            COVER(CV_RP_VSHIFT);
            const uint32_t M = rp_or_below(E);
            const uint32_t Mv = lane <= rs ? vv : 0u, M1 = M & ~Mv;      // Mv | M1 == M
#pragma unroll
            for (int b = 0; b < NB; b++)
                pl.p[b] = (rp_dn<3>(pl.p[b], 0u) & Mv) | (rp_dn<1>(pl.p[b], 0u) & M1) | (pl.p[b] & ~M);
            E = (rp_dn<3>(E, 0u) & Mv) | (rp_dn<1>(E, 0u) & M1) | (E & ~M);
            G = (rp_dn<3>(0u, ~0u) & Mv) | (rp_dn<1>(0u, ~0u) & M1);
            pass = 1;
            settle = __ballot(E != 0u) != 0ULL;
            if (settle) COVER(CV_RP_VMORE);
        }
        if (settle) {
            for (;; pass++) {
                const uint32_t M = rp_or_below(E);
#pragma unroll
                for (int b = 0; b < NB; b++) pl.p[b] = (rp_dn<1>(pl.p[b], 0u) & M) | (pl.p[b] & ~M);
                E = (rp_dn<1>(E, 0u) & M) | (E & ~M);
                G = (rp_dn<1>(G, ~0u) & M) | (G & ~M);
                if (__ballot(E != 0u) == 0ULL) break;
                // after a three-row shift pass starts at 1: that iteration was counted above
                if (pass == 0) COVER(CV_RP_PASSES);
            }
        }
        // refill (:233-241): row-major draw order
        const int n = __builtin_popcount(G);
        const uint32_t inc = rp_sum_above((uint32_t)n);
        const int T = __builtin_amdgcn_readlane((int)inc, kRpMaxR - 1);
        elim += T;                                       // R*C - nnz(type) after the resolve (:374)
#if TMG_RP_BATCH
        rp_take<NB>(P, w, lane, B, g, G, (int)inc - n, T, pl);
    }
    rp_sync(B, g);                                       // exact before the shuffle, a regeneration, store_rng
#else
        rp_refill<NB>(P, w, lane, J, g, G, (int)inc - n, T, pl);
    }
#endif
    // :381-391, from the planes: the effective mask of the final board; the
    // board to LDS for the write-back; the rare shuffle on the scalar bitboards
    const int any = rp_scan<NB, SCAN2>(P, w, lane, pl, cm);
    // nolds: the board goes to LDS only for the rare shuffle below
    if (!nolds || !any) {
        bp_to_lds<NB>(P, w, lane, pl);
        WSYNC();
    } else {
        COVER(CV_RP_NOLDS);
    }
    if (!any) {
        const LaneJump Jl = load_jump(P, lane, g);
        SBC c = sb_codes_from_lds(P, w.brd, lane);
        flags |= sb_ensure<NB, CODD>(P, w, lane, Jl, g, cl, c, false, true);
    }
    return elim;
}
