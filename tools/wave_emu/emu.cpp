// Host wave emulator (test/debug tool, never part of the product): runs the
// kernels of tile-match-gym_amd/csrc/tmg_board.hip with one host thread per
// lane, so AddressSanitizer / gdb see every LDS and global index.
#include "hip/hip_runtime.h"
#include "tmg_board.hip"
#include "tmg_aux.hip"
#include "tmg_expand.hip"
#include "tmg_dispatch.h"

#include <setjmp.h>
#include <ucontext.h>

#include <cstdio>
#include <dlfcn.h>
#include <cstring>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define EMU_ASAN 1
#endif
#endif
#if defined(__SANITIZE_ADDRESS__)
#define EMU_ASAN 1
#endif
#ifdef EMU_ASAN
#include <sanitizer/common_interface_defs.h>
#endif

EmuDim emu_block_idx, emu_grid_dim;

namespace {
constexpr size_t kStack = 1 << 20;
struct Lane {
    ucontext_t ctx;                 // only used to enter the fiber the first time
    jmp_buf jb;                     // later switches: _setjmp/_longjmp (no signal-mask syscalls)
    std::vector<char> stack;
    int done = 0, op = 0, arg = 0, started = 0;
    void *site = nullptr, *site2 = nullptr, *site3 = nullptr;
    uint64_t val = 0, res = 0;
};
Lane g_lanes[64];
jmp_buf g_main_jb;
int g_cur = -1;
unsigned char *g_smem = nullptr;
void (*g_body)(void *) = nullptr;
void *g_body_arg = nullptr;
#ifdef EMU_ASAN
void *g_main_fake = nullptr;
const void *g_main_bottom = nullptr;
size_t g_main_size = 0;
#endif

void switch_to_lane(int l) {
    g_cur = l;
    if (_setjmp(g_main_jb) == 0) {
#ifdef EMU_ASAN
        __sanitizer_start_switch_fiber(&g_main_fake, g_lanes[l].stack.data(), kStack);
#endif
        if (!g_lanes[l].started) { g_lanes[l].started = 1; setcontext(&g_lanes[l].ctx); }
        _longjmp(g_lanes[l].jb, 1);
    }
#ifdef EMU_ASAN
    __sanitizer_finish_switch_fiber(g_main_fake, &g_main_bottom, &g_main_size);
#endif
}
void yield_to_main(bool finished) {
    Lane &L = g_lanes[g_cur];
#ifdef EMU_ASAN
    void *fake = nullptr;
#endif
    if (finished || _setjmp(L.jb) == 0) {
#ifdef EMU_ASAN
        __sanitizer_start_switch_fiber(finished ? nullptr : &fake, g_main_bottom, g_main_size);
#endif
        _longjmp(g_main_jb, 1);
    }
#ifdef EMU_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
}
void lane_entry() {
#ifdef EMU_ASAN
    __sanitizer_finish_switch_fiber(nullptr, &g_main_bottom, &g_main_size);
#endif
    g_body(g_body_arg);
    g_lanes[g_cur].done = 1;
    yield_to_main(true);
}
}  // namespace

EmuDim emu_thread_idx() { EmuDim d; d.x = (unsigned)g_cur; return d; }
unsigned char *emu_smem() { return g_smem; }

static void print_site(void *a) {
    Dl_info di;
    if (a && dladdr(a, &di) && di.dli_fbase)
        fprintf(stderr, "%s+0x%lx", di.dli_fname, (unsigned long)((char *)a - (char *)di.dli_fbase));
    else
        fprintf(stderr, "%p", a);
}

__attribute__((noinline)) uint64_t emu_collective(int op, uint64_t v, int arg) {
    Lane &L = g_lanes[g_cur];
    L.op = op; L.val = v; L.arg = arg;
    L.site = __builtin_return_address(0);
#ifdef EMU_DEEP_SITES
    L.site2 = __builtin_return_address(1);
    L.site3 = __builtin_return_address(2);
#endif
    yield_to_main(false);
    return g_lanes[g_cur].res;
}

// run one workgroup of one wave: every lane to completion, resolving collectives
static void run_wave(void (*body)(void *), void *arg) {
    g_body = body; g_body_arg = arg;
    for (int l = 0; l < 64; l++) {
        Lane &L = g_lanes[l];
        if (L.stack.empty()) L.stack.resize(kStack);
        getcontext(&L.ctx);
        L.ctx.uc_stack.ss_sp = L.stack.data();
        L.ctx.uc_stack.ss_size = kStack;
        L.ctx.uc_link = nullptr;
        makecontext(&L.ctx, lane_entry, 0);
        L.done = 0; L.op = 0; L.started = 0;
    }
    for (;;) {
        int live = 0;
        for (int l = 0; l < 64; l++)
            if (!g_lanes[l].done) { switch_to_lane(l); }
        int op = 0;
        for (int l = 0; l < 64; l++) {
            if (g_lanes[l].done) continue;
            live++;
            if (op == 0) op = g_lanes[l].op;
            else if (g_lanes[l].op != op) {
                fprintf(stderr, "wave_emu: divergent collectives (lane %d op %d vs %d) at ", l, g_lanes[l].op, op);
                print_site(g_lanes[l].site); fprintf(stderr, "\n"); abort();
            }
        }
        if (!live) break;
        if (live != 64) {
            fprintf(stderr, "wave_emu: block %u: %d lanes exited before a collective; waiting lanes at:\n",
                    emu_block_idx.x, 64 - live);
            for (int l = 0; l < 64; l++) {
                if (g_lanes[l].done) { fprintf(stderr, "  lane %d: exited\n", l); continue; }
                fprintf(stderr, "  lane %d: op %d at ", l, g_lanes[l].op); print_site(g_lanes[l].site);
                fprintf(stderr, " <- "); print_site(g_lanes[l].site2); fprintf(stderr, " <- "); print_site(g_lanes[l].site3);
                fprintf(stderr, "\n");
                if (l > 2) break;
            }
            abort();
        }
        if (op == EMU_BALLOT) {
            uint64_t m = 0;
            for (int l = 0; l < 64; l++) m |= (g_lanes[l].val & 1) << l;
            for (int l = 0; l < 64; l++) g_lanes[l].res = m;
        } else if (op == EMU_READLANE) {
            for (int l = 0; l < 64; l++) g_lanes[l].res = g_lanes[g_lanes[l].arg & 63].val;
        } else if (op == EMU_DPP) {
            for (int l = 0; l < 64; l++) {
                const int a = g_lanes[l].arg, ctrl = a & 0xfff, rm = (a >> 12) & 0xf, bm = (a >> 16) & 0xf;
                const bool bc = (a >> 20) & 1;
                const uint32_t old = (uint32_t)(g_lanes[l].val >> 32);
                const int row = l >> 4, bank = (l & 15) >> 2;
                int srcl = -1;
                if (ctrl <= 0xff) srcl = (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);       // quad_perm
                else if (ctrl >= 0x101 && ctrl <= 0x10f) { int n = ctrl - 0x100; if ((l & 15) + n <= 15) srcl = l + n; }   // row_shl:n
                else if (ctrl >= 0x111 && ctrl <= 0x11f) { int n = ctrl - 0x110; if ((l & 15) >= n) srcl = l - n; }       // row_shr:n
                else if (ctrl == 0x138) { if (l >= 1) srcl = l - 1; }                 // wave_shr:1
                else if (ctrl == 0x130) { if (l <= 62) srcl = l + 1; }                // wave_shl:1
                else if (ctrl == 0x142) { if (row >= 1) srcl = row * 16 - 1; }
                else if (ctrl == 0x143) { if (row >= 2) srcl = 31; }
                else { fprintf(stderr, "wave_emu: unsupported DPP ctrl 0x%x\n", ctrl); abort(); }
                uint32_t r;
                if (!((rm >> row) & 1) || !((bm >> bank) & 1)) r = old;
                else if (srcl < 0) r = bc ? 0u : old;
                else r = (uint32_t)g_lanes[srcl].val;
                g_lanes[l].res = r;
            }
        }
    }
}

template <class F>
static void body_thunk(void *p) { (*reinterpret_cast<F *>(p))(); }

template <class F>
static void run_grid(int64_t nblocks, size_t lds, F kernel) {
    emu_grid_dim.x = (unsigned)nblocks;
    for (int64_t b = 0; b < nblocks; b++) {
        std::vector<unsigned char> smem(lds ? lds : 1);    // exactly sized: ASan catches any overrun
        memset(smem.data(), 0xA5, smem.size());
        g_smem = smem.data();
        emu_block_idx.x = (unsigned)b;
        run_wave(&body_thunk<F>, &kernel);
    }
}

// one wave per env; the grid is padded to 8 XCD blocks like the host launcher does
template <class F>
static void run_blocks(int64_t n, size_t lds, F kernel) {
    int64_t nblocks = n;
    nblocks = (nblocks + 7) & ~(int64_t)7;
    run_grid(nblocks, lds, kernel);
}

static uint64_t g_sbrows[64 * 4];
static uint32_t g_status[4];
static std::vector<int64_t> g_spill_buf;          // a SpillQ with room for every env of the call
static unsigned long long g_spill_total = 0;
static unsigned long long g_cover[tmg::CV_COUNT];
static std::vector<unsigned char> g_spill_ws(sizeof(tmg::WsSerialBig<512>) * tmg::kSpillWaves);
static tmg::SpillQ *spill_queue(std::vector<int64_t> &buf, int64_t n) {
    const size_t words = (sizeof(tmg::SpillQ) + (size_t)n * 8 + 7) / 8;
    buf.assign(words, 0);
    tmg::SpillQ *q = reinterpret_cast<tmg::SpillQ *>(buf.data());
    q->cap = n;
    q->total = 0;
    return q;
}
static tmg::Params make_params(int R, int C, int k, int smask, int moves, const uint64_t *jump) {
    tmg::Params P = tmg::make_params(R, C, k, smask, moves, jump);
    P.status = g_status;
    P.spill = nullptr;
    P.spill_ws = g_spill_ws.data();
    P.cover = g_cover;
    if (P.N <= 128) {
        tmg::build_sb_rows(R, C, g_sbrows);
        P.sb_rows = g_sbrows;
    }
    return P;
}

static uint64_t g_jump[tmg::kJumpRows * 4];
static bool g_jump_init = false;

// The launchers the route and ladders of tmg_dispatch.h call (the library's
// are in tmg_kernels.hip): each member runs the picked instantiation on
// fibers, one wave per env.
struct EmuStep {
    const tmg::Params &P;
    int64_t n;
    int8_t *board; uint64_t *rng; int32_t *timer; const int32_t *actions;
    int32_t *reward, *n_new, *n_act; uint8_t *flags; uint64_t *eff;
    int trust_eff, autoreset;
    template <int MAXN, bool GEN, int NB, bool CODD, int FIX>
    void step() {
        run_blocks(n, sizeof(tmg::Ws<MAXN, GEN>), [&] { tmg::step_kernel<MAXN, GEN, NB, CODD, FIX>(P, n, board, rng, timer, actions, reward, n_new, n_act, flags, eff, trust_eff, autoreset); });
    }
    template <int FIX>
    void step_plain() {
        const int64_t grid = (n + 7) & ~(int64_t)7;                    // run_blocks' padding
        const tmg::PlainHot H{(int32_t)n, (int32_t)(grid >> 3), P.num_moves - 1, autoreset, actions, timer, eff,
                              reward, n_new, n_act, flags, board, rng};
        run_blocks(n, sizeof(tmg::Ws<128, false>), [&] { tmg::plain_step_kernel<FIX>(H, P); });
    }
    template <int MAXN>
    void spill() {
        run_grid(tmg::kSpillWaves, sizeof(tmg::Ws<MAXN, false>), [&] { tmg::spill_kernel<MAXN>(P, n, board, rng, timer, actions, reward, n_new, n_act, flags, eff, trust_eff, autoreset); });
    }
};

struct EmuReset {
    const tmg::Params &P;
    int64_t n;
    int8_t *board; uint64_t *rng; int32_t *timer; uint64_t *eff;
    const uint8_t *mask;
    int bits, epw;
    template <int MAXN, int NB, bool CODD, int FIX>
    void reset() {
        run_blocks((n + epw - 1) / epw, sizeof(tmg::Ws<MAXN, false>),
                   [&] { tmg::reset_kernel<MAXN, NB, CODD, FIX>(P, n, board, rng, timer, eff, mask, bits, epw); });
    }
};

struct EmuEffective {
    const tmg::Params &P;
    int64_t n;
    const int8_t *board; uint64_t *eff;
    template <int MAXN>
    void effective() {
        run_blocks(n, sizeof(tmg::Ws<MAXN, false>), [&] { tmg::effective_kernel<MAXN>(P, n, board, eff); });
    }
};

struct EmuPeek {
    const tmg::Params &P;
    int64_t n;
    const int8_t *board; const uint64_t *rng; const uint64_t *eff;
    int trust_eff;
    int32_t *reward, *n_new, *n_act; uint8_t *flags; int32_t *best_action, *best_reward;
    template <int MAXN, bool GEN, int NB, bool CODD>
    void peek() {
        run_blocks(n, sizeof(tmg::Ws<MAXN, GEN>), [&] { tmg::peek_kernel<MAXN, GEN, NB, CODD>(P, n, board, rng, eff, trust_eff, reward, n_new, n_act, flags, best_action, best_reward); });
    }
    template <int MAXN>
    void spill() {
        run_grid(tmg::kSpillWaves, sizeof(tmg::Ws<MAXN, false>), [&] { tmg::peek_spill_kernel<MAXN>(P, n, board, rng, eff, trust_eff, reward, n_new, n_act, flags, best_action, best_reward); });
    }
};

// tmg_rollout takes peek's dispatch: peek<...>() runs the rollout kernel
struct EmuRollout {
    const tmg::Params &P;
    const tmg::RollArgs &a;
    template <int MAXN, bool GEN, int NB, bool CODD>
    void peek() {
        run_blocks(a.n * a.samples, sizeof(tmg::Ws<MAXN, GEN>), [&] { tmg::rollout_kernel<MAXN, GEN, NB, CODD>(P, a); });
    }
    template <int MAXN>
    void spill() {
        run_grid(tmg::kSpillWaves, sizeof(tmg::Ws<MAXN, false>), [&] { tmg::rollout_spill_kernel<MAXN>(P, a); });
    }
};

// tmg_playout takes peek's dispatch too: peek<...>() runs the playout kernel
struct EmuPlayout {
    const tmg::Params &P;
    const tmg::PlayArgs &a;
    template <int MAXN, bool GEN, int NB, bool CODD>
    void peek() {
        run_blocks(a.n * a.seqs, sizeof(tmg::Ws<MAXN, GEN>), [&] { tmg::playout_kernel<MAXN, GEN, NB, CODD>(P, a); });
    }
    template <int MAXN>
    void spill() {
        run_grid(tmg::kSpillWaves, sizeof(tmg::Ws<MAXN, false>), [&] { tmg::playout_spill_kernel<MAXN>(P, a); });
    }
};

static void emu_do_reset(const tmg::Params &P, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer, uint64_t *eff,
                         const uint8_t *mask, int bits, int epw) {
    EmuReset l{P, n, board, rng, timer, eff, mask, bits, epw};
    tmg::reset_ladder(P, tmg::shape_maxn(P), tmg::shape_sb(P), l);
}

// emu_route's launcher: notes the instantiation a ladder picks, runs nothing
struct Recorder {
    int *out;
    template <int MAXN, bool GEN, int NB, bool CODD, int FIX>
    void step() { out[0] = MAXN; out[1] = GEN; out[2] = NB; out[3] = CODD; out[4] = FIX; }
    // the plain form of step<128, false, NB, false, FIX>: the same instantiation tuple (StepRoute::plain tells them apart)
    template <int FIX>
    void step_plain() { out[0] = 128; out[1] = 0; out[2] = tmg::sb_planes((FIX >> 8) & 255); out[3] = 0; out[4] = FIX; }
    template <int MAXN, int NB, bool CODD, int FIX>
    void reset() { out[0] = MAXN; out[1] = NB; out[2] = CODD; out[3] = FIX; }
    template <int MAXN, bool GEN, int NB, bool CODD>
    void peek() { out[0] = MAXN; out[1] = GEN; out[2] = NB; out[3] = CODD; }
};

extern "C" {

// autoreset as tmg_plan_config (0 none, 1 same step, 2 next step); policy /
// key / first_env / t and the vector-env outputs as tmg_plan_config (NULL: none)
int emu_step(int R, int C, int k, int smask, int moves, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer,
             int32_t *actions, int32_t *reward, int32_t *n_new, int32_t *n_act, uint8_t *flags, uint64_t *eff,
             int trust_eff, int autoreset, int policy, uint64_t key, int64_t first_env, int32_t t, uint8_t *term,
             uint8_t *mask, int64_t *left, int8_t *final_board, int32_t *board32) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    tmg::Params P = make_params(R, C, k, smask, moves, g_jump);
    P.spill = spill_queue(g_spill_buf, n);
    P.sample = policy ? 1 : 0;
    P.pol_key = key;
    P.pol_first = first_env;
    P.pol_t = t;
    P.vo_term = term;
    P.vo_mask = mask;
    P.vo_left = left;
    P.vo_final = final_board;
    P.vo_obs = board32;
    // the library's route, but for the lane kernel, which the emulator has not
    const int maxn = tmg::shape_maxn(P);
    const tmg::StepRoute r = tmg::route_step(P, maxn, trust_eff, autoreset, n, false);
    EmuStep S{P, n, board, rng, timer, actions, reward, n_new, n_act, flags, eff, trust_eff, r.kernel_autoreset};
    tmg::step_ladder(P, maxn, tmg::shape_sb(P), r.lean, S, r.plain);
    if (r.spill) {
        if (maxn == 128) S.spill<128>();
        else S.spill<512>();
    }
    g_spill_total += P.spill->total;
    if (r.deferred) emu_do_reset(P, n, board, rng, timer, eff, flags, tmg::FL_RESET, r.reset_epw);
    return 0;
}

// What the rule picks for a step and for a reset of one call, nothing run.
// fused: bit 0 the one-hot output, bits 1..5 vo_term / vo_mask / vo_left /
// vo_final / vo_obs.  step[12]: MAXN, GEN, NB, CODD, FIX of the step kernel
// (all 0 when the lane kernel takes the step), then lean, lane, deferred,
// kernel_autoreset, spill, reset_epw, plain.  reset[6]: MAXN, NB, CODD, FIX of the
// reset kernel, then the envs per wave of a full and of a masked reset.
int emu_route(int R, int C, int k, int smask, int trust_eff, int mode, int64_t n, int have_lane, int policy, int fused,
              int *step, int *reset) {
    static uint8_t out[8];                              // stands for any requested output buffer
    tmg::Params P = tmg::make_params(R, C, k, smask, 1, nullptr);
    P.sample = policy ? 1 : 0;
    P.oh = fused & 1 ? out : nullptr;
    P.vo_term = fused & 2 ? out : nullptr;
    P.vo_mask = fused & 4 ? out : nullptr;
    P.vo_left = fused & 8 ? reinterpret_cast<int64_t *>(out) : nullptr;
    P.vo_final = fused & 16 ? reinterpret_cast<int8_t *>(out) : nullptr;
    P.vo_obs = fused & 32 ? reinterpret_cast<int32_t *>(out) : nullptr;
    const int maxn = tmg::shape_maxn(P);
    const bool sb = tmg::shape_sb(P);
    const tmg::StepRoute r = tmg::route_step(P, maxn, trust_eff, mode, n, have_lane != 0);
    for (int i = 0; i < 5; i++) step[i] = 0;
    Recorder rs{step}, rr{reset};
    if (!r.lane) tmg::step_ladder(P, maxn, sb, r.lean, rs, r.plain);
    step[5] = r.lean; step[6] = r.lane; step[7] = r.deferred; step[8] = r.kernel_autoreset; step[9] = r.spill;
    step[10] = r.reset_epw; step[11] = r.plain;
    tmg::reset_ladder(P, maxn, sb, rr);
    reset[4] = tmg::reset_envs_per_wave(maxn, false);
    reset[5] = tmg::reset_envs_per_wave(maxn, true);
    return 0;
}

// tmg_peek without the stream: peek_ladder, then (general kernels) the peek
// spill pass.  eff may be NULL when trust_eff == 0; any output may be NULL.
int emu_peek(int R, int C, int k, int smask, int64_t n, const int8_t *board, const uint64_t *rng, const uint64_t *eff,
             int trust_eff, int32_t *reward, int32_t *n_new, int32_t *n_act, uint8_t *flags, int32_t *best_action,
             int32_t *best_reward) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    tmg::Params P = make_params(R, C, k, smask, 1, g_jump);
    P.spill = spill_queue(g_spill_buf, n);
    const int maxn = tmg::shape_maxn(P);
    const bool lean = tmg::lean_step(P, trust_eff);
    EmuPeek S{P, n, board, rng, eff, trust_eff, reward, n_new, n_act, flags, best_action, best_reward};
    tmg::peek_ladder(P, maxn, tmg::shape_sb(P), lean, S);
    if (!lean) {
        if (maxn == 128) S.spill<128>();
        else S.spill<512>();
    }
    g_spill_total += P.spill->total;
    return 0;
}

// out[4]: MAXN, GEN, NB, CODD of the peek kernel the rule picks, nothing run
int emu_peek_route(int R, int C, int k, int smask, int trust_eff, int *out) {
    const tmg::Params P = tmg::make_params(R, C, k, smask, 1, nullptr);
    Recorder r{out};
    tmg::peek_ladder(P, tmg::shape_maxn(P), tmg::shape_sb(P), tmg::lean_step(P, trust_eff), r);
    return 0;
}

// tmg_rollout without the stream: peek_ladder on the rollout kernels, then
// (general kernels) the rollout spill pass, then the reduce kernel when one of
// total / best_action / best_total is asked for.  eff may be NULL when
// trust_eff == 0, timer NULL for no horizon; any output may be NULL.
int emu_rollout(int R, int C, int k, int smask, int moves, int64_t n, const int8_t *board, const uint64_t *rng,
                const int32_t *timer, const uint64_t *eff, int trust_eff, int depth, int samples, uint64_t key,
                int64_t first_env, int32_t t, int32_t *ret, int32_t *plies, uint8_t *flags, int32_t *total,
                int32_t *best_action, int32_t *best_total) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    if (depth < 1 || samples < 1 || ((total || best_action || best_total) && !ret)) return -2;
    tmg::Params P = make_params(R, C, k, smask, moves, g_jump);
    P.spill = spill_queue(g_spill_buf, n * samples);
    P.pol_key = key;
    P.pol_first = first_env;
    P.pol_t = t;
    const int maxn = tmg::shape_maxn(P);
    const bool lean = tmg::lean_step(P, trust_eff);
    const tmg::RollArgs a{n, samples, depth, board, rng, timer, eff, trust_eff ? 1 : 0, ret, plies, flags};
    EmuRollout S{P, a};
    tmg::peek_ladder(P, maxn, tmg::shape_sb(P), lean, S);
    if (!lean) {
        if (maxn == 128) S.spill<128>();
        else S.spill<512>();
    }
    g_spill_total += P.spill->total;
    if (total || best_action || best_total)
        run_blocks(n, 0, [&] { tmg::rollout_reduce_kernel(n, P.A, samples, ret, total, best_action, best_total); });
    return 0;
}

// tmg_playout without the context and the stream: the same refusals (-1 / -2),
// peek_ladder on the playout kernels, then (general kernels) the playout spill
// pass, then the reduce kernel when best_seq or best_ret is asked for.
int emu_playout(int R, int C, int k, int smask, int moves, int64_t n, const int8_t *board, const uint64_t *rng,
                int rng_per_seq, const int32_t *timer, const uint64_t *eff, int trust_eff, int seqs, int depth,
                const int32_t *actions, int32_t *ret, int32_t *n_new, int32_t *n_act, int32_t *plies, uint8_t *flags,
                int32_t *ply_reward, int8_t *out_board, uint64_t *out_rng, int32_t *out_timer, uint64_t *out_eff,
                int32_t *best_seq, int32_t *best_ret) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    if (n < 0 || seqs < 1 || depth < 1) return -2;
    if (n > ((1LL << 26) - 8) / seqs) return -2;
    if (out_timer && !timer) return -1;
    if ((best_seq || best_ret) && !ret) return -1;
    if (reinterpret_cast<uintptr_t>(out_board) & 7) return -2;
    if (n == 0) return 0;
    if (!board || !rng || !actions) return -1;
    if (trust_eff && !eff) return -1;
    tmg::Params P = make_params(R, C, k, smask, moves, g_jump);
    P.spill = spill_queue(g_spill_buf, n * seqs);
    const int maxn = tmg::shape_maxn(P);
    const bool lean = tmg::lean_step(P, trust_eff);
    const tmg::PlayArgs a{n, seqs, depth, board, rng, rng_per_seq ? 1 : 0, timer, eff, trust_eff ? 1 : 0, actions,
                          ret, n_new, n_act, plies, flags, ply_reward, out_board, out_rng, out_timer, out_eff};
    EmuPlayout S{P, a};
    tmg::peek_ladder(P, maxn, tmg::shape_sb(P), lean, S);
    if (!lean) {
        if (maxn == 128) S.spill<128>();
        else S.spill<512>();
    }
    g_spill_total += P.spill->total;
    if (best_seq || best_ret) run_blocks(n, 0, [&] { tmg::playout_reduce_kernel(n, seqs, ret, best_seq, best_ret); });
    return 0;
}

// tmg_trace without the context and the stream: the same refusals (-1 / -2),
// the general non-bitboard trace kernel of the shape's size class, then its
// spill pass.
int emu_trace(int R, int C, int k, int smask, int64_t n, const int8_t *board, const uint64_t *rng, const uint64_t *eff,
              int trust_eff, int seqs, const int32_t *actions, uint32_t stage_mask, int max_frames, int stop,
              int8_t *frames, uint8_t *kind, int32_t *frame_elim, int32_t *n_frames, int32_t *reward, int32_t *n_new,
              int32_t *n_act, uint8_t *flags, uint64_t *out_rng) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    if (n < 0 || seqs < 1 || max_frames < 1) return -2;
    if (stage_mask == 0 || (stage_mask & ~0x7Eu)) return -2;
    if (n > ((1LL << 26) - 8) / seqs) return -2;
    if ((2 * R * C) % 4 == 0 && (reinterpret_cast<uintptr_t>(frames) & 3)) return -2;
    if (n == 0) return 0;
    if (!board || !rng || !actions) return -1;
    if (trust_eff && !eff) return -1;
    tmg::Params P = make_params(R, C, k, smask, 1, g_jump);
    P.spill = spill_queue(g_spill_buf, n * seqs);
    const int maxn = tmg::shape_maxn(P);
    const tmg::TraceArgs a{n, seqs, board, rng, eff, trust_eff ? 1 : 0, actions, stage_mask, max_frames, stop ? 1 : 0,
                           frames, kind, frame_elim, n_frames, reward, n_new, n_act, flags, out_rng};
    if (maxn == 128) {
        run_blocks(n * seqs, sizeof(tmg::Ws<128, true>), [&] { tmg::trace_kernel<128>(P, a); });
        run_grid(tmg::kSpillWaves, sizeof(tmg::Ws<128, false>), [&] { tmg::trace_spill_kernel<128>(P, a); });
    } else {
        run_blocks(n * seqs, sizeof(tmg::Ws<512, true>), [&] { tmg::trace_kernel<512>(P, a); });
        run_grid(tmg::kSpillWaves, sizeof(tmg::Ws<512, false>), [&] { tmg::trace_spill_kernel<512>(P, a); });
    }
    g_spill_total += P.spill->total;
    return 0;
}

// tmg_expand_count without the context and the stream: the three launches of
// expand_count_kernel (csrc/tmg_expand.hip), one wave per tile of envs
int emu_expand_count(int R, int C, int moves, int64_t n, const int32_t *timer, const uint64_t *eff,
                     const uint64_t *select, int64_t *first_child) {
    if (n < 0 || !first_child || (n > 0 && (!timer || !eff))) return -2;
    const int A = 2 * R * C - R - C;
    const tmg::ExpandCountArgs a{n, (A + 63) / 64, A, moves, timer, eff, select, first_child};
    const int64_t tiles = (n + tmg::kExpandTile - 1) / tmg::kExpandTile;
    if (tiles) run_grid(tiles, 0, [&] { tmg::expand_count_kernel<0>(a); });
    run_grid(1, 0, [&] { tmg::expand_count_kernel<1>(a); });
    if (tiles) run_grid(tiles, 0, [&] { tmg::expand_count_kernel<2>(a); });
    return 0;
}

// tmg_expand without the stream: the gather kernel, then emu_step on the m
// child rows.  pack: 1 / 0 the gather's two store variants, -1 the library's
// (TMG_EXPAND_PACK).  The refusals are tmg_expand's (-1 / -2).
int emu_expand(int R, int C, int k, int smask, int moves, int64_t n, const int8_t *board, const uint64_t *rng,
               const int32_t *timer, const uint64_t *eff, const uint64_t *select, int trust_eff,
               const int64_t *first_child, int64_t m, int8_t *child_board, uint64_t *child_rng, int32_t *child_timer,
               uint64_t *child_eff, int64_t *child_parent, int32_t *child_action, int32_t *child_reward,
               int32_t *child_n_new, int32_t *child_n_act, uint8_t *child_flags, int pack) {
    if (n < 0 || m < 0) return -2;
    if (n == 0 || m == 0) return 0;
    if (!board || !rng || !timer || !eff || !first_child || !child_board || !child_rng || !child_timer || !child_eff ||
        !child_action || !child_reward || !child_n_new || !child_n_act || !child_flags)
        return -1;
    if (reinterpret_cast<uintptr_t>(child_board) & 7) return -2;
    const tmg::Params P = tmg::make_params(R, C, k, smask, moves, nullptr);
    const tmg::ExpandArgs a{n, m, P.N, P.W, P.A, P.num_moves, board, rng, timer, eff, select, first_child,
                            child_board, child_rng, child_timer, child_eff, child_parent, child_action};
    const bool pk = pack < 0 ? tmg::kExpandPack : pack != 0;
    if (tmg::shape_maxn(P) == 128) {
        if (pk) run_blocks(n, 0, [&] { tmg::expand_gather_kernel<1, true>(a); });
        else run_blocks(n, 0, [&] { tmg::expand_gather_kernel<1, false>(a); });
    } else {
        if (pk) run_blocks(n, 0, [&] { tmg::expand_gather_kernel<4, true>(a); });
        else run_blocks(n, 0, [&] { tmg::expand_gather_kernel<4, false>(a); });
    }
    return emu_step(R, C, k, smask, moves, m, child_board, child_rng, child_timer, child_action, child_reward,
                    child_n_new, child_n_act, child_flags, child_eff, trust_eff, 0, 0, 0, 0, 0, nullptr, nullptr,
                    nullptr, nullptr, nullptr);
}

// tmg_seed without the context and the stream: the same arguments and
// refusals (-1 / -2), seed_row (tmg_seed.h) on every row in turn.  The store
// variant bits of mode are accepted and change nothing here.
int emu_seed(int64_t m, int mode, const uint64_t *seeds, int seed_words, uint64_t base_lo, uint64_t base_hi,
             uint64_t key0, uint64_t key1, int64_t period, uint64_t *rng) {
    int rc = 0;
    if (tmg::seed_refusal(m, mode, seeds, seed_words, base_lo, base_hi, key0, key1, period, rng, &rc)) return rc;
    const tmg::SeedArgs a{m, (mode & tmg::kSeedSpawn) != 0, seeds, seed_words, base_lo, base_hi, key0, key1, period, rng};
    for (int64_t j = 0; j < m; j++) tmg::seed_row(a, j, rng + j * 5);
    return 0;
}

unsigned long long emu_spills(void) { return g_spill_total; }
int emu_cover_count(void) { return tmg::CV_COUNT; }
void emu_cover(unsigned long long *out, int clear) {
    for (int i = 0; i < tmg::CV_COUNT; i++) { out[i] = g_cover[i]; if (clear) g_cover[i] = 0; }
}
unsigned emu_status(void) { return (g_status[0] ? 1u : 0u) | (g_status[1] ? 2u : 0u) | (g_status[2] ? 4u : 0u); }
// tmg_status with clear != 0: the sticky bits so far, then none
unsigned emu_status_clear(void) {
    const unsigned st = emu_status();
    for (uint32_t &s : g_status) s = 0;
    return st;
}

int emu_reset(int R, int C, int k, int smask, int moves, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer,
              uint64_t *eff) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    tmg::Params P = make_params(R, C, k, smask, moves, g_jump);
    emu_do_reset(P, n, board, rng, timer, eff, nullptr, 0xFF, tmg::reset_envs_per_wave(tmg::shape_maxn(P), false));
    return 0;
}

// reset(env_mask): the masked reset_kernel launch (several envs per wave)
int emu_reset_masked(int R, int C, int k, int smask, int moves, int64_t n, int8_t *board, uint64_t *rng,
                     int32_t *timer, uint64_t *eff, const uint8_t *mask, int bits) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    tmg::Params P = make_params(R, C, k, smask, moves, g_jump);
    emu_do_reset(P, n, board, rng, timer, eff, mask, bits, tmg::reset_envs_per_wave(tmg::shape_maxn(P), mask != nullptr));
    return 0;
}

int emu_effective(int R, int C, int k, int smask, int64_t n, const int8_t *board, uint64_t *eff) {
    if (!g_jump_init) { tmg::build_jump_table(g_jump); g_jump_init = true; }
    tmg::Params P = make_params(R, C, k, smask, 1, g_jump);
    EmuEffective l{P, n, board, eff};
    tmg::effective_ladder(tmg::shape_maxn(P), l);
    return 0;
}

}  // extern "C"
