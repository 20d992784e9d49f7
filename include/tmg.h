/*
 * tmg.h — C ABI of libtmg.so, the MI355X (gfx950) batched tile-match Board.
 *
 * The reference (akshilpatel/tile-match-gym v1.0.6) has no FFI: its hot path is
 * the Python class API below, and this ABI is what a binding of that path
 * binds (the ctypes stub lives in tile_match_gym_amd/_native.py; see
 * INTEGRATION.md).  Each entry point cites the reference interface it replaces.
 *
 * Batched state (device memory, owned by the caller, e.g. PyTorch tensors):
 *   board  int8   [n][2][R][C]   plane 0 colour (0 empty/colourless, 1..k),
 *                                plane 1 type (0 empty, 1 normal, 2 v-laser,
 *                                3 h-laser, 4 bomb, -1 cookie)   board.py:18-25,96
 *   rng    uint64 [n][5]         numpy PCG64 per env: state lo/hi, inc lo/hi,
 *                                has_uint32<<32 | uinteger       tile_match_env.py:49
 *   timer  int32  [n]            moves taken this episode         tile_match_env.py:88,100
 *   eff    uint64 [n][W]         effective-action bitmask, W = ceil(A/64),
 *                                A = 2RC-R-C; bit a of word a/64  tile_match_env.py:118-124
 * Per-step outputs (device memory):
 *   reward int32 [n]   num_eliminations                            board.py:330-395
 *   n_new  int32 [n]   info["num_new_specials"]
 *   n_act  int32 [n]   info["num_specials_activated"]
 *   flags  uint8 [n]   bit0 done, bit1 is_combination_match, bit2 shuffled,
 *                      bit3 autoreset ran, bit7 error (step after done / bad
 *                      action, or an internal safety cap)  tile_match_env.py:94-95
 *                      (bit6, capacity overflow, is no longer produced: a step
 *                      whose cascade outgrows the kernels' LDS lists is re-run
 *                      on worst-case lists, and the queue of such steps holds
 *                      every env of the launch)
 *
 * Errors: 0 = ok, negative = error; tmg_last_error() gives a thread-local
 * message.  All launches are asynchronous on `stream` (a hipStream_t; NULL =
 * default stream).  Not re-entrant per context.
 */
#ifndef TMG_H
#define TMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tmg_ctx tmg_ctx;

#if defined(__GNUC__) || defined(__clang__)
#define TMG_API __attribute__((visibility("default")))
#else
#define TMG_API
#endif

/* Special-tile mask bits (Board(colourless_specials=..., colour_specials=...), board.py:42-61). */
#define TMG_SPECIAL_COOKIE 1u
#define TMG_SPECIAL_VLASER 2u
#define TMG_SPECIAL_HLASER 4u
#define TMG_SPECIAL_BOMB   8u

#define TMG_FLAG_DONE      0x01u
#define TMG_FLAG_COMBO     0x02u
#define TMG_FLAG_SHUFFLED  0x04u
#define TMG_FLAG_RESET     0x08u
#define TMG_FLAG_OVERFLOW  0x40u   /* not produced since ABI 3 (kept for old callers) */
#define TMG_FLAG_ERROR     0x80u

/* Replaces TileMatchEnv.__init__ / Board.__init__ (tile_match_env.py:17-77,
 * board.py:42-93): fixes the shape, colours, specials and episode length for a
 * batch, builds the action->coords table (board.py:77-93) and the PCG64
 * jump-ahead table on `device`. */
TMG_API int tmg_create(tmg_ctx **out, int device, int rows, int cols, int colours,
               uint32_t specials_mask, int num_moves);

/* A context for tmg_effective only, on any rows x cols board of up to 512
 * cells (no viability test, no colours or specials): the module-level
 * is_move_effective(board, c1, c2) / Board.possible_move(grid) of the
 * reference (board.py:558-569, 735-787), which accept any board.  Every other
 * call on it fails. */
TMG_API int tmg_create_scan(tmg_ctx **out, int device, int rows, int cols);

/* Frees the context's device tables.  Never frees caller buffers. */
TMG_API int tmg_destroy(tmg_ctx *ctx);

/* Replaces TileMatchEnv.reset (tile_match_env.py:84-91 -> Board.generate_board,
 * board.py:95-131) for every env i with env_mask == NULL or env_mask[i] != 0:
 * generates a board from the env's RNG stream (continuing it, like reset()
 * without a seed), sets timer = 0 and writes the effective-action mask. */
TMG_API int tmg_reset(tmg_ctx *ctx, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer,
              uint64_t *eff, const uint8_t *env_mask, void *stream);

/* Replaces TileMatchEnv.step (tile_match_env.py:93-112 -> Board.move,
 * board.py:330-395) for n envs at once.  actions[i] in [0, A).
 * trust_eff != 0: eff holds the mask a tmg_step / tmg_reset of this library
 *   wrote for the current boards (the effectiveness test of board.py:352 is
 *   then a bit lookup, and the boards are known to hold no line, which bounds
 *   the first line search); pass 0 after editing boards by hand, also when the
 *   mask was then recomputed by tmg_effective.
 * autoreset != 0: an env whose episode ends is regenerated in the same call
 *   (continuing its RNG stream, == reset() without a seed); reward / flags
 *   still describe the final move and flag bit3 is set.  With autoreset == 0
 *   a finished env writes an all-zero eff mask (tile_match_env.py:119-120) and
 *   a further step sets TMG_FLAG_ERROR without touching its state.
 * The type plane: with no special enabled and trust_eff != 0, every
 *   wave-per-board launch verifies it (a non-normal tile sets TMG_FLAG_ERROR
 *   for that env, leaves its board, RNG words and timer untouched and raises
 *   TMG_STATUS_INTERNAL), while the lane-per-board launch (10x10 boards of 4
 *   or 5 colours, under the in-kernel policy or from 131072 envs on) reads
 *   only the colour plane and relies on the caller. */
TMG_API int tmg_step(tmg_ctx *ctx, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer,
             const int32_t *actions, int32_t *reward, int32_t *n_new, int32_t *n_act,
             uint8_t *flags, uint64_t *eff, int trust_eff, int autoreset, void *stream);

/* What tmg_step(actions[i] = a) would report for env i, for every action a in
 * [0, A) at once, from the current state and without changing it: Board.move
 * (board.py:330-395) run on a copy of the board with a copy of the env's RNG
 * stream.  Reads board, rng and (trust_eff != 0) eff; writes only the outputs,
 * each [n][A] (or [n]) and each optional.
 *   Ineffective actions (board.py:352-353): reward 0, n_new 0, n_act 0, flags 0.
 *   best_action: the lowest action index among those of maximal reward over
 *     all A actions; an env with no effective action gets action 0, reward 0.
 *   The timer is neither read nor written and TMG_FLAG_DONE / TMG_FLAG_RESET
 *     are never set: peek describes the move, not the episode.  With trust_eff
 *     != 0 a finished env of a no-autoreset batch has an all-zero mask, so all
 *     its outputs are zero.
 *   trust_eff: as tmg_step.  Non-zero: eff is this library's mask of these
 *     boards (the lean kernels run when no special is enabled; the first line
 *     search is bounded).  Zero: eff may be NULL; the mask of each board is
 *     scanned as it stands and the general kernels run, so hand-edited boards
 *     work, including boards that already hold a line.
 *   rng is only read.  The envs' own array answers "what will this move
 *     return" exactly (an oracle-greedy policy: it sees the refills the env
 *     will really draw).  Any other [n][5] array of PCG64 words gives an
 *     honest sampled lookahead, whose refills are not the ones the env will
 *     draw: the fair baseline.
 *   Errors as for a step: bit 7 of that action's flags entry and
 *     TMG_STATUS_INTERNAL in the sticky status.  A lean launch that meets a
 *     non-normal tile flags every action of that env and raises
 *     TMG_STATUS_INTERNAL.
 *   n == 0 is a no-op; a tmg_create_scan context refuses the call.  Envs one
 *     of whose actions outgrew the kernels' LDS lists are re-run whole on the
 *     worst-case lists and count in tmg_spills. */
TMG_API int tmg_peek(tmg_ctx *ctx, int64_t n, const int8_t *board, const uint64_t *rng, const uint64_t *eff,
                     int trust_eff,
                     int32_t *reward,       /* [n][A] num_eliminations             or NULL */
                     int32_t *n_new,        /* [n][A]                              or NULL */
                     int32_t *n_act,        /* [n][A]                              or NULL */
                     uint8_t *flags,        /* [n][A] TMG_FLAG_COMBO | SHUFFLED | ERROR, or NULL */
                     int32_t *best_action,  /* [n] lowest a of maximal reward      or NULL */
                     int32_t *best_reward,  /* [n] that reward                     or NULL */
                     void *stream);

/* Policy rollouts of every action, without changing any state: the simulation
 * step of a Monte-Carlo planner.  Rollout (s, i, a), for every sample s in
 * [0, samples), env i and action a in [0, A):
 *   State: a copy of board[i] and of the RNG words rng[s][i].
 *   An action that is not effective on the board as it stands: ret = plies =
 *     flags = 0 (trust_eff as tmg_peek: non-zero, eff is this library's mask
 *     and the lean kernels run when no special is enabled; zero, eff may be
 *     NULL, the mask is scanned and hand-edited boards work).
 *   Horizon: H = depth when timer is NULL, else min(depth, num_moves -
 *     timer[i]) (the episode ends when the timer reaches num_moves).  H <= 0,
 *     a finished env: zeros for every action of that env.
 *   Ply 0 is Board.move(a) (board.py:330-395).  Ply d, 1 <= d < H, plays the
 *     action tmg_sample_effective would draw for that env from the mask of the
 *     board as ply d - 1 left it, with key (key + s * A + a) mod 2^64, global
 *     env first_env + i and step counter t + d (src/examples/q_learning.py:
 *     19-25: uniform over the effective actions).  The RNG stream runs on from
 *     ply to ply.
 *   ret: the sum of the plies' num_eliminations; plies: how many were played;
 *     flags: the OR of the plies' TMG_FLAG_COMBO | TMG_FLAG_SHUFFLED.  A ply
 *     that ends on a safety cap sets TMG_FLAG_ERROR, stops that rollout and
 *     raises TMG_STATUS_INTERNAL; a lean launch that meets a non-normal tile
 *     flags every action of that (s, i), as tmg_peek does.
 *   total[i][a] = sum over s of ret[s][i][a]; best_action[i]: the lowest a of
 *     maximal total over all A actions (0 when none is effective);
 *     best_total[i]: that total.  These three need ret.
 *   With depth == 1 and samples == 1, ret / flags are tmg_peek's reward /
 *     flags for the same rng.
 *   depth >= 1, samples >= 1, n * samples <= 2^26 - 8 (one wave each).  n == 0
 *     is a no-op; a tmg_create_scan context refuses the call.  Nothing of
 *     board, rng, timer, eff is written.  A (sample, env) one of whose plies
 *     outgrew the kernels' LDS lists is re-run whole on the worst-case lists
 *     and counts in tmg_spills. */
TMG_API int tmg_rollout(tmg_ctx *ctx, int64_t n, const int8_t *board,
                        const uint64_t *rng,      /* [samples][n][5], only read */
                        const int32_t *timer,     /* [n] or NULL (no horizon) */
                        const uint64_t *eff, int trust_eff,
                        int depth, int samples, uint64_t key, int64_t first_env, int32_t t,
                        int32_t *ret,             /* [samples][n][A] summed num_eliminations, or NULL */
                        int32_t *plies,           /* [samples][n][A] moves played (0 = not simulated), or NULL */
                        uint8_t *flags,           /* [samples][n][A] OR of COMBO | SHUFFLED | ERROR, or NULL */
                        int32_t *total,           /* [n][A] sum over samples of ret, or NULL */
                        int32_t *best_action,     /* [n] lowest a of maximal total, or NULL */
                        int32_t *best_total,      /* [n] that total, or NULL */
                        void *stream);

/* Given action sequences played on copies of every env, without changing any
 * state: what a shooting planner asks (random shooting, CEM, beam refinement,
 * the replay of a recorded trajectory).  Row (q, i), for every sequence q in
 * [0, seqs) and env i, is exactly what successive tmg_step(autoreset = 0) calls
 * with actions[q][i][0], [1], ... leave and report on a one-env copy of env i
 * whose RNG words are rng[i] (rng[q][i] when rng_per_seq != 0).
 *   An effective action is Board.move (board.py:330-395); the RNG stream runs
 *     on from ply to ply.  An ineffective action is a move like any other
 *     (board.py:352-353, tile_match_env.py:100): reward 0, board and RNG words
 *     unchanged, it counts in plies and the timer goes up by one.  trust_eff
 *     as tmg_rollout: non-zero, eff is this library's mask and the lean
 *     kernels run when no special is enabled; zero, eff may be NULL, the mask
 *     is scanned and hand-edited boards work.
 *   A negative action ends the sequence quietly (padding of ragged
 *     sequences): a sequence that starts with one has plies = 0, zero sums and
 *     flags, and its final state is its parent's.
 *   An action >= A is what a bad action is to a step: TMG_FLAG_ERROR in flags,
 *     the sequence stops before that ply with the state as the ply before left
 *     it, and TMG_STATUS_CALLER is raised.
 *   Horizon: H = depth when timer is NULL, else min(depth, num_moves -
 *     timer[i]); a sequence never steps after done.  One that reaches
 *     num_moves carries TMG_FLAG_DONE and an all-zero out_eff row
 *     (tile_match_env.py:119-120).  H <= 0, a finished env: zeros, and a final
 *     state that is a copy of the parent with a zero mask.
 *   ret / n_new / n_act: the sums over the plies played of the steps' reward
 *     / n_new / n_act; plies: how many were played; ply_reward[q][i][d]: ply
 *     d's reward, 0 for plies not played; flags: the OR of the plies'
 *     TMG_FLAG_COMBO | SHUFFLED | ERROR, plus DONE.  A ply that ends on a
 *     safety cap sets TMG_FLAG_ERROR, stops that sequence (the ply counted) and
 *     raises TMG_STATUS_INTERNAL; a lean launch that loads a non-normal tile
 *     flags every sequence of that env and plays none, as tmg_peek does.
 *   out_board / out_rng / out_timer / out_eff: the state after the last ply
 *     played, out_timer = timer[i] + plies (it needs timer), out_eff the
 *     library's own mask of out_board: the rows can be stepped, peeked or
 *     expanded with trust_eff = 1.
 *   best_seq[i]: the lowest q of maximal ret[q][i], best_ret[i] that value
 *     (any seqs); both need ret.
 *   Nothing of board, rng, timer, eff or actions is written.  A virtual env
 *     one of whose plies outgrew the kernels' LDS lists is re-run whole on the
 *     worst-case lists and counts in tmg_spills.
 *   Refused: a tmg_create_scan context, n < 0, seqs < 1, depth < 1, n * seqs
 *     above 2^26 - 8 (one wave each), a null board, rng or actions with n > 0,
 *     trust_eff != 0 with a null eff, out_timer without timer, best_seq /
 *     best_ret without ret, an out_board that is not 8-byte aligned (the
 *     lane-per-board step reads boards as 8-byte words).  n == 0 is a no-op.
 *     Asynchronous on `stream`. */
TMG_API int tmg_playout(tmg_ctx *ctx, int64_t n, const int8_t *board,
                        const uint64_t *rng, int rng_per_seq,   /* [n][5], or [seqs][n][5] when rng_per_seq != 0; only read */
                        const int32_t *timer,                   /* [n] or NULL (no horizon) */
                        const uint64_t *eff, int trust_eff,
                        int seqs, int depth,
                        const int32_t *actions,                 /* [seqs][n][depth] */
                        int32_t *ret, int32_t *n_new, int32_t *n_act,   /* [seqs][n] sums over the plies, each or NULL */
                        int32_t *plies, uint8_t *flags,         /* [seqs][n], each or NULL */
                        int32_t *ply_reward,                    /* [seqs][n][depth] or NULL */
                        int8_t *out_board, uint64_t *out_rng, int32_t *out_timer, uint64_t *out_eff, /* [seqs][n]..., each or NULL */
                        int32_t *best_seq, int32_t *best_ret,   /* [n], each or NULL; need ret */
                        void *stream);

/* One move's cascade stage by stage, on copies of every env: what happens
 * inside Board.move (board.py:330-395).  Row (q, i), for every action row q in
 * [0, seqs) and env i, traces Board.move(actions[q][i]) on a copy of board[i]
 * with a copy of rng[i].  Nothing of board, rng, eff or actions is written;
 * the timer is neither read nor written and TMG_FLAG_DONE is never set, as
 * for tmg_peek.
 *   Stages of a move, in order: SWAP; if the move is a combination, COMBO,
 *     FALL, REFILL; per cascade iteration CLEAR, FALL, REFILL; SHUFFLE when the
 *     ensure-playable loop shuffled (all its shuffles and row redraws in one
 *     frame).  A FALL or REFILL that moves or fills nothing is still a stage.
 *   A stage is recorded when bit (1u << kind) is set in stage_mask.  The f-th
 *     recorded stage writes frames[q][i][f] (the board after it, both planes),
 *     kind[q][i][f] and frame_elim[q][i][f]: the reference's count of type-zero
 *     cells after a COMBO or CLEAR stage (board.py:361, :373), 0 for the other
 *     kinds.  The first FALL frame of a move, before any draw, is its
 *     afterstate.
 *   stop == 0: the move is simulated to its end.  Stages past max_frames are
 *     not recorded; n_frames counts all stages of the selected kinds, so
 *     n_frames > max_frames says the trace was cut.  reward / n_new / n_act /
 *     flags (TMG_FLAG_COMBO | SHUFFLED | ERROR) are exactly tmg_peek's for that
 *     action and rng, out_rng the words after the move, and the sum of every
 *     stage's frame_elim plus n_new is reward.
 *   stop != 0: the row ends right after its max_frames-th recorded frame is
 *     written and carries TMG_FLAG_STOPPED; n_frames <= max_frames.  reward,
 *     n_new and n_act cover the stages simulated so far (reward = their
 *     frame_elim sum + n_new so far), flags holds TMG_FLAG_COMBO once the COMBO
 *     stage has run and TMG_FLAG_SHUFFLED once the SHUFFLE stage has, out_rng
 *     the words as those stages left them.  A row whose move ends with fewer
 *     recorded frames is not stopped and equals the stop == 0 row.
 *     stage_mask = 1u << TMG_STAGE_FALL, max_frames = 1, stop = 1 is the
 *     afterstate form: out_rng equals rng[i] (no draw was made) and reward is
 *     the deterministic part of the move's reward.
 *   kind / frame_elim entries from min(n_frames, max_frames) on are zeroed;
 *     frame boards there are not written.
 *   An ineffective action, as trust_eff defines it, gives zeros, n_frames = 0
 *     and out_rng = rng[i]; a negative action is quiet padding and gives the
 *     same.  An action >= A sets TMG_FLAG_ERROR with n_frames = 0 and raises
 *     TMG_STATUS_CALLER.  trust_eff as tmg_peek: non-zero, eff is this
 *     library's mask and the first line search is bounded; zero, eff may be
 *     NULL, the mask is scanned and boards that already hold a line work.
 *   The general kernels always run (there is no lean precondition): a board
 *     that holds specials in a no-specials context is traced as the general
 *     step kernels would step it.  A stage that ends on a safety cap sets
 *     TMG_FLAG_ERROR, the frames written so far stay valid, and
 *     TMG_STATUS_INTERNAL is raised.  A row whose cascade outgrows the
 *     kernels' LDS lists is re-run whole on the worst-case lists, every output
 *     rewritten, and counts in tmg_spills.
 *   frames: row (q, i)'s slot f starts at byte ((q * n + i) * max_frames + f)
 *     * 2 * R * C.  When 2 * R * C is a multiple of 4 the frames are written as
 *     32-bit words and `frames` must be 4-byte aligned; otherwise they are
 *     written as bytes, any address works and slots start on 2-byte boundaries.
 *   Refused: a tmg_create_scan context, n < 0, seqs < 1, max_frames < 1, a
 *     stage_mask that is zero or has bits outside kinds 1..6, n * seqs above
 *     2^26 - 8 (one wave each), a null board, rng or actions with n > 0,
 *     trust_eff != 0 with a null eff, a misaligned frames.  n == 0 is a no-op.
 *     Asynchronous on `stream`. */
#define TMG_STAGE_SWAP    1  /* after swap_coords                          board.py:355     */
#define TMG_STAGE_COMBO   2  /* after combination_match, before gravity    board.py:357-364 */
#define TMG_STAGE_CLEAR   3  /* after one cascade iteration's resolve: cells cleared,
                                new specials placed                        board.py:367-376 */
#define TMG_STAGE_FALL    4  /* after gravity                              board.py:217-229 */
#define TMG_STAGE_REFILL  5  /* after refill                               board.py:231-241 */
#define TMG_STAGE_SHUFFLE 6  /* after the whole ensure-playable loop, only when it shuffled:
                                all its shuffles and row redraws in one frame  board.py:381-391 */
#define TMG_FLAG_STOPPED  0x10u   /* produced by tmg_trace only */
TMG_API int tmg_trace(tmg_ctx *ctx, int64_t n, const int8_t *board, const uint64_t *rng /* [n][5] */,
                      const uint64_t *eff, int trust_eff,
                      int seqs, const int32_t *actions /* [seqs][n] */,
                      uint32_t stage_mask, int max_frames, int stop,
                      int8_t *frames      /* [seqs][n][max_frames][2][R][C] or NULL */,
                      uint8_t *kind       /* [seqs][n][max_frames] or NULL */,
                      int32_t *frame_elim /* [seqs][n][max_frames] or NULL */,
                      int32_t *n_frames   /* [seqs][n] or NULL */,
                      int32_t *reward, int32_t *n_new, int32_t *n_act, uint8_t *flags /* [seqs][n], each or NULL */,
                      uint64_t *out_rng   /* [seqs][n][5] or NULL */, void *stream);

/* Successor states of every effective action: the expansion step of a tree
 * search that keeps its children (board, RNG position, timer, mask), to peek,
 * roll out, expand again or score them.  Two calls: tmg_expand_count places
 * the children, tmg_expand writes and steps them.
 *
 * tmg_expand_count: first_child[i] = number of children of envs 0..i-1 (an
 * exclusive prefix sum), first_child[n] = the total.  Env i has one child per
 * action a in [0, A) whose bit is set in eff[i] (and in select[i], when select
 * != NULL); bits at or above A are ignored; an env with timer[i] >= num_moves
 * has none, whatever its mask.  Computed on the device with no host round
 * trip, deterministically, for any n up to 2^31.  n == 0 writes first_child[0]
 * = 0.  Refused: a tmg_create_scan context, negative n, a null first_child, a
 * null timer or eff with n > 0. */
TMG_API int tmg_expand_count(tmg_ctx *ctx, int64_t n, const int32_t *timer, const uint64_t *eff,
                             const uint64_t *select /* [n][W] or NULL */,
                             int64_t *first_child /* [n+1], device */, void *stream);

/* tmg_expand: child row c = first_child[i] + (rank of a among env i's expanded
 * actions, ascending) becomes exactly what tmg_step(actions = a, autoreset = 0)
 * leaves and reports on a copy of env i whose RNG words are rng[i].
 *   The child: row c of child_board / child_rng / child_timer / child_eff is
 *     the state after the move (Board.move, board.py:330-395; child_timer =
 *     timer[i] + 1), row c of child_reward / child_n_new / child_n_act /
 *     child_flags what the move reports.  A child that reaches num_moves
 *     carries TMG_FLAG_DONE and an all-zero mask (tile_match_env.py:119-120).
 *     child_parent[c] = i (optional), child_action[c] = a.  Children are
 *     ordered env-major, then by ascending action.  Nothing of board, rng,
 *     timer, eff, select or first_child is written.
 *   rng: as tmg_peek.  The envs' own array gives the children the env would
 *     really reach; any other [n][5] array of PCG64 words gives sampled
 *     children.
 *   trust_eff: as tmg_step.  Non-zero: eff is this library's mask of these
 *     boards.  Zero: the boards were edited by hand, eff is the mask
 *     tmg_effective wrote for them, and the general kernels run.  eff is
 *     required either way: it names the children.  A child of an action that
 *     turns out ineffective is what a step of it is: reward 0, board
 *     unchanged, timer + 1.
 *   m: the number of child rows to produce, known to the host (the caller
 *     reads first_child[n] after tmg_expand_count).  m below the total expands
 *     the first m rows only, a prefix; rows from m on are not touched.  For m
 *     above the total the excess rows get child_timer = num_moves,
 *     child_action = 0, child_parent = -1 and a zero mask, and the step treats
 *     them as steps after done: TMG_FLAG_ERROR, board and RNG words untouched,
 *     TMG_STATUS_CALLER.  No kernel runs on rows nobody initialised.
 *   The moves are a tmg_step of the m rows, routed as any step (the
 *     lane-per-board, shape-specialised or generic kernels); steps that
 *     outgrow the LDS lists go through the spill tier and count in tmg_spills.
 *   Refused: a tmg_create_scan context, negative n or m, n or m above 2^26 - 8
 *     (one wave each), a null required pointer, a child_board that is not
 *     8-byte aligned (the lane-per-board step reads boards as 8-byte words).
 *     n == 0 or m == 0 is a no-op.  Asynchronous on `stream`. */
TMG_API int tmg_expand(tmg_ctx *ctx, int64_t n, const int8_t *board, const uint64_t *rng, const int32_t *timer,
                       const uint64_t *eff, const uint64_t *select, int trust_eff,
                       const int64_t *first_child, int64_t m,
                       int8_t *child_board, uint64_t *child_rng, int32_t *child_timer, uint64_t *child_eff,
                       int64_t *child_parent /* or NULL */, int32_t *child_action,
                       int32_t *child_reward, int32_t *child_n_new, int32_t *child_n_act, uint8_t *child_flags,
                       void *stream);

/* Step plans: one host call per batched step of a fixed set of buffers
 * (TileMatchEnv.step, tile_match_env.py:93-124, for every env of the batch),
 * with the batch split into env groups on their own streams, the callers'
 * per-step outputs written in the kernels' own write-back, and optionally
 * the examples' policy sampled inside the step.
 *
 * tmg_plan_create binds the state / output buffers (as for tmg_step) and
 * `groups` contiguous env groups: group g = envs [bounds[g], bounds[g+1])
 * (bounds[0] = 0, bounds[groups] = n), stepped on streams[g] (NULL: the
 * stream of each tmg_plan_step / tmg_plan_join call).  The plan keeps
 * the pointers; the caller keeps the buffers and streams alive until
 * tmg_plan_destroy. */
typedef struct tmg_plan tmg_plan;
TMG_API int tmg_plan_create(tmg_plan **out, tmg_ctx *ctx, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer,
                            int32_t *reward, int32_t *n_new, int32_t *n_act, uint8_t *flags, uint64_t *eff,
                            int groups, const int64_t *bounds, void *const *streams);

/* What each tmg_plan_step does (default: autoreset 1, no policy, no extra
 * outputs).
 *   autoreset: 0 none (as tmg_step's 0); 1 same step (as tmg_step's 1);
 *     2 next step (gymnasium.vector's default): an env whose episode ends is
 *     left as with 0 (terminated, all-zero mask), and the next call resets it
 *     (Board regenerated from its stream) instead of stepping it: its action
 *     is ignored, reward / n_new / n_act / flags 0 but TMG_FLAG_RESET.
 *   policy != 0: actions[] is an output: env i plays a uniform draw over its
 *     effective actions, exactly tmg_sample_effective(key, first_env + i, t)
 *     (src/examples/q_learning.py:19-25), drawn inside the step (the lean
 *     kernels) or by the sampler kernel enqueued right before it.
 *   onehot / onehot_dtype: fused OneHotWrapper planes, as tmg_step_onehot.
 *   terminated [n][4] bytes: terminated, is_combination_match, shuffled,
 *     error (0/1 each; the reference's step info, tile_match_env.py:102-112).
 *   action_mask [n][A] bytes: 0/1 of the effective-action bitmask (the
 *     reference's info["effective_actions"] as a mask), kept up to date: a
 *     call rewrites the rows whose mask changed.  The caller initialises it
 *     (e.g. after tmg_reset) from the bitmask.
 *   moves_left [n]: num_moves - timer after the call (tile_match_env.py:114-116).
 *   final_board [n][2][R][C]: with autoreset 1, the board each env whose
 *     episode ended had before its regeneration (rows of other envs untouched).
 *   board32 [n][2][R][C] int32: the boards in the reference's observation
 *     dtype (tile_match_env.py:52-77), kept up to date like action_mask
 *     (initialise it after a reset).
 *   A finished env with autoreset 0 (timer == num_moves, nothing regenerates
 *     it): the call that ends its episode writes terminated 1, moves_left 0
 *     and an all-zero action_mask row; every later call is a step after done
 *     (tile_match_env.py:94-95) and writes terminated {0, 0, 0, 1}, moves_left
 *     0, reward / n_new / n_act 0, leaves the mask row all zero and the state
 *     untouched, and raises TMG_STATUS_CALLER.  The policy draws such an
 *     env's action over all A actions, its mask being empty.
 * Any output pointer may be NULL (not written). */
TMG_API int tmg_plan_config(tmg_plan *plan, int autoreset, int policy, uint64_t key, int64_t first_env,
                            void *onehot, int onehot_dtype, uint8_t *terminated, uint8_t *action_mask,
                            int64_t *moves_left, int8_t *final_board, int32_t *board32);

/* One step of every env: with fork != 0 the group streams first wait for
 * the work queued on `stream` (an event; fork = 0 when nothing queued there
 * since the previous step is read by this one, e.g. back-to-back steps on
 * actions staged beforehand), then each group's launches are enqueued on its
 * stream.  Nothing waits for them: call tmg_plan_join before reading the
 * results on `stream`.  actions [n] (input, or the policy's output) must stay
 * valid until then.  t: the step counter of the policy draw.  trust_eff: as
 * tmg_step. */
TMG_API int tmg_plan_step(tmg_plan *plan, int32_t *actions, int32_t t, int trust_eff, int fork, void *stream);

/* `stream` waits for every group's queued work (events). */
TMG_API int tmg_plan_join(tmg_plan *plan, void *stream);
TMG_API int tmg_plan_destroy(tmg_plan *plan);

/* `steps` consecutive tmg_plan_step calls (step k: actions[k], t[k]; trust_eff
 * for the first, 1 after it) and the final tmg_plan_join, captured on
 * `stream` (a created stream, not NULL) into a HIP graph: tmg_graph_launch
 * then enqueues all of them on a stream with one call, the env groups'
 * launches still overlapping across the steps inside it.  Nothing runs at
 * capture time.  The graph keeps the plan's buffers, the action pointers and
 * the configuration of the moment; re-capture after tmg_plan_config. */
typedef struct tmg_graph tmg_graph;
TMG_API int tmg_plan_capture(tmg_plan *plan, int steps, int32_t *const *actions, const int32_t *t, int trust_eff,
                             void *stream, tmg_graph **out);
TMG_API int tmg_graph_launch(tmg_graph *graph, void *stream);
TMG_API int tmg_graph_destroy(tmg_graph *graph);

/* Replaces TileMatchEnv._get_effective_actions (tile_match_env.py:118-124,
 * is_move_effective board.py:735-787) as a bitmask, ignoring the timer. */
TMG_API int tmg_effective(tmg_ctx *ctx, int64_t n, const int8_t *board, uint64_t *eff, void *stream);

/* Output element types of tmg_onehot. */
#define TMG_DTYPE_F32 0
#define TMG_DTYPE_U8  1
#define TMG_DTYPE_I32 2

/* Replaces OneHotWrapper._one_hot_encode_board (src/tile_match_gym/wrappers.py:56-69)
 * for n boards: out[n][C_oh][R][C] with C_oh = tmg_onehot_channels(ctx) =
 * colours + #enabled specials.  Channel c < colours is (colour == c + 1); then
 * one channel per enabled special in the order cookie, v-laser, h-laser, bomb
 * (sorted(type id + 1), wrappers.py:39-46), set where the type equals it.
 * The reference builds float64; out_dtype picks f32 / u8 / i32 (TMG_DTYPE_*).
 * Asynchronous on `stream`. */
TMG_API int tmg_onehot(tmg_ctx *ctx, int64_t n, const int8_t *board, void *out, int out_dtype, void *stream);
TMG_API int tmg_onehot_channels(const tmg_ctx *ctx);

/* tmg_step / tmg_reset with the one-hot planes fused into the kernels' own
 * write-back (OneHotWrapper.observation, wrappers.py:50-69,
 * applied to every step's obs): `onehot` is out[n][C_oh][R][C] as for
 * tmg_onehot and must already hold the planes of the current boards (from a
 * tmg_reset_onehot or a tmg_onehot call); a step rewrites the planes of every
 * board it changes (any board when trust_eff == 0), tmg_reset_onehot those of
 * every board it generates.  onehot == NULL: plain tmg_step / tmg_reset. */
TMG_API int tmg_step_onehot(tmg_ctx *ctx, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer,
                            const int32_t *actions, int32_t *reward, int32_t *n_new, int32_t *n_act,
                            uint8_t *flags, uint64_t *eff, int trust_eff, int autoreset, void *onehot,
                            int onehot_dtype, void *stream);
TMG_API int tmg_reset_onehot(tmg_ctx *ctx, int64_t n, int8_t *board, uint64_t *rng, int32_t *timer,
                             uint64_t *eff, const uint8_t *env_mask, void *onehot, int onehot_dtype, void *stream);

/* The examples' policy over info["effective_actions"] (src/examples/q_learning.py:19-25,
 * qrdqn.py:58), on device: actions[i] uniform over env i's effective actions
 * (the ascending list of tile_match_env.py:118-124, read from the bitmask eff
 * [n][W]), picked by a counter-based draw of (key, first_env + i, t) — the
 * stream of the bench's synthetic actions, so shard layouts agree.  An env with
 * no effective action gets the uniform draw over all A actions.  Asynchronous
 * on `stream`. */
TMG_API int tmg_sample_effective(tmg_ctx *ctx, int64_t n, const uint64_t *eff, uint64_t key, int64_t first_env,
                                 int32_t t, int32_t *actions, void *stream);

/* Replaces the per-env np.random.default_rng(...) of TileMatchEnv.__init__ and
 * set_seed (tile_match_env.py:49, 79-82) for m streams at once, on the device:
 * rng[j] ([m][5], the layout above, half-word buffer empty) becomes the state
 * of PCG64(SeedSequence(...)) exactly as numpy seeds it.
 *   TMG_SEED_INT: row j is np.random.default_rng(seed_j).  seed_j is seeds[j]
 *     (seed_words == 1) or seeds[2j] | seeds[2j+1] << 64 (seed_words == 2), a
 *     device array; with seeds == NULL it is base + j, base = base_lo |
 *     base_hi << 64 (no array at all).  key0, key1 and period are not used.
 *   TMG_SEED_SPAWN: row j is np.random.default_rng(np.random.SeedSequence(base,
 *     spawn_key=key)) with key = (key0 + j,) for period == 0 — the j-th child
 *     of SeedSequence(base).spawn(m) when key0 == 0 — and key = (key0 + j /
 *     period, key1 + j % period) for period > 0: a (sample, global env) key
 *     with period = the shard's env count and key1 = its first env, so shard
 *     layouts agree.  seeds must be NULL.
 * seed_words must be 1 or 2 either way.  OR one of TMG_SEED_STORE_* into mode
 * to pick the kernel's store variant (diagnostic: the results are the same).
 * m == 0 is a no-op; any context serves (a tmg_create_scan one too: only its
 * device is used).  Refused: seed_words other than 1 or 2, a null rng,
 * m < 0 or m > 2^31, period < 0, an unknown mode, a key element or (range
 * form) a seed that would pass its width (2^64, 2^128) within the m rows.
 * Asynchronous on `stream`. */
#define TMG_SEED_INT   0
#define TMG_SEED_SPAWN 1
#define TMG_SEED_STORE_DIRECT 0x100   /* each lane stores its own row */
#define TMG_SEED_STORE_STAGED 0x200   /* rows staged in LDS, coalesced stores */
TMG_API int tmg_seed(tmg_ctx *ctx, int64_t m, int mode, const uint64_t *seeds, int seed_words,
                     uint64_t base_lo, uint64_t base_hi, uint64_t key0, uint64_t key1, int64_t period,
                     uint64_t *rng, void *stream);

/* Replaces utils.compute_num_states (src/tile_match_gym/utils/utils.py:6-26) on
 * `device`: over all colours^(rows*cols) colourings of an all-normal board,
 * num_line_free = boards with no colour line, num_playable = those that also
 * have an effective move (the reference's two returned sums, in the order
 * (playable, line_free)).  Needs rows*cols <= 16.  Synchronous. */
TMG_API int tmg_count_states(int device, int rows, int cols, int colours, uint64_t *num_playable,
                             uint64_t *num_line_free);

/* Sticky status of the context: the OR, over every env of every call since
 * the last clear, of TMG_STATUS_INTERNAL (a safety cap or an inconsistent
 * board ended a step with TMG_FLAG_ERROR), TMG_STATUS_OVERFLOW (not produced
 * since ABI 3) and TMG_STATUS_CALLER (a step after done / a bad action).
 * Waits for the device; clear != 0 then zeroes it.  The reference raises at
 * the point of failure (tile_match_env.py:94-95, board.py:349-350); a batch
 * reports through this word and the per-env flags instead. */
#define TMG_STATUS_INTERNAL 1u
#define TMG_STATUS_OVERFLOW 2u
#define TMG_STATUS_CALLER   4u
TMG_API int tmg_status(tmg_ctx *ctx, uint32_t *status, int clear);

/* Number of steps, since the context was created, whose cascade outgrew the
 * general kernels' LDS lists and was re-run on global-memory lists sized for
 * the worst case (spill_kernel; diagnostic — results are exact either way;
 * the queue of such steps is sized per stream for the largest launch).
 * Waits for the device. */
TMG_API int tmg_spills(tmg_ctx *ctx, uint64_t *count);

/* 1 when some rows x cols board with `colours` colours is line-free and has an
 * effective move, i.e. the reference's generate_board terminates
 * (board.py:102-109); tmg_create refuses the other shapes. */
TMG_API int tmg_viable(int rows, int cols, int colours);

/* Number of actions A = 2RC - R - C (tile_match_env.py:58) and mask words W. */
TMG_API int tmg_num_actions(const tmg_ctx *ctx);
TMG_API int tmg_mask_words(const tmg_ctx *ctx);

/* Message for the last failing call on this thread. */
TMG_API const char *tmg_last_error(void);

/* ABI version (bumped on any signature change). */
TMG_API int tmg_abi_version(void);

/* "src=<sha256 of the library's sources>;variant=<product|diagnostic name>":
 * the loader compares the hash with the sources next to the library and
 * refuses a stale build. */
TMG_API const char *tmg_build_info(void);

#ifdef __cplusplus
}
#endif

#endif /* TMG_H */
