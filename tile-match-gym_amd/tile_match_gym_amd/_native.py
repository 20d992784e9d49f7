"""ctypes binding of libtmg.so (include/tmg.h).

This is the reference-side binding a maintainer would add: the reference has
no FFI, so the binding replaces the Python Board calls of
tile_match_env.py:49-124 with the C entry points below.  There is no CPU
fallback: if the library or a HIP device is missing, every call raises.

Build provenance: the library carries the sha256 of the sources it was built
from (tmg_build_info); load() recomputes it from the sources in this tree and
refuses a stale library.  TMG_LIB selects another build (a diagnostic
variant, or an A/B library); its variant is reported by build_info().
"""
from __future__ import annotations

import ctypes
import hashlib
import os

from . import _buildinfo

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "_lib", "libtmg.so")
LIB_PATH = os.environ.get("TMG_LIB") or DEFAULT_LIB   # TMG_LIB: a diagnostic or A/B build
EXPORTS = ("tmg_create", "tmg_create_scan", "tmg_destroy", "tmg_reset", "tmg_step", "tmg_effective",
           "tmg_num_actions", "tmg_mask_words", "tmg_last_error", "tmg_abi_version", "tmg_build_info",
           "tmg_onehot", "tmg_onehot_channels", "tmg_count_states", "tmg_sample_effective", "tmg_status",
           "tmg_viable", "tmg_spills", "tmg_step_onehot", "tmg_reset_onehot", "tmg_plan_create", "tmg_plan_config",
           "tmg_plan_step", "tmg_plan_join", "tmg_plan_destroy", "tmg_plan_capture", "tmg_graph_launch",
           "tmg_graph_destroy", "tmg_peek", "tmg_rollout", "tmg_seed", "tmg_expand_count", "tmg_expand",
           "tmg_playout", "tmg_trace")
DTYPE_F32, DTYPE_U8, DTYPE_I32 = 0, 1, 2
ABI_VERSION = 10
SEED_INT, SEED_SPAWN, SEED_STORE_DIRECT, SEED_STORE_STAGED = 0, 1, 0x100, 0x200
STATUS_INTERNAL, STATUS_OVERFLOW, STATUS_CALLER = 1, 2, 4

# CV_* branch counters of TMG_COVER builds (tmg_board.hip), in index order
COVER_NAMES = ("sb_lean", "sb_normal", "sb_laser", "sb_perp_bomb", "sb_row_bomb", "sb_closure", "sb_fallback",
               "lds_normal", "lds_laser", "lds_bomb", "lds_fallback", "serial_step", "serial_act", "serial_cookie",
               "combo", "spill", "spill_run", "shuffle", "reject", "fast", "shuffle_gen", "reject_gen",
               "rp_passes", "rp_perp", "rp_vlong", "rp_wide", "rp_reject",
               "lane_step", "lane_shuffle", "lane_redraw", "lane_reject", "lane_reject_redraw",
               "rp_carry", "rp_rebatch", "peek_move", "peek_spill", "peek_spill_run",
               "roll_ply", "roll_horizon", "roll_spill", "roll_spill_run",
               "bp_pair_acc", "bp_pair_rej", "rp_vshift", "rp_vmore", "rp_scan2", "bp_round_carry", "rp_nolds",
               "plain_exit", "plain_step")

SPECIAL_BITS = {"cookie": 1, "vertical_laser": 2, "horizontal_laser": 4, "bomb": 8}
FLAG_DONE, FLAG_COMBO, FLAG_SHUFFLED, FLAG_RESET, FLAG_OVERFLOW, FLAG_ERROR = 1, 2, 4, 8, 0x40, 0x80
FLAG_STOPPED = 0x10                 # tmg_trace only
STAGE_SWAP, STAGE_COMBO, STAGE_CLEAR, STAGE_FALL, STAGE_REFILL, STAGE_SHUFFLE = 1, 2, 3, 4, 5, 6
STAGE_NAMES = {STAGE_SWAP: "swap", STAGE_COMBO: "combo", STAGE_CLEAR: "clear", STAGE_FALL: "fall",
               STAGE_REFILL: "refill", STAGE_SHUFFLE: "shuffle"}

_libs = {}          # loaded libraries by path
_M64 = (1 << 64) - 1

P = ctypes.c_void_p
I = ctypes.c_int
I64 = ctypes.c_int64
U64 = ctypes.c_uint64


class TmgError(RuntimeError):
    pass


def load(path: str = None):
    """Load libtmg.so — or the build at `path` (a diagnostic variant such as
    _lib/libtmg_cover.so, loaded beside the product library, each with its own
    kernels) — and check it against this tree's sources.  Raises TmgError when
    it was not built or is stale."""
    path = path or LIB_PATH
    L = _libs.get(path)
    if L is not None:
        return L
    if not os.path.exists(path):
        raise TmgError(f"{path} not found: build it with `make -C tile-match-gym_amd` "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(path)
    L.tmg_create.argtypes = [ctypes.POINTER(P), I, I, I, I, ctypes.c_uint32, I]
    L.tmg_create_scan.argtypes = [ctypes.POINTER(P), I, I, I]
    L.tmg_build_info.argtypes = []
    L.tmg_build_info.restype = ctypes.c_char_p
    L.tmg_destroy.argtypes = [P]
    L.tmg_reset.argtypes = [P, I64, P, P, P, P, P, P]
    L.tmg_step.argtypes = [P, I64, P, P, P, P, P, P, P, P, P, I, I, P]
    L.tmg_effective.argtypes = [P, I64, P, P, P]
    L.tmg_num_actions.argtypes = [P]
    L.tmg_mask_words.argtypes = [P]
    L.tmg_last_error.argtypes = []
    L.tmg_last_error.restype = ctypes.c_char_p
    L.tmg_abi_version.argtypes = []
    L.tmg_onehot.argtypes = [P, I64, P, P, I, P]
    L.tmg_onehot_channels.argtypes = [P]
    L.tmg_count_states.argtypes = [I, I, I, I, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.tmg_sample_effective.argtypes = [P, I64, P, ctypes.c_uint64, I64, ctypes.c_int32, P, P]
    L.tmg_status.argtypes = [P, ctypes.POINTER(ctypes.c_uint32), I]
    L.tmg_viable.argtypes = [I, I, I]
    L.tmg_spills.argtypes = [P, ctypes.POINTER(ctypes.c_uint64)]
    L.tmg_step_onehot.argtypes = [P, I64, P, P, P, P, P, P, P, P, P, I, I, P, I, P]
    L.tmg_reset_onehot.argtypes = [P, I64, P, P, P, P, P, P, I, P]
    L.tmg_plan_create.argtypes = [ctypes.POINTER(P), P, I64, P, P, P, P, P, P, P, P, I, P, P]
    L.tmg_plan_config.argtypes = [P, I, I, ctypes.c_uint64, I64, P, I, P, P, P, P, P]
    L.tmg_plan_step.argtypes = [P, P, ctypes.c_int32, I, I, P]
    L.tmg_plan_join.argtypes = [P, P]
    L.tmg_plan_destroy.argtypes = [P]
    L.tmg_plan_capture.argtypes = [P, I, P, P, I, P, ctypes.POINTER(P)]
    L.tmg_graph_launch.argtypes = [P, P]
    L.tmg_graph_destroy.argtypes = [P]
    L.tmg_peek.argtypes = [P, I64, P, P, P, I, P, P, P, P, P, P, P]
    L.tmg_rollout.argtypes = [P, I64, P, P, P, P, I, I, I, ctypes.c_uint64, I64, ctypes.c_int32, P, P, P, P, P, P, P]
    L.tmg_seed.argtypes = [P, I64, I, P, I, U64, U64, U64, U64, I64, P, P]
    L.tmg_expand_count.argtypes = [P, I64, P, P, P, P, P]
    L.tmg_expand.argtypes = [P, I64, P, P, P, P, P, I, P, I64] + [P] * 10 + [P]
    L.tmg_playout.argtypes = [P, I64, P, P, I, P, P, I, I, I, P] + [P] * 12 + [P]
    L.tmg_trace.argtypes = [P, I64, P, P, P, I, I, P, ctypes.c_uint32, I, I] + [P] * 9 + [P]
    for name in ("tmg_create", "tmg_create_scan", "tmg_destroy", "tmg_reset", "tmg_step", "tmg_effective",
                 "tmg_num_actions", "tmg_mask_words", "tmg_abi_version", "tmg_onehot", "tmg_onehot_channels",
                 "tmg_sample_effective", "tmg_status", "tmg_viable", "tmg_spills", "tmg_step_onehot", "tmg_reset_onehot",
                 "tmg_count_states", "tmg_plan_create", "tmg_plan_config", "tmg_plan_step", "tmg_plan_join",
                 "tmg_plan_destroy", "tmg_plan_capture", "tmg_graph_launch", "tmg_graph_destroy", "tmg_peek",
                 "tmg_rollout", "tmg_seed", "tmg_expand_count", "tmg_expand", "tmg_playout", "tmg_trace"):
        getattr(L, name).restype = I
    if L.tmg_abi_version() != ABI_VERSION:
        raise TmgError("libtmg.so ABI version mismatch; rebuild it")
    info = _parse_info(L.tmg_build_info().decode())
    want = _buildinfo.source_hash()
    if want is not None and info.get("src") != want:
        raise TmgError(f"{path} was built from other sources (src={info.get('src')}, tree={want}): "
                       "stale build, run `make -C tile-match-gym_amd -B`")
    if path == DEFAULT_LIB and info.get("variant") != "product":
        raise TmgError(f"{path} is a {info.get('variant')!r} build, not the product library")
    _libs[path] = L
    return L


def _parse_info(s: str) -> dict:
    return dict(kv.split("=", 1) for kv in s.split(";") if "=" in kv)


def build_info(path: str = None) -> dict:
    """{'src': sha256 of the sources built in, 'variant': ..., 'path': ..., 'so_sha256': ...}."""
    path = path or LIB_PATH
    L = load(path)
    info = _parse_info(L.tmg_build_info().decode())
    with open(path, "rb") as f:
        info["so_sha256"] = hashlib.sha256(f.read()).hexdigest()
    info["path"] = path
    return info


def check(rc: int, L=None):
    if rc != 0:
        msg = (L or load()).tmg_last_error().decode(errors="replace")
        raise TmgError(f"libtmg error {rc}: {msg}")


def specials_mask(colourless_specials, colour_specials) -> int:
    m = 0
    for name in list(colourless_specials) + list(colour_specials):
        if name not in SPECIAL_BITS:
            raise ValueError(f"unknown special {name!r}")
        m |= SPECIAL_BITS[name]
    return m


class Context:
    """Owns a tmg_ctx (shape / colours / specials / episode length on one device).
    scan_only=True: tmg_create_scan, a context for effective() on any shape."""

    def __init__(self, device_index: int, rows: int, cols: int, colours: int = 0, smask: int = 0,
                 num_moves: int = 1, scan_only: bool = False, lib_path: str = None):
        L = self._L = load(lib_path)
        h = P()
        if scan_only:
            check(L.tmg_create_scan(ctypes.byref(h), int(device_index), int(rows), int(cols)), L)
        else:
            check(L.tmg_create(ctypes.byref(h), int(device_index), int(rows), int(cols), int(colours),
                               int(smask), int(num_moves)), L)
        self._h = h
        self.num_actions = L.tmg_num_actions(h)
        self.mask_words = L.tmg_mask_words(h)

    def _check(self, rc: int):
        check(rc, self._L)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tmg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, n, board, rng, timer, eff, env_mask, stream, onehot=None, onehot_dtype=DTYPE_F32):
        """tmg_reset, or tmg_reset_onehot when a fused one-hot output pointer is given."""
        if onehot:
            self._check(self._L.tmg_reset_onehot(self._h, int(n), board, rng, timer, eff, env_mask, onehot,
                                          int(onehot_dtype), stream))
        else:
            self._check(self._L.tmg_reset(self._h, int(n), board, rng, timer, eff, env_mask, stream))

    def step(self, n, board, rng, timer, actions, reward, n_new, n_act, flags, eff, trust_eff, autoreset, stream,
             onehot=None, onehot_dtype=DTYPE_F32):
        """tmg_step, or tmg_step_onehot when a fused one-hot output pointer is given."""
        if onehot:
            self._check(self._L.tmg_step_onehot(self._h, int(n), board, rng, timer, actions, reward, n_new, n_act, flags,
                                         eff, int(trust_eff), int(autoreset), onehot, int(onehot_dtype), stream))
        else:
            self._check(self._L.tmg_step(self._h, int(n), board, rng, timer, actions, reward, n_new, n_act, flags, eff,
                                  int(trust_eff), int(autoreset), stream))

    def peek(self, n, board, rng, eff, trust_eff, reward, n_new, n_act, flags, best_action, best_reward, stream):
        """tmg_peek: every action's step outcome, [n][A] per output (any of them None), no state written."""
        self._check(self._L.tmg_peek(self._h, int(n), board, rng, eff, int(trust_eff), reward, n_new, n_act, flags,
                                     best_action, best_reward, stream))

    def rollout(self, n, board, rng, timer, eff, trust_eff, depth, samples, key, first_env, t, ret, plies, flags,
                total, best_action, best_total, stream):
        """tmg_rollout: every action's policy rollout, [samples][n][A] per rollout output, [n][A] / [n] for the
        sums over samples (any of them None; the sums need ret), no state written.  timer None: no horizon."""
        self._check(self._L.tmg_rollout(self._h, int(n), board, rng, timer, eff, int(trust_eff), int(depth),
                                        int(samples), int(key) % 2 ** 64, int(first_env), int(t), ret, plies, flags,
                                        total, best_action, best_total, stream))

    def expand_count(self, n, timer, eff, select, first_child, stream):
        """tmg_expand_count: first_child ([n + 1] int64, device) <- the exclusive prefix sum of every env's
        child count (its effective actions, of those in select ([n][W] words) when given; none for a
        finished env), first_child[n] the total.  No host round trip."""
        self._check(self._L.tmg_expand_count(self._h, int(n), timer, eff, select, first_child, stream))

    def expand(self, n, board, rng, timer, eff, select, trust_eff, first_child, m, child_board, child_rng,
               child_timer, child_eff, child_parent, child_action, child_reward, child_n_new, child_n_act,
               child_flags, stream):
        """tmg_expand: the m child rows first_child places, each what tmg_step(actions = a, autoreset = 0)
        leaves and reports on a copy of its parent env (child_parent may be None).  No input is written."""
        self._check(self._L.tmg_expand(self._h, int(n), board, rng, timer, eff, select, int(trust_eff), first_child,
                                       int(m), child_board, child_rng, child_timer, child_eff, child_parent,
                                       child_action, child_reward, child_n_new, child_n_act, child_flags, stream))

    def playout(self, n, board, rng, rng_per_seq, timer, eff, trust_eff, seqs, depth, actions, ret, n_new, n_act,
                plies, flags, ply_reward, out_board, out_rng, out_timer, out_eff, best_seq, best_ret, stream):
        """tmg_playout: the given action sequences ([seqs][n][depth] int32) played on copies of every env,
        [seqs][n] per output and per final-state array, [n] for best_seq / best_ret (any of them None; the
        best need ret, out_timer needs timer).  rng: [n][5], or [seqs][n][5] with rng_per_seq.  No input is
        written.  timer None: no horizon."""
        self._check(self._L.tmg_playout(self._h, int(n), board, rng, int(bool(rng_per_seq)), timer, eff,
                                        int(trust_eff), int(seqs), int(depth), actions, ret, n_new, n_act, plies,
                                        flags, ply_reward, out_board, out_rng, out_timer, out_eff, best_seq,
                                        best_ret, stream))

    def trace(self, n, board, rng, eff, trust_eff, seqs, actions, stage_mask, max_frames, stop, frames, kind,
              frame_elim, n_frames, reward, n_new, n_act, flags, out_rng, stream):
        """tmg_trace: Board.move(actions[q][i]) ([seqs][n] int32) on a copy of every env, stage by stage:
        the recorded stages' boards into frames ([seqs][n][max_frames][2][R][C] int8), kinds and
        eliminations into kind / frame_elim ([seqs][n][max_frames]), [seqs][n] per count, sum and flag,
        out_rng [seqs][n][5] (any of them None).  No input is written."""
        self._check(self._L.tmg_trace(self._h, int(n), board, rng, eff, int(trust_eff), int(seqs), actions,
                                      int(stage_mask), int(max_frames), int(bool(stop)), frames, kind, frame_elim,
                                      n_frames, reward, n_new, n_act, flags, out_rng, stream))

    def seed(self, m, rng, stream, mode=SEED_INT, seeds=None, seed_words=1, base=0, key0=0, key1=0, period=0):
        """tmg_seed: the PCG64 words of m streams into rng ([m][5] uint64), seeded on the device as numpy
        seeds them.  SEED_INT: default_rng(seed_j), seed_j from the device array `seeds` ([m] uint64, or
        [m][2] lo / hi with seed_words=2) or, with seeds None, base + j.  SEED_SPAWN:
        default_rng(SeedSequence(base, spawn_key=(key0 + j,))) or, with period > 0, spawn_key=(key0 + j //
        period, key1 + j % period).  base: a non-negative int below 2^128."""
        base = int(base)
        if not 0 <= base < 1 << 128:
            raise ValueError("base must be in [0, 2^128)")
        key0, key1 = int(key0), int(key1)
        if not (0 <= key0 < 1 << 64 and 0 <= key1 < 1 << 64):
            raise ValueError("spawn key elements must be in [0, 2^64)")
        self._check(self._L.tmg_seed(self._h, int(m), int(mode), seeds, int(seed_words), base & _M64, base >> 64,
                                     key0, key1, int(period), rng, stream))

    def status(self, clear: bool = False) -> int:
        """Sticky STATUS_* bits of this context (waits for the device)."""
        v = ctypes.c_uint32(0)
        self._check(self._L.tmg_status(self._h, ctypes.byref(v), int(clear)))
        return int(v.value)

    def spills(self) -> int:
        """Steps re-run on the worst-case global-memory lists so far (tmg_spills; waits for the device)."""
        v = ctypes.c_uint64(0)
        self._check(self._L.tmg_spills(self._h, ctypes.byref(v)))
        return int(v.value)

    def effective(self, n, board, eff, stream):
        self._check(self._L.tmg_effective(self._h, int(n), board, eff, stream))

    def onehot_channels(self) -> int:
        return self._L.tmg_onehot_channels(self._h)

    def onehot(self, n, board, out, out_dtype, stream):
        self._check(self._L.tmg_onehot(self._h, int(n), board, out, int(out_dtype), stream))

    def cover(self, clear: bool = False):
        """CV_* branch hit counters (diagnostic TMG_COVER builds only: tmg_debug_cover)."""
        L = self._L
        fn = getattr(L, "tmg_debug_cover", None)
        if fn is None:
            raise TmgError("this context's library is not a TMG_COVER build")
        import numpy as np
        out = np.zeros(len(COVER_NAMES), np.uint64)
        fn.argtypes = [P, P, I, I]
        fn.restype = I
        check(fn(self._h, out.ctypes.data, out.size, int(clear)), L)
        return out

    def sample_effective(self, n, eff, key, first_env, t, actions, stream):
        self._check(self._L.tmg_sample_effective(self._h, int(n), eff, int(key) & 0xFFFFFFFFFFFFFFFF, int(first_env),
                                          int(t), actions, stream))


class Plan:
    """A tmg_plan: one host call per batched step of fixed buffers over env
    groups on their own streams (include/tmg.h).  `bufs`: the state / output
    tensors (board, rng, timer, reward, n_new, n_act, flags, eff); `bounds`:
    group g = envs [bounds[g], bounds[g+1]); `streams`: raw hipStream_t per
    group.  The caller keeps the buffers and streams alive."""

    AUTORESET = {"none": 0, "same_step": 1, "next_step": 2}

    def __init__(self, ctx: "Context", n, board, rng, timer, reward, n_new, n_act, flags, eff, bounds, streams):
        L = self._L = ctx._L
        self._ctx = ctx                      # the context outlives the plan
        G = len(streams)
        self._bounds = (ctypes.c_int64 * (G + 1))(*[int(b) for b in bounds])
        self._streams = (P * G)(*[int(x) for x in streams])
        h = P()
        check(L.tmg_plan_create(ctypes.byref(h), ctx.handle, int(n), board, rng, timer, reward, n_new, n_act, flags,
                                eff, G, self._bounds, self._streams), L)
        self._h = h
        self._step = L.tmg_plan_step
        self._join = L.tmg_plan_join

    def config(self, autoreset="same_step", policy=False, key=0, first_env=0, onehot=None, onehot_dtype=DTYPE_F32,
               terminated=None, action_mask=None, moves_left=None, final_board=None, board32=None):
        check(self._L.tmg_plan_config(self._h, self.AUTORESET[autoreset], int(bool(policy)),
                                      int(key) & 0xFFFFFFFFFFFFFFFF, int(first_env), onehot, int(onehot_dtype),
                                      terminated, action_mask, moves_left, final_board, board32), self._L)

    def step(self, actions_ptr: int, t: int, trust_eff: int, stream: int, fork: int = 1):
        rc = self._step(self._h, actions_ptr, t, trust_eff, fork, stream)
        if rc:
            check(rc, self._L)

    def join(self, stream: int):
        rc = self._join(self._h, stream)
        if rc:
            check(rc, self._L)

    def capture(self, actions_ptrs, ts, trust_eff: int, stream: int) -> "StepGraph":
        """len(actions_ptrs) steps + the join, captured into a HIP graph (tmg_plan_capture)."""
        k = len(actions_ptrs)
        a = (P * k)(*[int(x) for x in actions_ptrs])
        t = (ctypes.c_int32 * k)(*[int(x) for x in ts])
        h = P()
        check(self._L.tmg_plan_capture(self._h, k, a, t, int(trust_eff), stream, ctypes.byref(h)), self._L)
        return StepGraph(self, h, k)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tmg_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StepGraph:
    """A captured run of plan steps (tmg_graph): launch() enqueues them all."""

    def __init__(self, plan: Plan, h, steps: int):
        self._plan, self._h, self.steps = plan, h, steps
        self._L = plan._L

    def launch(self, stream: int):
        rc = self._L.tmg_graph_launch(self._h, stream)
        if rc:
            check(rc, self._L)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tmg_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_SCAN_CTX = {}


def scan_context(device_index: int, rows: int, cols: int) -> "Context":
    """One cached tmg_create_scan context per (device, rows, cols)."""
    key = (int(device_index), int(rows), int(cols))
    c = _SCAN_CTX.get(key)
    if c is None:
        c = _SCAN_CTX[key] = Context(key[0], key[1], key[2], scan_only=True)
    return c


def viable(rows: int, cols: int, colours: int) -> bool:
    """Whether a line-free playable board exists (tmg_viable; tmg_create refuses the others)."""
    return bool(load().tmg_viable(int(rows), int(cols), int(colours)))


def count_states(device_index: int, rows: int, cols: int, colours: int):
    """(num_playable, num_line_free) over all colourings (tmg_count_states)."""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().tmg_count_states(int(device_index), int(rows), int(cols), int(colours), ctypes.byref(a),
                                  ctypes.byref(b)))
    return int(a.value), int(b.value)
