"""ctypes driver of the host wave emulator (debug/test tool, not the product).

    LD_PRELOAD=$(gcc -print-file-name=libasan.so) ASAN_OPTIONS=detect_leaks=0 \
        python tools/wave_emu/emu.py --asan R C k smask n steps
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
P = ctypes.c_void_p
I = ctypes.c_int
I64 = ctypes.c_int64


def load(asan=False):
    L = ctypes.CDLL(os.path.join(HERE, "libwave_emu_asan.so" if asan else os.environ.get("EMU_LIB", "libwave_emu.so")))
    L.emu_step.argtypes = [I, I, I, I, I, I64, P, P, P, P, P, P, P, P, P, I, I, I, ctypes.c_uint64, I64, ctypes.c_int32,
                           P, P, P, P, P]
    L.emu_reset.argtypes = [I, I, I, I, I, I64, P, P, P, P]
    L.emu_reset_masked.argtypes = [I, I, I, I, I, I64, P, P, P, P, P, I]
    L.emu_effective.argtypes = [I, I, I, I, I64, P, P]
    L.emu_spills.restype = ctypes.c_ulonglong
    L.emu_status.restype = ctypes.c_uint
    L.emu_status_clear.restype = ctypes.c_uint
    L.emu_cover.argtypes = [P, I]
    L.emu_cover.restype = None
    L.emu_route.argtypes = [I, I, I, I, I, I, I64, I, I, I, P, P]
    L.emu_peek.argtypes = [I, I, I, I, I64, P, P, P, I, P, P, P, P, P, P]
    L.emu_peek_route.argtypes = [I, I, I, I, I, P]
    L.emu_rollout.argtypes = [I, I, I, I, I, I64, P, P, P, P, I, I, I, ctypes.c_uint64, I64, ctypes.c_int32,
                              P, P, P, P, P, P]
    L.emu_playout.argtypes = [I, I, I, I, I, I64, P, P, I, P, P, I, I, I, P] + [P] * 12
    L.emu_trace.argtypes = [I, I, I, I, I64, P, P, P, I, I, P, ctypes.c_uint32, I, I] + [P] * 9
    L.emu_expand_count.argtypes = [I, I, I, I64, P, P, P, P]
    L.emu_expand.argtypes = [I, I, I, I, I, I64, P, P, P, P, P, I, P, I64] + [P] * 10 + [I]
    U64 = ctypes.c_uint64
    L.emu_seed.argtypes = [I64, I, P, I, U64, U64, U64, U64, I64, P]
    return L


STEP_ROUTE = ("MAXN", "GEN", "NB", "CODD", "FIX", "lean", "lane", "deferred", "kernel_autoreset", "spill", "reset_epw",
              "plain")
RESET_ROUTE = ("MAXN", "NB", "CODD", "FIX", "epw_full", "epw_masked")
FUSED = ("onehot", "terminated", "action_mask", "moves_left", "final_board", "board32")


def route(L, R, C, k, smask, trust_eff=1, mode=1, n=1024, have_lane=False, policy=False, fused=()):
    """What the dispatch rule (csrc/tmg_dispatch.h) picks for one step and one
    reset, as two dicts keyed by STEP_ROUTE / RESET_ROUTE; nothing is run.
    The step's instantiation fields are 0 when the lane kernel takes it.
    fused: the names (of FUSED) of the fused outputs asked for."""
    step = np.zeros(len(STEP_ROUTE), np.int32)
    reset = np.zeros(len(RESET_ROUTE), np.int32)
    bits = sum(1 << FUSED.index(f) for f in fused)
    L.emu_route(R, C, k, smask, int(trust_eff), int(mode), int(n), int(have_lane), int(policy), bits,
                step.ctypes.data, reset.ctypes.data)
    return dict(zip(STEP_ROUTE, step.tolist())), dict(zip(RESET_ROUTE, reset.tolist()))


PEEK_ROUTE = ("MAXN", "GEN", "NB", "CODD")


def peek_route(L, R, C, k, smask, trust_eff=1):
    """The peek kernel instantiation the rule picks (peek_ladder), keyed by PEEK_ROUTE; nothing is run."""
    out = np.zeros(len(PEEK_ROUTE), np.int32)
    L.emu_peek_route(R, C, k, smask, int(trust_eff), out.ctypes.data)
    return dict(zip(PEEK_ROUTE, out.tolist()))


def peek(L, R, C, k, smask, board, rng, eff=None, trust_eff=1):
    """tmg_peek on the emulated kernels: dict of reward / n_new / n_act (n, A)
    int32, flags (n, A) uint8, best_action / best_reward (n,) int32.  The
    inputs are only read; eff may be None when trust_eff == 0."""
    n = board.shape[0]
    A = 2 * R * C - R - C
    board = np.ascontiguousarray(board, dtype=np.int8)
    rng = np.ascontiguousarray(rng, dtype=np.uint64)
    if eff is not None:
        eff = np.ascontiguousarray(eff, dtype=np.uint64)
    out = {name: np.full((n, A), -1, np.int32) for name in ("reward", "n_new", "n_act")}
    out["flags"] = np.full((n, A), 0x55, np.uint8)
    out["best_action"] = np.full(n, -1, np.int32)
    out["best_reward"] = np.full(n, -1, np.int32)
    L.emu_peek(R, C, k, smask, n, board.ctypes.data, rng.ctypes.data, eff.ctypes.data if eff is not None else None,
               int(trust_eff), out["reward"].ctypes.data, out["n_new"].ctypes.data, out["n_act"].ctypes.data,
               out["flags"].ctypes.data, out["best_action"].ctypes.data, out["best_reward"].ctypes.data)
    return out


def rollout(L, R, C, k, smask, num_moves, board, rng, timer, eff, trust_eff, depth, samples, key, first_env, t):
    """tmg_rollout on the emulated kernels: dict of ret / plies (S, n, A) int32,
    flags (S, n, A) uint8, total (n, A), best_action / best_total (n,) int32.
    rng: (S, n, 5) uint64 ((n, 5) for S = 1).  The inputs are only read; timer
    None is no horizon; eff may be None when trust_eff == 0."""
    n = board.shape[0]
    A = 2 * R * C - R - C
    board = np.ascontiguousarray(board, dtype=np.int8)
    rng = np.ascontiguousarray(rng, dtype=np.uint64)
    assert rng.size == samples * n * 5
    if timer is not None:
        timer = np.ascontiguousarray(timer, dtype=np.int32)
    if eff is not None:
        eff = np.ascontiguousarray(eff, dtype=np.uint64)
    out = {name: np.full((samples, n, A), -1, np.int32) for name in ("ret", "plies")}
    out["flags"] = np.full((samples, n, A), 0x55, np.uint8)
    out["total"] = np.full((n, A), -1, np.int32)
    out["best_action"] = np.full(n, -1, np.int32)
    out["best_total"] = np.full(n, -1, np.int32)
    rc = L.emu_rollout(R, C, k, smask, int(num_moves), n, board.ctypes.data, rng.ctypes.data,
                       timer.ctypes.data if timer is not None else None, eff.ctypes.data if eff is not None else None,
                       int(trust_eff), int(depth), int(samples), int(key) % 2 ** 64, int(first_env), int(t),
                       *(out[f].ctypes.data for f in ("ret", "plies", "flags", "total", "best_action", "best_total")))
    if rc:
        raise ValueError(f"emu_rollout refused the call ({rc})")
    return out


def _opt(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _addr(a):
    return None if a is None else a.ctypes.data


PLAYOUT_FIELDS = ("ret", "n_new", "n_act", "plies", "flags", "ply_reward", "out_board", "out_rng", "out_timer",
                  "out_eff", "best_seq", "best_ret")


def playout(L, R, C, k, smask, num_moves, board, rng, timer, eff, trust_eff, actions, fields=PLAYOUT_FIELDS, out=None):
    """tmg_playout on the emulated kernels: dict of the requested PLAYOUT_FIELDS
    (ret / n_new / n_act / plies (Q, n) int32, flags (Q, n) uint8, ply_reward
    (Q, n, D) int32, out_board (Q * n, 2, R, C) int8, out_rng (Q * n, 5) /
    out_eff (Q * n, W) uint64, out_timer (Q * n,) int32, best_seq / best_ret
    (n,) int32), freshly allocated with a sentinel fill, or the arrays of `out`
    (a dict by field name).  actions: (Q, n, D) int32; rng: (n, 5) uint64, or
    (Q, n, 5) for words per sequence.  The inputs are only read; timer None
    is no horizon; eff may be None when trust_eff == 0.  A refused call
    raises ValueError with the return code."""
    n = board.shape[0]
    A = 2 * R * C - R - C
    W = (A + 63) // 64
    actions = np.ascontiguousarray(actions, dtype=np.int32)
    Q, _, D = actions.shape
    assert actions.shape[1] == n
    board = np.ascontiguousarray(board, dtype=np.int8)
    rng = np.ascontiguousarray(rng, dtype=np.uint64)
    assert rng.size in (n * 5, Q * n * 5)
    per_seq = rng.ndim == 3
    timer = _opt(timer, np.int32)
    eff = _opt(eff, np.uint64)
    if out is None:
        m = Q * n
        new = {"ply_reward": np.full((Q, n, D), -7, np.int32), "flags": np.full((Q, n), 0x55, np.uint8),
               "out_board": np.full((m, 2, R, C), -7, np.int8), "out_rng": np.full((m, 5), 0xA5A5A5A5A5A5A5A5, np.uint64),
               "out_eff": np.full((m, W), 0xA5A5A5A5A5A5A5A5, np.uint64), "out_timer": np.full(m, -7, np.int32),
               "best_seq": np.full(n, -7, np.int32), "best_ret": np.full(n, -7, np.int32)}
        new.update({f: np.full((Q, n), -7, np.int32) for f in ("ret", "n_new", "n_act", "plies")})
        out = {f: new[f] for f in fields}
    rc = L.emu_playout(R, C, k, smask, int(num_moves), n, _addr(board), _addr(rng), int(per_seq), _addr(timer),
                       _addr(eff), int(trust_eff), Q, D, _addr(actions), *(_addr(out.get(f)) for f in PLAYOUT_FIELDS))
    if rc:
        raise ValueError(f"emu_playout refused the call ({rc})")
    return out


TRACE_FIELDS = ("frames", "kind", "frame_elim", "n_frames", "reward", "n_new", "n_act", "flags", "out_rng")


def trace(L, R, C, k, smask, board, rng, eff, trust_eff, actions, stage_mask, max_frames, stop=0, fields=TRACE_FIELDS,
          out=None):
    """tmg_trace on the emulated kernels: dict of the requested TRACE_FIELDS
    (frames (Q, n, F, 2, R, C) int8, kind (Q, n, F) uint8, frame_elim (Q, n, F)
    int32, n_frames / reward / n_new / n_act (Q, n) int32, flags (Q, n) uint8,
    out_rng (Q, n, 5) uint64), freshly allocated with a sentinel fill, or the
    arrays of `out` (a dict by field name).  actions: (Q, n) int32.  The inputs
    are only read; eff may be None when trust_eff == 0.  A refused call raises
    ValueError with the return code."""
    n = board.shape[0]
    actions = np.ascontiguousarray(actions, dtype=np.int32)
    Q = actions.shape[0]
    assert actions.shape == (Q, n)
    board = np.ascontiguousarray(board, dtype=np.int8)
    rng = np.ascontiguousarray(rng, dtype=np.uint64)
    assert rng.size == n * 5
    eff = _opt(eff, np.uint64)
    F = int(max_frames)
    if out is None:
        new = {"frames": np.full((Q, n, max(F, 0), 2, R, C), -7, np.int8), "kind": np.full((Q, n, max(F, 0)), 0x55, np.uint8),
               "frame_elim": np.full((Q, n, max(F, 0)), -7, np.int32), "flags": np.full((Q, n), 0x55, np.uint8),
               "out_rng": np.full((Q, n, 5), 0xA5A5A5A5A5A5A5A5, np.uint64)}
        new.update({f: np.full((Q, n), -7, np.int32) for f in ("n_frames", "reward", "n_new", "n_act")})
        out = {f: new[f] for f in fields}
    rc = L.emu_trace(R, C, k, smask, n, _addr(board), _addr(rng), _addr(eff), int(trust_eff), Q, _addr(actions),
                     int(stage_mask), F, int(stop), *(_addr(out.get(f)) for f in TRACE_FIELDS))
    if rc:
        raise ValueError(f"emu_trace refused the call ({rc})")
    return out


def expand_count(L, R, C, num_moves, timer, eff, select=None):
    """tmg_expand_count on the emulated kernels: the (n + 1,) int64 first_child
    array of n envs.  eff / select: (n, W) uint64 mask words (select None: every
    effective action); timer: (n,) int32.  The inputs are only read."""
    timer = np.ascontiguousarray(timer, dtype=np.int32)
    n = timer.shape[0]
    eff = np.ascontiguousarray(eff, dtype=np.uint64)
    select = _opt(select, np.uint64)
    out = np.full(n + 1, -7, np.int64)
    rc = L.emu_expand_count(R, C, int(num_moves), n, _addr(timer), _addr(eff), _addr(select), out.ctypes.data)
    if rc:
        raise ValueError(f"emu_expand_count refused the call ({rc})")
    return out


EXPAND_FIELDS = ("board", "rng", "timer", "eff", "parent", "action", "reward", "n_new", "n_act", "flags")


def expand(L, R, C, k, smask, num_moves, board, rng, timer, eff, select=None, trust_eff=1, m=None, pack=-1):
    """tmg_expand_count + tmg_expand on the emulated kernels, the moves by
    emu_step on the child rows: dict of first_child (n + 1,) int64 and, per
    child row, EXPAND_FIELDS (board (m, 2, R, C) int8, rng (m, 5) / eff (m, W)
    uint64, timer / action / reward / n_new / n_act int32, parent int64, flags
    uint8).  m None: first_child[n] rows; rows nothing writes keep a sentinel
    fill (board -7, rng / eff 0xA5..., the rest -7 / 0x55).  pack: the gather's
    store variant (-1: the library's).  The inputs are only read."""
    n = board.shape[0]
    A = 2 * R * C - R - C
    W = (A + 63) // 64
    board = np.ascontiguousarray(board, dtype=np.int8)
    rng = np.ascontiguousarray(rng, dtype=np.uint64)
    timer = np.ascontiguousarray(timer, dtype=np.int32)
    eff = np.ascontiguousarray(eff, dtype=np.uint64)
    select = _opt(select, np.uint64)
    first = expand_count(L, R, C, num_moves, timer, eff, select)
    m = int(first[n]) if m is None else int(m)
    out = {"board": np.full((m, 2, R, C), -7, np.int8), "rng": np.full((m, 5), 0xA5A5A5A5A5A5A5A5, np.uint64),
           "timer": np.full(m, -7, np.int32), "eff": np.full((m, W), 0xA5A5A5A5A5A5A5A5, np.uint64),
           "parent": np.full(m, -7, np.int64), "action": np.full(m, -7, np.int32)}
    out.update({f: np.full(m, -7, np.int32) for f in ("reward", "n_new", "n_act")})
    out["flags"] = np.full(m, 0x55, np.uint8)
    rc = L.emu_expand(R, C, k, smask, int(num_moves), n, _addr(board), _addr(rng), _addr(timer), _addr(eff),
                      _addr(select), int(trust_eff), first.ctypes.data, m, *(out[f].ctypes.data for f in EXPAND_FIELDS),
                      int(pack))
    if rc:
        raise ValueError(f"emu_expand refused the call ({rc})")
    out["first_child"] = first
    return out


SEED_INT, SEED_SPAWN = 0, 1


def seed(L, m, mode=SEED_INT, seeds=None, seed_words=1, base=0, key0=0, key1=0, period=0):
    """tmg_seed through the emulator's host loop over csrc/tmg_seed.h: the (m, 5)
    uint64 PCG64 words.  seeds: None (the range / spawn forms) or a uint64
    array of m * seed_words words; base: an int below 2^128.  A refused call
    raises ValueError with the return code."""
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.size == m * seed_words
    out = np.full((max(int(m), 0), 5), 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = L.emu_seed(int(m), int(mode), seeds.ctypes.data if seeds is not None else None, int(seed_words),
                    int(base) & (2 ** 64 - 1), int(base) >> 64, int(key0), int(key1), int(period), out.ctypes.data)
    if rc:
        raise ValueError(f"emu_seed refused the call ({rc})")
    return out


def cover(L, clear=False):
    """The CV_* branch counters of the emulated kernels (the emulator is built with TMG_COVER)."""
    out = np.zeros(L.emu_cover_count(), np.uint64)
    L.emu_cover(out.ctypes.data, int(clear))
    return out


class EmuBatch:
    """Same fields/semantics as oracle.OracleBatch, executed by the emulated kernels."""

    def __init__(self, L, R, C, k, smask, num_moves, rng_words):
        self.L = L
        self.R, self.C, self.k, self.smask, self.num_moves = R, C, k, smask, num_moves
        self.n = rng_words.shape[0]
        self.A = 2 * R * C - R - C
        self.W = (self.A + 63) // 64
        self.board = np.zeros((self.n, 2, R, C), np.int8)
        self.rng = np.ascontiguousarray(rng_words, dtype=np.uint64).copy()
        self.timer = np.zeros(self.n, np.int32)
        self.eff = np.zeros((self.n, self.W), np.uint64)
        self.reward = np.zeros(self.n, np.int32)
        self.n_new = np.zeros(self.n, np.int32)
        self.n_act = np.zeros(self.n, np.int32)
        self.flags = np.zeros(self.n, np.uint8)
        self.trust = False

    def reset(self, mask=None):
        """reset(); with a uint8 mask, only the envs whose mask byte is non-zero (reset(env_mask=...))."""
        if mask is None:
            self.L.emu_reset(self.R, self.C, self.k, self.smask, self.num_moves, self.n, self.board.ctypes.data,
                             self.rng.ctypes.data, self.timer.ctypes.data, self.eff.ctypes.data)
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            self.L.emu_reset_masked(self.R, self.C, self.k, self.smask, self.num_moves, self.n,
                                    self.board.ctypes.data, self.rng.ctypes.data, self.timer.ctypes.data,
                                    self.eff.ctypes.data, m.ctypes.data, 0xFF)
        self.trust = True

    def step(self, actions, autoreset=True, mode=None, policy=None, outputs=None):
        """mode: 0 none / 1 same step / 2 next step (tmg_plan_config; default from
        autoreset); policy = (key, first_env, t): actions is then the output
        array of the in-kernel draw; outputs: dict of numpy arrays terminated
        (n, 4) u8, action_mask (n, A) u8, moves_left (n,) i64, final_board, board32."""
        a = actions if policy is not None else np.ascontiguousarray(actions, dtype=np.int32)
        mode = (1 if autoreset else 0) if mode is None else mode
        key, first, t = policy if policy is not None else (0, 0, 0)
        o = outputs or {}
        ptr = lambda name: o[name].ctypes.data if name in o else None   # noqa: E731
        self.L.emu_step(self.R, self.C, self.k, self.smask, self.num_moves, self.n, self.board.ctypes.data,
                        self.rng.ctypes.data, self.timer.ctypes.data, a.ctypes.data, self.reward.ctypes.data,
                        self.n_new.ctypes.data, self.n_act.ctypes.data, self.flags.ctypes.data,
                        self.eff.ctypes.data, int(self.trust), int(mode), int(policy is not None), int(key), int(first),
                        int(t), ptr("terminated"), ptr("action_mask"), ptr("moves_left"), ptr("final_board"),
                        ptr("board32"))


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tile-match-gym_amd")]
    from oracle import oracle as orc
    from tile_match_gym_amd.seeding import batch_rng_words
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    R, C, k, sm, n, steps = (int(x) for x in args)
    L = load(asan="--asan" in sys.argv)
    w = batch_rng_words(range(100, 100 + n))
    e = EmuBatch(L, R, C, k, sm, 30, w)
    o = orc.OracleBatch(R, C, k, sm, 30, w)
    e.reset(); o.reset()
    assert np.array_equal(e.board, o.board), "reset board"
    assert np.array_equal(e.rng, o.rng), "reset rng"
    assert np.array_equal(e.eff, o.eff), "reset eff"
    rs = np.random.default_rng(7)
    for t in range(steps):
        a = rs.integers(0, e.A, n).astype(np.int32)
        e.step(a); o.step(a)
        for name in ("board", "rng", "reward", "n_new", "n_act", "flags", "eff", "timer"):
            if not np.array_equal(getattr(e, name), getattr(o, name)):
                bad = np.nonzero((getattr(e, name).reshape(n, -1) != getattr(o, name).reshape(n, -1)).any(1))[0]
                raise SystemExit(f"step {t}: {name} differs in envs {bad[:10]}")
    print(f"emu == oracle for {n} envs x {steps} steps ({R}x{C} k={k} smask={sm})")


if __name__ == "__main__":
    main()
