"""The fused step outputs of tmg_plan_config (terminated / info bytes, action-mask
bytes, moves left, same-step final boards, int32 boards, one-hot planes) on
every step_kernel / reset_kernel instantiation: the shapes, the schedule and
the comparisons shared by tests/test_fused_emulated.py (the host wave
emulator) and tests/test_gpu_fused.py (the device); the census of
tests/test_dispatch_route.py routes SHAPES and fails when a row that is the
only cover of an instantiation is deleted.

Each backend plays one schedule (drive): short episodes with staggered
timers, so every step ends some; effective and uniform actions in turn, two
steps of the in-kernel policy, two untrusted steps after a hand edit; and
after every step every output is compared over all of its rows with the
oracle driven with the same autoreset semantics (tests/vector_ref.py)."""
import numpy as np

import dispatch_cases as dc
from vector_ref import VectorOracle, mask_bytes

# (R, C, k, smask)
SPECIALISED = [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)]    # the c2 / c3 / c5 kernels
EXTRA = [
    (4, 4, 2, 0),       # lean, 1 plane, even C: <128,0,1,0>
    (9, 15, 15, 0),     # lean 512-cell board of 4 planes: the deferred reset<512,4>
]
# A % 64 == 0: the mask's last word is full, action A - 1 sits in bit 63
FULL_WORD_MASKS = [(2, 22, 4, 0), (2, 22, 4, 15), (3, 39, 5, 0)]    # A = 64, 64, 192
SHAPES = dc.CASES + [dc.ROW_PLANE_CONTROL] + SPECIALISED + EXTRA + FULL_WORD_MASKS

MODES = ("none", "same_step", "next_step")
MODE_CODE = {"none": 0, "same_step": 1, "next_step": 2}            # tmg_plan_config's autoreset
STATUS_CALLER = 4                                                   # TMG_STATUS_CALLER

M = 4                       # moves per episode
STEPS = 3 * M + 2
POLICY_STEPS = (2, 10)      # even steps played by the in-kernel policy
EDIT_STEPS = (5, 6)         # a hand edit before each: these run untrusted
POLICY_KEY, POLICY_FIRST = 4242, 1000
FINAL_FILL = 0x55

# boards the oracle generates slowly (a line-free one is rare), and the 512-cell family
SLOW = {(4, 29, 4, 0), (2, 64, 4, 0), (2, 64, 4, 15), (12, 12, 4, 0)}

SPILL_SHAPES = [(10, 10, 4, 14), (20, 20, 6, 15)]
SPILL_BOARDS = ("laser_sea", "cookie_field", "combo_grid")          # adversarial.MODES whose boards all spill
SPILL_M = 6
SPILL_TIMERS = ("last_move", "first_move")      # every timer at M - 1 (each spilled step ends its episode) / at 0


def case_id(s):
    return "{}x{}k{}s{}".format(*s)


def num_actions(R, C):
    return 2 * R * C - R - C


def onehot_np(board, k, sm):
    """The one-hot planes of (n, 2, R, C) boards by the channel rule of
    include/tmg.h (tmg_onehot): colours 1..k, then one channel per enabled
    special in the order cookie, v-laser, h-laser, bomb (type ids -1, 2, 3, 4)."""
    ids = [t for bit, t in ((1, -1), (2, 2), (4, 3), (8, 4)) if sm & bit]
    chans = [board[:, 0] == c for c in range(1, k + 1)] + [board[:, 1] == t for t in ids]
    return np.stack(chans, axis=1).astype(np.float32)


def fresh_outputs(state, moves, junk=False):
    """Host arrays for the five outputs: as vector.py initialises them after a
    reset (from the boards, masks and timers of `state`), or junk in every row
    that a step has to overwrite.  final_board is FINAL_FILL either way."""
    board, eff, timer = state["board"], state["eff"], state["timer"]
    n, _, R, C = board.shape
    A = num_actions(R, C)
    out = {"final_board": np.full((n, 2, R, C), FINAL_FILL, np.int8)}
    if junk:
        out.update(terminated=np.full((n, 4), 9, np.uint8), action_mask=np.full((n, A), 7, np.uint8),
                   moves_left=np.full(n, -1, np.int64), board32=np.full((n, 2, R, C), -9, np.int32))
    else:
        out.update(terminated=np.zeros((n, 4), np.uint8), action_mask=mask_bytes(eff, A),
                   moves_left=(moves - timer).astype(np.int64), board32=board.astype(np.int32))
    return out


class EmuBackend:
    """emu.EmuBatch with the outputs attached as numpy arrays."""

    def __init__(self, emu, L, shape, moves, n, mode, seed=700):
        from tile_match_gym_amd.seeding import batch_rng_words
        self.L, self.mode, self.moves = L, MODE_CODE[mode], moves
        self.words = batch_rng_words(range(seed, seed + n))
        self.e = emu.EmuBatch(L, *shape, moves, self.words)
        self.out = None
        L.emu_status_clear()

    def reset(self):
        self.e.reset()

    def set_boards(self, b):
        self.e.board[:] = b
        self.e.trust = False

    def set_timers(self, t):
        self.e.timer[:] = t

    def new_outputs(self, junk=False):
        self.out = fresh_outputs(self.state(), self.moves, junk)

    def edit(self, idx):
        self.e.board[idx, :, 0, 0] = 1
        self.e.trust = False

    def step(self, a):
        self.e.step(a, mode=self.mode, outputs=self.out)
        self.e.trust = True

    def step_policy(self, key, first, t):
        acts = np.full(self.e.n, -1, np.int32)
        self.e.step(acts, mode=self.mode, policy=(key, first, t), outputs=self.out)
        self.e.trust = True
        return acts

    def state(self):
        return {f: getattr(self.e, f) for f in ("board", "rng", "eff", "timer", "reward", "n_new", "n_act")}

    def outputs(self):
        return self.out

    def status(self):
        return self.L.emu_status()

    def spills(self):
        return self.L.emu_spills()


class DeviceBackend:
    """TileMatchVecEnv with output tensors of its own (set_step_outputs) and
    fused float32 one-hot planes (attach_onehot)."""

    def __init__(self, shape, moves, n, mode, groups, seed=40, device="cuda:0"):
        from tile_match_gym_amd.vec_env import TileMatchVecEnv
        R, C, k, sm = shape
        cl = ["cookie"] if sm & 1 else []
        co = [nm for bit, nm in ((2, "vertical_laser"), (4, "horizontal_laser"), (8, "bomb")) if sm & bit]
        self.mode, self.moves, self.dev = mode, moves, device
        self.env = TileMatchVecEnv(n, R, C, k, moves, cl, co, seed=seed, device=device, autoreset=False,
                                   groups=groups)
        self.words = self.env.rng_words().copy()
        self.t = None

    def reset(self):
        self.env.reset()

    def set_boards(self, b):
        import torch
        self.env.join()
        self.env.board.copy_(torch.from_numpy(b))
        self.env.invalidate_effective_cache()

    def set_timers(self, t):
        import torch
        self.env.join()
        self.env.timer.copy_(torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)))

    def new_outputs(self, junk=False):
        import torch
        env = self.env
        self.t = {f: torch.from_numpy(v).to(self.dev) for f, v in fresh_outputs(self.state(), self.moves, junk).items()}
        env.set_step_outputs(self.mode, **self.t)
        if env.onehot is None:
            env.attach_onehot(torch.float32)        # encodes the current boards
        else:
            env.refresh_onehot()
        if junk:
            env.onehot.fill_(3.0)

    def edit(self, idx):
        env = self.env
        env.join()
        env.board[idx, 0, 0, 0] = 1
        env.board[idx, 1, 0, 0] = 1
        env.invalidate_effective_cache()

    def step(self, a):
        import torch
        self.env.step_raw(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev))
        self.env.join()

    def step_policy(self, key, first, t):
        self.env.step_effective(t, key=key, first_env=first)
        self.env.join()
        return self.env.actions.cpu().numpy()

    def state(self):
        env = self.env
        env.join()
        s = {f: getattr(env, f).cpu().numpy() for f in ("board", "timer", "reward", "n_new", "n_act")}
        s["rng"] = env.rng_words()
        s["eff"] = env.eff.cpu().numpy().view(np.uint64)
        return s

    def outputs(self):
        out = {f: v.cpu().numpy() for f, v in self.t.items()}
        out["onehot"] = self.env.onehot.cpu().numpy()
        return out

    def status(self):
        return self.env.status()

    def spills(self):
        self.env.join()
        return self.env.ctx.spills()


def oracle_for(be, shape, moves, threads=1):
    from oracle import oracle as orc
    return orc.OracleBatch(*shape, moves, be.words, threads=threads)


def compare(be, o, want, shadow, what):
    """Every field of one step: the state against the oracle, the step's own
    outputs against the live-masked values, every fused output over all rows."""
    st, out = be.state(), be.outputs()
    for f in ("board", "rng", "eff", "timer"):
        assert np.array_equal(st[f], getattr(o, f)), (*what, f)
    for f in ("reward", "n_new", "n_act"):
        assert np.array_equal(st[f], want[f]), (*what, f)
    for f in ("terminated", "action_mask", "moves_left"):
        assert np.array_equal(out[f], want[f]), (*what, f)
    assert np.array_equal(out["board32"], o.board.astype(np.int32)), (*what, "board32")
    assert np.array_equal(out["final_board"], shadow), (*what, "final_board")
    if "onehot" in out:
        assert np.array_equal(out["onehot"], onehot_np(o.board, o.k, o.smask)), (*what, "onehot")


def keep_final(shadow, want, mode):
    """The host shadow of final_board: only the rows that terminated in a same-step call change."""
    if mode == "same_step":
        term = want["terminated"][:, 0].astype(bool)
        shadow[term] = want["final_board"][term]


def choose(o, rs, effective):
    """Uniform actions over [0, A); effective: one the oracle's mask holds, for every env that has one."""
    a = rs.integers(0, o.A, o.n).astype(np.int32)
    if effective:
        m = mask_bytes(o.eff, o.A)
        for i in range(o.n):
            nz = np.nonzero(m[i])[0]
            if nz.size:
                a[i] = nz[rs.integers(nz.size)]
    return a


def check_status(be, mode, what):
    """Steps after done are the caller's error in mode none and happen there; nothing else is ever flagged."""
    assert be.status() == (STATUS_CALLER if mode == "none" else 0), (*what, "status")


def drive(be, o, mode):
    """The schedule of the module docstring on backend `be` and its oracle `o`
    (same streams, num_moves = M).  Returns the number of (env, step) pairs that
    ended an episode and that ran as a step after done."""
    from oracle.policy_np import sample_effective_np
    shape = (o.R, o.C, o.k, o.smask)
    n, A = o.n, o.A
    assert o.num_moves == M and n % 8 != 0 and n % 64 != 0
    rs = np.random.default_rng([o.R, o.C, o.k, o.smask, MODE_CODE[mode]])
    shadow = np.full((n, 2, o.R, o.C), FINAL_FILL, np.int8)

    def start():
        be.reset()
        o.reset()
        for f in ("board", "rng", "eff"):
            assert np.array_equal(be.state()[f], getattr(o, f)), (shape, mode, "reset", f)
        timers = (np.arange(n) % M).astype(np.int32)
        be.set_timers(timers)
        o.timer[:] = timers
        be.new_outputs()
        return VectorOracle(o, mode)

    vo = start()
    ended = after_done = 0
    for t in range(STEPS):
        what = (shape, mode, t)
        if mode == "none" and (o.timer >= M).all():
            vo = start()
        if t in EDIT_STEPS:
            idx = np.arange(0, n, 3)
            be.edit(idx)
            o.board[idx, :, 0, 0] = 1
        if t in POLICY_STEPS:
            a = sample_effective_np(o.eff, A, POLICY_KEY, POLICY_FIRST, t)
            got = be.step_policy(POLICY_KEY, POLICY_FIRST, t)
            assert np.array_equal(got, a), (*what, "policy actions")
        else:
            a = choose(o, rs, effective=t % 2 == 1)
            be.step(a)
        want = vo.step(a)
        keep_final(shadow, want, mode)
        compare(be, o, want, shadow, what)
        ended += int(want["terminated"][:, 0].sum())
        after_done += int(want["terminated"][:, 3].sum())
    check_status(be, mode, (shape, mode))
    assert ended >= 2 * n, (shape, mode, ended)
    if mode == "none":
        assert after_done > 0, (shape, mode)
    return ended, after_done


def drive_spill(be, o, mode, timers):
    """Adversarial boards whose first (untrusted) step outgrows the LDS lists in
    every env, so spill_kernel writes every output of that step; with timers at
    M - 1 each of those steps ends its episode.  Every output starts as junk."""
    from adversarial import adversarial_boards, effective_actions
    shape = (o.R, o.C, o.k, o.smask)
    assert o.num_moves == SPILL_M and mode in ("same_step", "next_step")
    boards = [adversarial_boards(4, *shape, 11, m) for m in SPILL_BOARDS]
    b = np.concatenate(boards)
    a = np.concatenate([effective_actions(x) for x in boards])
    n = b.shape[0]
    assert n == o.n
    be.set_boards(b)
    o.board[:] = b
    tm = np.full(n, SPILL_M - 1 if timers == "last_move" else 0, np.int32)
    be.set_timers(tm)
    o.timer[:] = tm
    be.new_outputs(junk=True)
    vo = VectorOracle(o, mode)
    shadow = np.full((n, 2, o.R, o.C), FINAL_FILL, np.int8)
    rs = np.random.default_rng(5)
    s0 = be.spills()
    for t in range(3):
        be.step(a)
        want = vo.step(a)
        if t == 0:
            assert be.spills() - s0 == n, (shape, mode, timers, "spilled", be.spills() - s0)
            assert int(want["terminated"][:, 0].sum()) == (n if timers == "last_move" else 0)
        keep_final(shadow, want, mode)
        compare(be, o, want, shadow, (shape, mode, timers, t))
        a = choose(o, rs, effective=True)
    check_status(be, mode, (shape, mode, timers))
