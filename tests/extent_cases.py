"""The extent of every entry point of include/tmg.h at ragged batch sizes: the
shapes, the batch sizes, the banded buffers and the calls of
tests/test_gpu_extent.py; the census of tests/test_dispatch_route.py routes
EXTENT_SHAPES and fails when a row is deleted.

A call on n rows may write rows 0..n-1 of each of its arrays and nothing
else.  The other device tests hand the library tensors of exactly n rows
inside torch's caching allocator, where a stray store lands in a neighbouring
block that nobody looks at.  Here every array of every call, inputs included,
is a Band: FRONT guard rows, the n payload rows, BACK guard rows, every byte
0x5A, and the library gets the payload's address.  After each call the rows
below n are compared with the oracle as the parity tests do, every guard byte
must still be 0x5A, and every input must hold the bytes it held before.

0x5A in every byte is no legitimate output of any array: cells are -1..15,
counters are small, mask bytes are 0 / 1, one-hot values 0 / 1 / 1.0f, flag
bit 4 is never produced, and an untouched PCG64 or mask word would be
0x5A5A5A5A5A5A5A5A.

The guards are whole rows, so a payload starts where the rows of a plan group
with bounds[g] = FRONT start: a 7x9 board base is 2-byte aligned, a 10x10 one
8-byte aligned.  No other misalignment is tried: the ABI has none.  BACK
covers the padding of a grid to 8 workgroups, a 64-lane wave of the lane
kernel and the 8 envs per wave of a masked reset.

Only stores can be seen this way; tools/wave_emu/extent_asan.cpp sees the
loads too, on the host."""
import functools

import numpy as np

import fused_cases as fc
import rollout_cases as rc
from vector_ref import VectorOracle, reset_subset

FRONT, BACK, FILL = 3, 72, 0x5A

# (R, C, k, smask): one row per route class (the census names them)
EXTENT_SHAPES = [
    (3, 5, 2, 0),       # lean bitboard, odd C, 2N = 30, A = 22: byte stores for board and mask
    (7, 9, 5, 15),      # general bitboard, odd C, 2N = 126
    (10, 10, 4, 0),     # the c2 kernel, reset<128,2,kFixReset10>, the lane kernel with k = 4
    (10, 10, 5, 0),     # the lane kernel with k = 5, generic lean
    (10, 10, 4, 14),    # the c3 kernel, deferred reset at 8 envs per wave, spill tier
    (2, 22, 4, 0),      # A = 64, a full mask word, lean
    (2, 22, 4, 15),     # A = 64, general
    (2, 64, 4, 0),      # the non-bitboard 128-cell kernels
    (20, 20, 6, 15),    # the c5 kernel, reset<512,3,kFixReset20>, deferred reset at 2 envs per wave, spill tier
    (9, 15, 15, 0),     # lean 512-cell, reset<512,4>
]
LANE_SHAPES = [(10, 10, 4, 0), (10, 10, 5, 0)]
LANE_SMALL = 32768          # kLaneSmallEnvs: launches from this size on take 64 envs per wave
LANE_MIN = 131072           # kLaneMinEnvs: given-action launches from this size on run on the lane kernel
SPILL_SHAPES = fc.SPILL_SHAPES

MOVES = 2                   # every second step ends every episode
KEY, FIRST_ENV = fc.POLICY_KEY, fc.POLICY_FIRST
SEED0 = 300
STATUS_CALLER, FLAG_ERROR = 4, 0x80
# a period no wave, block or grid size divides: the large batches repeat the state of this many envs
BIG_PERIOD = 1031

case_id = fc.case_id


def batch_sizes(shape):
    """1: seven of eight workgroups idle.  9: a second masked-reset wave holding
    one env, odd for 2 envs per wave.  65: a third 32-env lane wave with one live
    lane, the sampler's second block, the one-hot block tail.  3: a ragged second
    wave at 2 envs per wave."""
    if shape in fc.SLOW:
        return (1, 9)
    return (1, 9, 65) if shape[0] * shape[1] <= 128 else (1, 3, 9)


CASES = [(s, n) for s in EXTENT_SHAPES for n in batch_sizes(s)]
GROUPS = ("reset", "step", "plan", "onehot", "effective", "peek", "rollout")
LANE_CASES = [(s, n) for s in LANE_SHAPES for n in (1, 9, 65, LANE_SMALL + 1)]


# ---------------------------------------------------------------- banded buffers
class Band:
    """FRONT + n + BACK rows of `row_shape` elements of a torch dtype, every
    byte FILL; `view` is the contiguous payload rows [FRONT, FRONT + n)."""

    def __init__(self, n, row_shape, dtype, device="cuda:0"):
        import torch
        self.n, self.row_shape, self.dtype = int(n), tuple(row_shape), dtype
        rows = FRONT + self.n + BACK
        self.row_bytes = torch.empty((), dtype=dtype).element_size() * int(np.prod(self.row_shape, dtype=np.int64))
        self.raw = torch.full((rows * self.row_bytes,), FILL, dtype=torch.uint8, device=device)
        self.view = self.raw.view(dtype).view(rows, *self.row_shape)[FRONT:FRONT + self.n]
        assert self.view.is_contiguous() and self.view.data_ptr() == self.raw.data_ptr() + FRONT * self.row_bytes

    def data_ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        lo, hi = FRONT * self.row_bytes, (FRONT + self.n) * self.row_bytes
        return bool((self.raw[:lo] == FILL).all().item()) and bool((self.raw[hi:] == FILL).all().item())

    def put(self, a):
        import torch
        a = np.array(a, order="C")                            # a writable copy: torch takes no read-only array
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        t = torch.from_numpy(a)
        assert t.dtype == self.dtype and tuple(t.shape) == tuple(self.view.shape), (t.dtype, t.shape, self.view.shape)
        self.view.copy_(t)

    def refill(self):
        self.raw.fill_(FILL)

    def host(self):
        return self.view.cpu().numpy()

    def words(self):
        return self.host().view(np.uint64)

    def payload_bytes(self):
        lo, hi = FRONT * self.row_bytes, (FRONT + self.n) * self.row_bytes
        return self.raw[lo:hi].cpu().numpy()


class Bands(dict):
    """The arrays of one call sequence by name."""

    def add(self, name, n, row_shape, dtype, data=None):
        b = self[name] = Band(n, row_shape, dtype)
        if data is not None:
            b.put(data)
        return b

    def ptr(self, name):
        return self[name].data_ptr()

    def ptrs(self, *names):
        return [self[f].data_ptr() for f in names]

    def snapshot(self, *names):
        return {f: self[f].payload_bytes() for f in names}

    def check(self, what, inputs=None):
        """Every guard of every array is intact; the arrays of `inputs` (a snapshot) hold the same bytes."""
        import torch
        torch.cuda.synchronize()
        for f, b in self.items():
            assert b.guards_intact(), (*what, f, "guard rows overwritten")
        for f, before in (inputs or {}).items():
            assert np.array_equal(self[f].payload_bytes(), before), (*what, f, "an input was written")


# ---------------------------------------------------------------- oracle states
def np_dtype(dtype):
    import torch
    return {torch.float32: np.float32, torch.uint8: np.uint8, torch.int32: np.int32}[dtype]


def oh_dtypes():
    import torch
    return ((torch.float32, 0), (torch.uint8, 1), (torch.int32, 2))      # TMG_DTYPE_F32 / U8 / I32


@functools.lru_cache(maxsize=None)
def seed_words(n, seed=SEED0):
    """(n, 5) PCG64 words; past BIG_PERIOD rows the first BIG_PERIOD repeat."""
    from tile_match_gym_amd.seeding import batch_rng_words
    w = batch_rng_words(range(seed, seed + min(n, BIG_PERIOD)))
    w = np.tile(w, ((n + BIG_PERIOD - 1) // BIG_PERIOD, 1))[:n] if n > BIG_PERIOD else w
    w.setflags(write=False)
    return w


def new_oracle(shape, n, num_moves=MOVES):
    from oracle import oracle as orc
    return orc.OracleBatch(*shape, num_moves, seed_words(n), threads=16 if n > BIG_PERIOD else 1)


@functools.lru_cache(maxsize=None)
def _reset_state(shape, n):
    o = new_oracle(shape, min(n, BIG_PERIOD))
    o.reset()
    st = {f: getattr(o, f) for f in ("board", "rng", "timer", "eff")}
    if n > BIG_PERIOD:
        reps = (n + BIG_PERIOD - 1) // BIG_PERIOD
        st = {f: np.concatenate([v] * reps)[:n] for f, v in st.items()}
    for v in st.values():
        v.setflags(write=False)
    return st


def reset_oracle(shape, n):
    """A fresh OracleBatch of the shape right after reset() (computed once per (shape, n))."""
    o = new_oracle(shape, n)
    for f, v in _reset_state(shape, n).items():
        getattr(o, f)[:] = v
    return o


@functools.lru_cache(maxsize=None)
def rolled_state(shape, n):
    """Boards that hold specials where the shape has them: reset() and three
    uniform-random steps of a 30-move episode; board, rng, eff (read-only)."""
    o = new_oracle(shape, n, 30)
    o.reset()
    rs = np.random.default_rng([*shape, n])
    for _ in range(3):
        o.step(rs.integers(0, o.A, n).astype(np.int32))
    st = {"board": o.board, "rng": o.rng, "eff": o.eff}
    for v in st.values():
        v.setflags(write=False)
    return st


def edited(board):
    """The hand edit of fused_cases: every third board gets a normal tile of colour 1 in its first cell."""
    b = board.copy()
    b[np.arange(0, b.shape[0], 3), :, 0, 0] = 1
    return b


def pack_masks(board):
    from oracle import oracle as orc
    return np.stack([rc.pack_mask(orc.effective_mask(x)[0]) for x in board])


@functools.lru_cache(maxsize=None)
def context(shape):
    from tile_match_gym_amd import _native
    return _native.Context(0, *shape, MOVES)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- the state and step arrays
class Rig:
    """The state arrays and the step's own outputs of n envs, banded."""

    STATE = ("board", "rng", "timer", "eff")
    OUTS = ("reward", "n_new", "n_act")

    def __init__(self, shape, n):
        import torch
        self.shape, self.n = shape, n
        R, C, k, sm = shape
        self.ctx = context(shape)
        self.A, self.W = self.ctx.num_actions, self.ctx.mask_words
        assert self.ctx.status(clear=True) >= 0
        b = self.b = Bands()
        b.add("board", n, (2, R, C), torch.int8)
        b.add("rng", n, (5,), torch.int64)
        b.add("timer", n, (), torch.int32)
        b.add("eff", n, (self.W,), torch.int64)
        for f in ("actions",) + self.OUTS:
            b.add(f, n, (), torch.int32)
        b.add("flags", n, (), torch.uint8)
        self.plans = []

    def plan(self, bounds, streams, mode, policy, **outputs):
        """A tmg_plan over the rig's arrays (streams: raw handles, 0 for the call's own)."""
        from tile_match_gym_amd import _native
        p = _native.Plan(self.ctx, self.n, *self.b.ptrs("board", "rng", "timer", "reward", "n_new", "n_act", "flags",
                                                        "eff"), bounds, streams)
        p.config(mode, policy=policy, key=KEY, first_env=FIRST_ENV, **outputs)
        self.plans.append(p)
        return p

    def run(self, plan, t, trust=1):
        plan.step(self.b.ptr("actions"), t, trust, stream())
        plan.join(stream())

    def close(self):
        for p in self.plans:
            p.close()

    def load(self, o):
        for f in self.STATE:
            self.b[f].put(getattr(o, f))

    def state_ptrs(self):
        return self.b.ptrs(*self.STATE)

    def step_ptrs(self):
        return self.b.ptrs("board", "rng", "timer", "actions", "reward", "n_new", "n_act", "flags", "eff")

    def same(self, f, want, what):
        got = self.b[f].host()
        if got.dtype == np.int64 and np.asarray(want).dtype == np.uint64:
            got = got.view(np.uint64)
        if not np.array_equal(got, want):
            bad = np.nonzero((got.reshape(self.n, -1) != np.asarray(want).reshape(self.n, -1)).any(axis=1))[0]
            raise AssertionError(f"{what}: {f} differs in {bad.size} rows of {self.n}, first {bad[:5].tolist()}")

    def check_state(self, o, what):
        import torch
        torch.cuda.synchronize()
        for f in self.STATE:
            self.same(f, getattr(o, f), what)

    def check_step(self, o, what):
        self.check_state(o, what)
        for f in self.OUTS + ("flags",):
            self.same(f, getattr(o, f), what)

    def check_status(self, o_flags, what):
        want = STATUS_CALLER if (np.asarray(o_flags) & 0xC0).any() else 0
        assert self.ctx.status(clear=True) == want, (*what, "status")


# ---------------------------------------------------------------- 1. tmg_reset
def run_reset(shape, n):
    """tmg_reset of every env, then of the envs of a mask: row 0, row n - 1 and a
    random third of the rest.  Timers are set to 1 first, so a row the masked
    call should not touch shows it."""
    import torch
    rig = Rig(shape, n)
    b, ctx = rig.b, rig.ctx
    o = new_oracle(shape, n)
    b["rng"].put(o.rng)                                     # board, timer and eff are outputs: FILL
    what = (shape, n, "reset")
    ctx.reset(n, *rig.state_ptrs(), None, stream())
    for f, v in _reset_state(shape, n).items():
        getattr(o, f)[:] = v
    rig.check_state(o, what)
    b.check(what)
    sel = np.random.default_rng([*shape, n]).random(n) < 1 / 3
    sel[0] = sel[n - 1] = True
    mask = np.where(sel, np.array([1, 0x80, 0xFF], np.uint8)[np.arange(n) % 3], 0).astype(np.uint8)
    b.add("env_mask", n, (), torch.uint8, mask)
    o.timer[:] = 1
    b["timer"].put(o.timer)
    before = b.snapshot("env_mask")
    what = (shape, n, "masked reset")
    ctx.reset(n, *rig.state_ptrs(), b.ptr("env_mask"), stream())
    reset_subset(o, np.nonzero(sel)[0])
    assert (o.timer[~sel] == 1).all() and (o.timer[sel] == 0).all()
    rig.check_state(o, what)                                # the unselected rows are the oracle's untouched ones
    b.check(what, before)
    rig.check_status(0, what)


# ---------------------------------------------------------------- 2. tmg_step
def run_step(shape, n):
    """tmg_step with num_moves = 2.  autoreset 1: two trusted steps (the second
    ends every episode and the reset regenerates every row), a hand edit, one
    untrusted step.  autoreset 0: a trusted step, the edit and the untrusted step
    (which ends every episode), then a trusted step after done: state untouched,
    TMG_FLAG_ERROR in every row, TMG_STATUS_CALLER."""
    for autoreset, kinds in ((1, ("trusted", "trusted", "edited")), (0, ("trusted", "edited", "trusted"))):
        rig = Rig(shape, n)
        b, ctx = rig.b, rig.ctx
        o = reset_oracle(shape, n)
        rig.load(o)
        rs = np.random.default_rng([*shape, n, autoreset])
        for t, kind in enumerate(kinds):
            what = (shape, n, "step", autoreset, t, kind)
            if kind == "edited":
                o.board[:] = edited(o.board)
                b["board"].put(o.board)
            a = fc.choose(o, rs, effective=t == 0)
            b["actions"].put(a)
            before = b.snapshot("actions")
            ctx.step(n, *rig.step_ptrs(), int(kind != "edited"), autoreset, stream())
            state = {f: getattr(o, f).copy() for f in rig.STATE}
            o.step(a, autoreset=bool(autoreset))
            rig.check_step(o, what)
            b.check(what, before)
            if t == 1:
                assert (o.flags & 1).all(), (*what, "the second move ends every episode")
                if autoreset:
                    assert (o.flags & 8).all() and not o.timer.any()
        if autoreset:
            rig.check_status(0, what)
        else:
            assert (o.flags == FLAG_ERROR).all() and all(np.array_equal(getattr(o, f), v) for f, v in state.items())
            rig.check_status(o.flags, what)


# ---------------------------------------------------------------- 3. step plans
class PlanRig(Rig):
    """Rig plus the fused outputs of tmg_plan_config."""

    FUSED = ("terminated", "action_mask", "moves_left", "final_board", "board32")

    def __init__(self, shape, n, oh_dtype, oh_code):
        import torch
        super().__init__(shape, n)
        R, C, k, sm = shape
        self.oh_dtype, self.oh_code = oh_dtype, oh_code
        b = self.b
        b.add("terminated", n, (4,), torch.uint8)
        b.add("action_mask", n, (self.A,), torch.uint8)
        b.add("moves_left", n, (), torch.int64)
        b.add("final_board", n, (2, R, C), torch.int8)
        b.add("board32", n, (2, R, C), torch.int32)
        b.add("onehot", n, (self.ctx.onehot_channels(), R, C), oh_dtype)

    def init_outputs(self, o, junk=False):
        """As vec_env initialises them after a reset; junk: values a step has to overwrite."""
        out = fc.fresh_outputs({"board": o.board, "eff": o.eff, "timer": o.timer}, MOVES, junk)
        for f in self.FUSED:
            self.b[f].put(out[f])
        oh = self.onehot_of(o)
        self.b["onehot"].put(np.full_like(oh, 3) if junk else oh)
        self.shadow = out["final_board"].copy()

    def onehot_of(self, o):
        return fc.onehot_np(o.board, o.k, o.smask).astype(np_dtype(self.oh_dtype))

    def plan(self, bounds, streams, mode, policy):
        b = self.b
        return super().plan(bounds, streams, mode, policy, onehot=b.ptr("onehot"), onehot_dtype=self.oh_code,
                            **{f: b.ptr(f) for f in self.FUSED})

    def check_fused(self, o, want, mode, what):
        fc.keep_final(self.shadow, want, mode)
        self.check_state(o, what)
        for f in self.OUTS + ("terminated", "action_mask", "moves_left"):
            self.same(f, want[f], what)
        self.same("board32", o.board.astype(np.int32), what)
        self.same("final_board", self.shadow, what)
        self.same("onehot", self.onehot_of(o), what)


def plan_steps(rig, o, mode, given, policy, kinds, what0, trust0=1):
    """One step per entry of `kinds` ("given": drawn here, "policy": the in-kernel
    draw, or an array of given actions) of the plans on rig against VectorOracle."""
    from oracle.policy_np import sample_effective_np
    b = rig.b
    vo = VectorOracle(o, mode)
    rs = np.random.default_rng([*rig.shape, rig.n, fc.MODE_CODE[mode]])
    ended = 0
    for t, kind in enumerate(kinds):
        what = (*what0, mode, t, kind if isinstance(kind, str) else "given")
        if isinstance(kind, str) and kind == "policy":
            a = sample_effective_np(o.eff, rig.A, KEY, FIRST_ENV, t)
            b["actions"].refill()
            rig.run(policy, t)
            before = None
        else:
            a = fc.choose(o, rs, effective=t % 2 == 0) if isinstance(kind, str) else kind
            b["actions"].put(a)
            before = b.snapshot("actions")
            rig.run(given, t, trust0 if t == 0 else 1)
        want = vo.step(a)
        rig.check_fused(o, want, mode, what)
        if before is None:
            rig.same("actions", a, what)
        b.check(what, before)
        ended += int(want["terminated"][:, 0].sum())
    return ended


def run_plan(shape, n):
    """A plan over bounds [0, 0, 1, n]: an empty group, a group of one, the rest,
    so every kernel runs at row offsets 0 and 1.  NULL group streams and three
    streams, same-step and next-step autoreset, the one-hot planes in each
    dtype, every fused output attached: given actions, given actions (every
    episode ends), the in-kernel policy (next step: every row is reset), given
    actions."""
    import torch
    assert n >= 2
    (f32, c32), (u8, cu8), (i32, ci32) = oh_dtypes()
    streams = [torch.cuda.Stream("cuda:0") for _ in range(3)]
    configs = [(None, "same_step", f32, c32), (streams, "next_step", u8, cu8), (streams, "same_step", i32, ci32),
               (None, "next_step", f32, c32)]
    for sts, mode, dtype, code in configs:
        rig = PlanRig(shape, n, dtype, code)
        o = reset_oracle(shape, n)
        rig.load(o)
        rig.init_outputs(o)
        raw = [s.cuda_stream for s in sts] if sts else [0, 0, 0]
        given = rig.plan([0, 0, 1, n], raw, mode, False)
        policy = rig.plan([0, 0, 1, n], raw, mode, True)
        what = (shape, n, "plan", "streams" if sts else "null")
        ended = plan_steps(rig, o, mode, given, policy, ("given", "given", "policy", "given"), what)
        assert ended >= n, (*what, mode, ended)
        rig.check_status(0, what)
        rig.close()


def run_lane(shape, n):
    """The in-kernel policy with no fused output: the lane kernel, 32 envs per
    wave below LANE_SMALL envs and 64 from there on, one launch over all n rows.
    Same step: three steps, the second ends every episode and the deferred reset
    (2 envs per wave) regenerates every row.  Next step, on the small batches:
    four steps against VectorOracle."""
    from oracle.policy_np import sample_effective_np
    big = n > BIG_PERIOD
    rig = Rig(shape, n)
    b = rig.b
    o = reset_oracle(shape, n)
    rig.load(o)
    plan = rig.plan([0, n], [0], "same_step", True)
    for t in range(2 if big else 3):
        what = (shape, n, "lane", "same_step", t)
        a = sample_effective_np(o.eff, rig.A, KEY, FIRST_ENV, t)
        b["actions"].refill()
        rig.run(plan, t)
        o.step(a, autoreset=True)
        rig.check_step(o, what)
        rig.same("actions", a, what)
        b.check(what)
        if t == 1:
            assert (o.flags & 9 == 9).all() and not o.timer.any()
    rig.check_status(0, what)
    if big:
        rig.close()
        return
    o = reset_oracle(shape, n)
    rig.load(o)
    plan = rig.plan([0, n], [0], "next_step", True)
    vo = VectorOracle(o, "next_step")
    for t in range(4):
        what = (shape, n, "lane", "next_step", t)
        a = sample_effective_np(o.eff, rig.A, KEY, FIRST_ENV, t)
        b["actions"].refill()
        rig.run(plan, t)
        want = vo.step(a)
        rig.check_state(o, what)
        for f in rig.OUTS:
            rig.same(f, want[f], what)
        rig.same("actions", a, what)
        b.check(what)
    rig.check_status(0, what)
    rig.close()


def run_lane_given(shape, n):
    """One given-action tmg_step of more than LANE_MIN envs: the lane kernel at 64
    envs per wave with one live lane in the last wave.  Every 16th env and the
    last one are on their last move, so the deferred reset has rows to regenerate."""
    assert n > LANE_MIN
    rig = Rig(shape, n)
    b = rig.b
    o = reset_oracle(shape, n)
    o.timer[::16] = MOVES - 1
    o.timer[n - 1] = MOVES - 1
    rig.load(o)
    a = fc.choose(reset_oracle(shape, BIG_PERIOD), np.random.default_rng(5), effective=True)
    a = np.tile(a, (n + BIG_PERIOD - 1) // BIG_PERIOD)[:n]
    a[1::7] = np.random.default_rng(6).integers(0, rig.A, a[1::7].size)
    b["actions"].put(a)
    before = b.snapshot("actions")
    what = (shape, n, "lane, given actions")
    rig.ctx.step(n, *rig.step_ptrs(), 1, 1, stream())
    o.step(a, autoreset=True)
    assert (o.flags[::16] & 9 == 9).all() and o.flags[n - 1] & 9 == 9
    rig.check_step(o, what)
    b.check(what, before)
    rig.check_status(0, what)


# ---------------------------------------------------------------- 4. one-hot planes
def run_onehot(shape, n):
    """tmg_onehot in the three dtypes; tmg_reset_onehot and two tmg_step_onehot
    calls (the second ends every episode and regenerates every row) per dtype."""
    import torch
    R, C, k, sm = shape
    ctx = context(shape)
    for dtype, code in oh_dtypes():
        rig = Rig(shape, n)
        b = rig.b
        o = reset_oracle(shape, n)
        want = lambda: fc.onehot_np(o.board, k, sm).astype(np_dtype(dtype))      # noqa: E731
        b.add("onehot", n, (ctx.onehot_channels(), R, C), dtype)
        b["board"].put(edited(o.board))
        before = b.snapshot("board")
        what = (shape, n, "onehot", code)
        ctx.onehot(n, b.ptr("board"), b.ptr("onehot"), code, stream())
        torch.cuda.synchronize()
        rig.same("onehot", fc.onehot_np(edited(o.board), k, sm).astype(np_dtype(dtype)), what)
        b.check(what, before)
        # tmg_reset_onehot from the seeds' words: every state array and the planes are outputs
        for f in ("board", "timer", "eff", "onehot"):
            b[f].refill()
        b["rng"].put(seed_words(n))
        what = (shape, n, "reset_onehot", code)
        ctx.reset(n, *rig.state_ptrs(), None, stream(), onehot=b.ptr("onehot"), onehot_dtype=code)
        rig.check_state(o, what)
        rig.same("onehot", want(), what)
        b.check(what)
        rs = np.random.default_rng([*shape, n, code])
        for t in range(2):
            what = (shape, n, "step_onehot", code, t)
            a = fc.choose(o, rs, effective=True)
            b["actions"].put(a)
            before = b.snapshot("actions")
            ctx.step(n, *rig.step_ptrs(), 1, 1, stream(), onehot=b.ptr("onehot"), onehot_dtype=code)
            o.step(a, autoreset=True)
            rig.check_step(o, what)
            rig.same("onehot", want(), what)
            b.check(what, before)
        rig.check_status(0, what)


# ---------------------------------------------------------------- 5. masks and the sampler
def run_effective(shape, n):
    """tmg_effective on hand-edited boards; tmg_sample_effective on those masks
    with the last row's mask empty (the uniform draw over all A), first_env = 1000."""
    import torch
    from oracle.policy_np import sample_effective_np
    R, C, k, sm = shape
    ctx = context(shape)
    b = Bands()
    board = edited(rolled_state(shape, n)["board"])
    b.add("board", n, (2, R, C), torch.int8, board)
    b.add("eff", n, (ctx.mask_words,), torch.int64)
    b.add("actions", n, (), torch.int32)
    what = (shape, n, "effective")
    before = b.snapshot("board")
    ctx.effective(n, b.ptr("board"), b.ptr("eff"), stream())
    torch.cuda.synchronize()
    eff = pack_masks(board)
    assert np.array_equal(b["eff"].words(), eff), what
    b.check(what, before)
    eff[n - 1] = 0
    b["eff"].put(eff)
    before = b.snapshot("board", "eff")
    what = (shape, n, "sample_effective")
    ctx.sample_effective(n, b.ptr("eff"), KEY, FIRST_ENV, 7, b.ptr("actions"), stream())
    torch.cuda.synchronize()
    assert np.array_equal(b["actions"].host(), sample_effective_np(eff, ctx.num_actions, KEY, FIRST_ENV, 7)), what
    b.check(what, before)
    assert ctx.status(clear=True) == 0


# ---------------------------------------------------------------- 6. tmg_peek
PEEK_OUT = ("reward", "n_new", "n_act", "flags", "best_action", "best_reward")


def peek_bands(shape, n, board, rng, eff):
    import torch
    R, C, k, sm = shape
    A, W = 2 * R * C - R - C, (2 * R * C - R - C + 63) // 64
    b = Bands()
    b.add("board", n, (2, R, C), torch.int8, board)
    b.add("rng", n, (5,), torch.int64, rng)
    b.add("eff", n, (W,), torch.int64, eff)
    for f in ("reward", "n_new", "n_act"):
        b.add(f, n, (A,), torch.int32)
    b.add("flags", n, (A,), torch.uint8)
    b.add("best_action", n, (), torch.int32)
    b.add("best_reward", n, (), torch.int32)
    return b


def check_peek(b, want, what, inputs):
    import torch
    torch.cuda.synchronize()
    for f in PEEK_OUT:
        got = b[f].host()
        assert np.array_equal(got, want[f]), (*what, f, np.argwhere(got != want[f])[:5].tolist())
    b.check(what, inputs)


def run_peek(shape, n):
    """tmg_peek with all six outputs: trusted on rolled boards with their own
    masks, untrusted on hand-edited boards (eff still passed: it is not written)."""
    from peek_cases import oracle_peek
    R, C, k, sm = shape
    ctx = context(shape)
    st = rolled_state(shape, n)
    for trust, board in ((1, st["board"]), (0, edited(st["board"]))):
        b = peek_bands(shape, n, board, st["rng"], st["eff"])
        before = b.snapshot("board", "rng", "eff")
        what = (shape, n, "peek", trust)
        ctx.peek(n, b.ptr("board"), b.ptr("rng"), b.ptr("eff"), trust, *b.ptrs(*PEEK_OUT), stream())
        check_peek(b, oracle_peek(board, st["rng"], k, sm), what, before)
    assert ctx.status(clear=True) == 0


# ---------------------------------------------------------------- 7. tmg_rollout
def rollout_bands(shape, n, samples, board, rng, eff, timer):
    import torch
    R, C, k, sm = shape
    A, W = 2 * R * C - R - C, (2 * R * C - R - C + 63) // 64
    b = Bands()
    b.add("board", n, (2, R, C), torch.int8, board)
    b.add("rng", samples * n, (5,), torch.int64, np.asarray(rng).reshape(samples * n, 5))      # [samples][n][5]
    b.add("eff", n, (W,), torch.int64, eff)
    b.add("timer", n, (), torch.int32, timer)
    for f in ("ret", "plies"):
        b.add(f, samples * n, (A,), torch.int32)                                                # [samples][n][A]
    b.add("flags", samples * n, (A,), torch.uint8)
    b.add("total", n, (A,), torch.int32)
    b.add("best_action", n, (), torch.int32)
    b.add("best_total", n, (), torch.int32)
    return b


def check_rollout(b, want, what, inputs):
    import torch
    torch.cuda.synchronize()
    for f in rc.FIELDS:
        got = b[f].host().reshape(want[f].shape)
        assert np.array_equal(got, want[f]), (*what, f, np.argwhere(got != want[f])[:5].tolist())
    b.check(what, inputs)


def run_rollout(shape, n):
    """tmg_rollout, depth 2, 2 samples (the envs' own words and words of other
    seeds), all six outputs: with the timers (horizons 2, 1 and 0 in turn) and
    without."""
    R, C, k, sm = shape
    ctx = context(shape)
    st = rolled_state(shape, n)
    rng = np.stack([st["rng"], seed_words(n, 7000)])
    timers = (np.arange(n) % 3).astype(np.int32)
    for timed in (True, False):
        b = rollout_bands(shape, n, 2, st["board"], rng, st["eff"], timers)
        before = b.snapshot("board", "rng", "eff", "timer")
        what = (shape, n, "rollout", timed)
        ctx.rollout(n, b.ptr("board"), b.ptr("rng"), b.ptr("timer") if timed else None, b.ptr("eff"), 1, 2, 2,
                    rc.KEY, rc.FIRST_ENV, rc.T, *b.ptrs(*rc.FIELDS), stream())
        want = rc.oracle_rollout(st["board"], rng, timers if timed else None, MOVES, k, sm, 2, 2, rc.KEY, rc.FIRST_ENV,
                                 rc.T)
        check_rollout(b, want, what, before)
    assert ctx.status(clear=True) == 0


RUN = {"reset": run_reset, "step": run_step, "plan": run_plan, "onehot": run_onehot, "effective": run_effective,
       "peek": run_peek, "rollout": run_rollout}


# ---------------------------------------------------------------- 8. the spill tier
SPILL_N = 3 * len(fc.SPILL_BOARDS)
SPILL_CALLS = ("step", "peek", "rollout")


@functools.lru_cache(maxsize=None)
def spill_boards(shape):
    """The first three boards of each mode of fused_cases.SPILL_BOARDS as drive_spill
    makes them (four per mode), with drive_spill's effective action of each."""
    from adversarial import adversarial_boards, effective_actions
    boards = [adversarial_boards(4, *shape, 11, m) for m in fc.SPILL_BOARDS]
    b, a = np.concatenate([x[:3] for x in boards]), np.concatenate([effective_actions(x)[:3] for x in boards])
    b.setflags(write=False)
    a.setflags(write=False)
    return b, a


def run_spill(shape, call):
    """Boards whose move outgrows the LDS lists in every env, so the spill kernels
    write the results (n = 9 rows; a spill launch has 16 waves).  step: one
    untrusted same-step plan step over bounds [0, 0, 1, n] with every fused
    output junk before and the timers at num_moves - 1, so every spilled step
    ends its episode and the deferred reset follows.  peek: untrusted, the same
    words, so every env spills again.  rollout: 2 samples, 18 queued ids for 16
    waves; sample 0 has the envs' words and spills in every env."""
    import torch
    R, C, k, sm = shape
    n = SPILL_N
    boards, acts = spill_boards(shape)
    ctx = context(shape)
    words = seed_words(n, 40)
    s0 = ctx.spills()
    what = (shape, n, "spill", call)
    if call == "step":
        rig = PlanRig(shape, n, torch.float32, 0)
        o = new_oracle(shape, n)
        o.rng[:] = words
        o.board[:] = boards
        o.timer[:] = MOVES - 1
        rig.load(o)                                         # eff: zeros, not read (untrusted)
        rig.init_outputs(o, junk=True)
        given = rig.plan([0, 0, 1, n], [0, 0, 0], "same_step", False)
        ended = plan_steps(rig, o, "same_step", given, None, (acts.copy(),), what, trust0=0)
        assert ended == n and ctx.spills() - s0 == n, (*what, ended, ctx.spills() - s0)
        rig.check_status(0, what)
        rig.close()
        return
    from peek_cases import oracle_peek
    eff = np.zeros((n, ctx.mask_words), np.uint64)
    if call == "peek":
        b = peek_bands(shape, n, boards, words, eff)
        before = b.snapshot("board", "rng", "eff")
        ctx.peek(n, b.ptr("board"), b.ptr("rng"), b.ptr("eff"), 0, *b.ptrs(*PEEK_OUT), stream())
        check_peek(b, oracle_peek(boards, words, k, sm), what, before)
        assert ctx.spills() - s0 == n, (*what, ctx.spills() - s0)
    else:
        # depth 2 on the 128-cell shape; the 512-cell one plays one ply (its oracle needs 6 s for two)
        depth = 2 if R * C <= 128 else 1
        rng = np.stack([words, seed_words(n, 7000)])
        b = rollout_bands(shape, n, 2, boards, rng, eff, np.zeros(n, np.int32))
        before = b.snapshot("board", "rng", "eff", "timer")
        ctx.rollout(n, b.ptr("board"), b.ptr("rng"), None, b.ptr("eff"), 0, depth, 2, rc.KEY, rc.FIRST_ENV, rc.T,
                    *b.ptrs(*rc.FIELDS), stream())
        want = rc.oracle_rollout(boards, rng, None, MOVES, k, sm, depth, 2, rc.KEY, rc.FIRST_ENV, rc.T)
        check_rollout(b, want, what, before)
        assert ctx.spills() - s0 >= n, (*what, ctx.spills() - s0)
    assert ctx.status(clear=True) == 0
