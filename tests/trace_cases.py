"""The oracle side of the tmg_trace tests (tests/test_trace_emulated.py on the
host wave emulator, tests/test_gpu_trace.py on the device, tests/test_trace_cases.py
for the walk itself).

The expected frames come from a stage-by-stage walk composed from the oracle's
primitives only (effective_mask, combination, detect_resolve, gravity,
rng_colours, rng_shuffle, get_colour_lines): oracle.move is never called for
them and tmg_step never.  tests/test_trace_cases.py pins that walk to
oracle.move."""
import functools

import numpy as np

import dispatch_cases
import edge_cases
import peek_cases
from oracle import oracle as orc
from rowplane_cases import action_cells

SWAP, COMBO, CLEAR, FALL, REFILL, SHUFFLE = 1, 2, 3, 4, 5, 6
KINDS = (SWAP, COMBO, CLEAR, FALL, REFILL, SHUFFLE)
STAGE_NAMES = {SWAP: "swap", COMBO: "combo", CLEAR: "clear", FALL: "fall", REFILL: "refill", SHUFFLE: "shuffle"}
ALL_STAGES = sum(1 << s for s in KINDS)
DEFAULT_STAGES = (1 << CLEAR) | (1 << FALL) | (1 << REFILL)
FLAG_COMBO, FLAG_SHUFFLED, FLAG_STOPPED, FLAG_ERROR = 2, 4, 0x10, 0x80
STATUS_INTERNAL, STATUS_CALLER = 1, 4
SMALL = ("n_frames", "reward", "n_new", "n_act", "flags", "kind", "frame_elim", "out_rng")
FIELDS = ("frames",) + SMALL
WHOLE = 256                     # max_frames of the whole-move cases (8x8 k3 reaches 163 frames)
FILL = -7                       # what unwritten frame boards hold in the expected arrays
FILL_BYTE = FILL & 0xFF

case_id = peek_cases.case_id


class Stage:
    """One stage of a move: its kind, the board after it, its eliminations,
    and the RNG words / n_new / n_act / combo flag of the move so far."""

    def __init__(self, kind, board, elim, rng, n_new, n_act, combo):
        self.kind, self.board, self.elim, self.rng = kind, board.copy(), int(elim), rng.copy()
        self.n_new, self.n_act, self.combo = int(n_new), int(n_act), int(combo)


def oracle_trace(board, rng, a, k, smask):
    """Board.move(a) (board.py:330-395) on a copy of board (2, R, C) int8 with a
    copy of the words rng (5,) uint64, stage by stage -> ([Stage], board after
    the move, words after it, (elim, combo, n_new, n_act, shuffled)).  An
    ineffective action: no stage, board and words as given, zeros."""
    b = np.ascontiguousarray(board, np.int8).copy()
    g = np.asarray(rng, np.uint64).copy()
    _, R, C = b.shape
    if not orc.effective_mask(b)[0][a]:
        return [], b, g, (0, 0, 0, 0, 0)
    st = {"n_new": 0, "n_act": 0, "combo": 0, "elim": 0}
    stages = []

    def emit(kind, e=0):
        stages.append(Stage(kind, b, e, g, st["n_new"], st["n_act"], st["combo"]))

    def fall_refill():
        nonlocal b, g
        b = orc.gravity(b)
        emit(FALL)
        holes = (b[0] == 0) & (b[1] == 0)                       # row-major, board.py:233-241
        if holes.any():
            cols, g = orc.rng_colours(g, k, int(holes.sum()))
            b[0][holes] = cols.astype(np.int8)
            b[1][holes] = 1
        emit(REFILL)

    (r1, c1), (r2, c2) = action_cells(R, C, a)
    for pl in (0, 1):
        b[pl, r1, c1], b[pl, r2, c2] = b[pl, r2, c2], b[pl, r1, c1]
    emit(SWAP)
    t1, t2 = int(b[1, r1, c1]), int(b[1, r2, c2])
    if (t1 not in (0, 1) and t2 not in (0, 1)) or t1 < 0 or t2 < 0:            # board.py:357
        b, na, err = orc.combination(b, a, k, smask)
        assert err == 0
        st["combo"], st["n_act"] = 1, st["n_act"] + na
        e = int((b[1] == 0).sum())
        st["elim"] += e
        emit(COMBO, e)
        fall_refill()
    while True:
        nb, na, nn, err = orc.detect_resolve(b, k, smask)
        assert err == 0
        if np.array_equal(nb, b):                                # no line (or lines but no match)
            break
        b = nb
        st["n_act"] += na
        st["n_new"] += nn
        e = int((b[1] == 0).sum())
        st["elim"] += e
        emit(CLEAR, e)
        fall_refill()
    shuffled = 0
    lines = []
    while not orc.effective_mask(b)[1] or lines:                 # board.py:381-391
        if lines:
            while lines:                                         # remove_colour_lines :120-131
                row = min(R - 1, lines[0][0][0] + 1)
                cols, g = orc.rng_colours(g, k, (row + 1) * C)
                b[0].reshape(-1)[:(row + 1) * C] = cols.astype(np.int8)
                lines = orc.get_colour_lines(b, k, smask)
        else:
            idx, g = orc.rng_shuffle(g, R * C)
            b = np.ascontiguousarray(b.reshape(2, -1)[:, idx].reshape(2, R, C))
            shuffled = 1
        lines = orc.get_colour_lines(b, k, smask)
    if shuffled:
        emit(SHUFFLE)
    return stages, b, g, (st["elim"] + st["n_new"], st["combo"], st["n_new"], st["n_act"], shuffled)


@functools.lru_cache(maxsize=4096)
def _walk(board_bytes, shape3, rng_bytes, a, k, smask):
    board = np.frombuffer(board_bytes, np.int8).reshape(shape3)
    return oracle_trace(board, np.frombuffer(rng_bytes, np.uint64), a, k, smask)


def expected(board, rng, actions, k, smask, stage_mask, max_frames, stop):
    """What tmg_trace must write for board (n, 2, R, C), rng (n, 5), actions
    (Q, n): dict of FIELDS.  Frame boards that are not written hold FILL."""
    n, _, R, C = board.shape
    A = orc.num_actions(R, C)
    actions = np.asarray(actions, np.int32)
    Q, F = actions.shape[0], max_frames
    out = {f: np.zeros((Q, n), np.int32) for f in ("n_frames", "reward", "n_new", "n_act")}
    out["flags"] = np.zeros((Q, n), np.uint8)
    out["kind"] = np.zeros((Q, n, F), np.uint8)
    out["frame_elim"] = np.zeros((Q, n, F), np.int32)
    out["frames"] = np.full((Q, n, F, 2, R, C), FILL, np.int8)
    out["out_rng"] = np.zeros((Q, n, 5), np.uint64)
    for q in range(Q):
        for i in range(n):
            a = int(actions[q, i])
            out["out_rng"][q, i] = rng[i]
            if a < 0:
                continue
            if a >= A:
                out["flags"][q, i] = FLAG_ERROR
                continue
            stages, _, g1, res = _walk(np.ascontiguousarray(board[i], np.int8).tobytes(), board[i].shape,
                                       np.ascontiguousarray(rng[i], np.uint64).tobytes(), a, k, smask)
            nf, last = 0, None
            for s_i, s in enumerate(stages):
                if not (stage_mask >> s.kind) & 1:
                    continue
                if nf < F:
                    out["frames"][q, i, nf], out["kind"][q, i, nf], out["frame_elim"][q, i, nf] = s.board, s.kind, s.elim
                nf += 1
                if stop and nf == F:
                    last = s_i
                    break
            out["n_frames"][q, i] = nf
            if last is None:                                     # the whole move
                out["reward"][q, i], combo, out["n_new"][q, i], out["n_act"][q, i], shuf = res
                out["flags"][q, i] = (FLAG_COMBO if combo else 0) | (FLAG_SHUFFLED if shuf else 0)
                out["out_rng"][q, i] = g1
            else:                                                # stopped right after stage `last`
                s = stages[last]
                out["reward"][q, i] = sum(x.elim for x in stages[:last + 1]) + s.n_new
                out["n_new"][q, i], out["n_act"][q, i] = s.n_new, s.n_act
                # the flags of the stages run: a row stopped on its SHUFFLE frame has shuffled
                out["flags"][q, i] = (FLAG_STOPPED | (FLAG_COMBO if s.combo else 0)
                                      | (FLAG_SHUFFLED if s.kind == SHUFFLE else 0))
                out["out_rng"][q, i] = s.rng
    return out


def assert_trace_equal(got, want, what="", fields=FIELDS):
    for f in fields:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.dtype == np.int64 and w.dtype == np.uint64:
            g = g.view(np.uint64)
        g = g.reshape(w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:5]
            raise AssertionError(f"{what}: {f} differs at {bad.tolist()}: "
                                 f"got {[int(g[tuple(b)]) for b in bad]}, want {[int(w[tuple(b)]) for b in bad]}")


# ---------------------------------------------------------------- every field, whole moves
SHUFFLING = list(dispatch_cases.SHUFFLES)                        # (2, 63, 9, 0), (7, 9, 10, 15), (6, 8, 12, 0)
# 2N no multiple of 4 (frames on 2-byte boundaries), the lean and general shapes of the other lookahead tests, the
# shuffling shapes, 20x20 and the smallest board of the 512-cell family
FIELD_SHAPES = ([(3, 3, 2, 0), (3, 5, 3, 15), (4, 4, 2, 0), (8, 8, 3, 15), (10, 10, 4, 0), (10, 10, 4, 14)] + SHUFFLING
                + [(20, 20, 6, 15), dispatch_cases.FAMILY_512[1]])
LIMIT_SHAPES = list(edge_cases.LOOKAHEAD_DEVICE)                 # on the device; on the emulator where it is quick
EMU_LIMIT_SHAPES = [(1, 64, 5, 15), (64, 1, 3, 14)]
STEP_SHAPES = [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)]  # also against a real tmg_step on a copy


def greedy_action(board, rs):
    return int(rs.choice(np.nonzero(orc.effective_mask(board)[0])[0]))


@functools.lru_cache(maxsize=None)
def shuffle_state(shape, seed0, n):
    """(board (n, 2, R, C), rng (n, 5), action (n,)): per env, the state and the
    action of the first move that shuffles, found by playing effective actions
    forward with the oracle (6 seeds of 30 moves at the most per env)."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k, sm = shape
    boards, words, acts = [], [], []
    seed = seed0
    rs = np.random.default_rng([*shape, seed0])
    while len(boards) < n:
        assert seed < seed0 + 6 * n, f"{shape}: no shuffling move found"
        b, g = orc.generate(R, C, k, sm, batch_rng_words([seed])[0])
        seed += 1
        for _ in range(30):
            a = greedy_action(b, rs)
            nb, ng, res, err = orc.move(b, g, a, k, sm)
            assert err == 0
            if res[4]:
                boards.append(b), words.append(g), acts.append(a)
                break
            b, g = nb, ng
    return np.stack(boards), np.stack(words), np.array(acts, np.int32)


def action_rows(board, rs, first=None):
    """(3, n) int32: an effective action per env (`first` when given); a
    uniformly random action; a row mixing -1, A and valid actions."""
    n, _, R, C = board.shape
    A = orc.num_actions(R, C)
    acts = np.zeros((3, n), np.int32)
    acts[0] = first if first is not None else [greedy_action(board[i], rs) for i in range(n)]
    acts[1] = rs.integers(0, A, n)
    acts[2] = [(-1, A, greedy_action(board[i], rs), int(rs.integers(0, A)))[i % 4] for i in range(n)]
    return acts


@functools.lru_cache(maxsize=None)
def field_case(shape):
    """(board, rng, actions (3, n), want) of the whole-move case of a shape:
    all stages, max_frames = WHOLE, stop = 0.  Computed once, read-only."""
    n = peek_cases.envs_of(shape)
    rs = np.random.default_rng([*shape, 77])
    if shape in SHUFFLING:
        board, rng, first = shuffle_state(shape, 900, n)
    else:
        o = peek_cases.rolled_batch(shape, range(500, 500 + n), steps=7)
        board, rng, first = o.board.copy(), o.rng.copy(), None
    acts = action_rows(board, rs, first)
    want = expected(board, rng, acts, shape[2], shape[3], ALL_STAGES, WHOLE, 0)
    for a in (board, rng, acts, *want.values()):
        a.setflags(write=False)
    return board, rng, acts, want


# ---------------------------------------------------------------- stage masks and cuts
CUT_SHAPES = [(10, 10, 4, 14), (6, 8, 12, 0)]
CUT_MASKS = [1 << s for s in KINDS] + [DEFAULT_STAGES]
CUT_FRAMES = (1, 4)


# ---------------------------------------------------------------- hand-written boards
@functools.lru_cache(maxsize=None)
def adversarial_case(shape, mode, n):
    """(boards, words, actions (2, n)) of the untrusted / spill case: the boards
    of tests/adversarial.py (they may hold a line), q0 an action the oracle's
    mask of the board as it stands calls effective, q1 uniform over [0, A)."""
    from adversarial import adversarial_boards
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k, sm = shape
    b = adversarial_boards(n, R, C, k, sm, 11, mode)
    words = batch_rng_words(range(300, 300 + n))
    rs = np.random.default_rng([*shape, n])
    acts = np.stack([np.array([greedy_action(b[i], rs) for i in range(n)]),
                     rs.integers(0, orc.num_actions(R, C), n)]).astype(np.int32)
    for a in (b, words, acts):
        a.setflags(write=False)
    return b, words, acts


# ---------------------------------------------------------------- extent
EXTENT_SHAPE = (10, 10, 4, 14)
EXTENT_ODD_SHAPE = (3, 5, 3, 15)            # frames on 2-byte boundaries
EXTENT_N = (1, 3, 9, 65)
EXTENT_SEQS = (1, 2)
EXTENT_FRAMES = 6
GUARD = 2                                    # guard rows in front of and behind every array


@functools.lru_cache(maxsize=None)
def extent_state(shape, n):
    o = peek_cases.rolled_batch(shape, range(1200, 1200 + n), steps=3)
    rs = np.random.default_rng([*shape, n])
    acts = np.stack([np.array([greedy_action(o.board[i], rs) for i in range(n)]),
                     rs.integers(-1, o.A + 1, n)]).astype(np.int32)
    # env 0 plays its shortest move, so that a row leaves frame slots unwritten at any n
    eff0 = np.nonzero(orc.effective_mask(o.board[0])[0])[0]
    acts[0, 0] = min(eff0, key=lambda a: len(oracle_trace(o.board[0], o.rng[0], int(a), shape[2], shape[3])[0]))
    return o.board.copy(), o.rng.copy(), acts


def all_cases():
    """(name, board, rng, actions, k, smask) of every state the other files
    trace, for tests/test_trace_cases.py."""
    from adversarial import MODES
    for s in FIELD_SHAPES + EMU_LIMIT_SHAPES:
        b, g, a, _ = field_case(s)
        yield case_id(s), b, g, a, s[2], s[3]
    for s in peek_cases.ADVERSARIAL_SHAPES:
        if s[0] * s[1] > 128:
            continue                                    # the oracle walk of the 20x20 sea is the device test's
        for m in MODES:
            b, g, a = adversarial_case(s, m, peek_cases.envs_of(s))
            yield f"{case_id(s)}-{m}", b, g, a, s[2], s[3]
    for s in (EXTENT_SHAPE, EXTENT_ODD_SHAPE):
        b, g, a = extent_state(s, 9)
        yield f"extent-{case_id(s)}", b, g, a, s[2], s[3]


# ---------------------------------------------------------------- the checks both test files run
# `dev` is the thing under test (the host wave emulator or the library on the
# device), behind four methods:
#   dev.run(shape, board, rng, eff, trust_eff, actions, stage_mask, max_frames, stop, bufs, lead) -> None
#       tmg_trace; bufs: field name -> C-contiguous numpy array of GUARD + Q * n + GUARD rows, written in
#       place from row `lead` on; a field that is absent is passed as NULL
#   dev.status_clear(shape) -> the sticky status word, cleared
#   dev.spills(shape) -> the spill counter
#   dev.step(shape, board, rng, actions) -> (board, rng, reward, n_new, n_act, flags) of one
#       tmg_step(autoreset = 0, trust_eff = 0) on copies
def row_shapes(F, R, C):
    return {"frames": ((F, 2, R, C), np.int8), "kind": ((F,), np.uint8), "frame_elim": ((F,), np.int32),
            "n_frames": ((), np.int32), "reward": ((), np.int32), "n_new": ((), np.int32), "n_act": ((), np.int32),
            "flags": ((), np.uint8), "out_rng": ((5,), np.uint64)}


def trace(dev, shape, board, rng, eff, trust_eff, actions, stage_mask, max_frames, stop=0, fields=FIELDS):
    """One tmg_trace call on `dev`, every array between GUARD rows of FILL
    bytes in front and behind: asserts that no guard byte changed and returns
    the rows in between, (Q, n, ...) per field."""
    R, C = shape[:2]
    actions = np.ascontiguousarray(actions, np.int32)
    Q, n = actions.shape
    rows = row_shapes(max_frames, R, C)
    bufs = {}
    for f in fields:
        rs, dt = rows[f]
        a = np.zeros((GUARD + Q * n + GUARD, *rs), dt)
        a.view(np.uint8).reshape(-1)[:] = FILL_BYTE
        bufs[f] = a
    ins = [np.ascontiguousarray(board, np.int8).copy(), np.ascontiguousarray(rng, np.uint64).copy(), actions.copy(),
           None if eff is None else np.ascontiguousarray(eff, np.uint64).copy()]
    before = [None if x is None else x.copy() for x in ins]
    dev.run(shape, ins[0], ins[1], ins[3], trust_eff, ins[2], stage_mask, max_frames, stop, bufs, GUARD)
    for x, y in zip(ins, before):
        assert x is None or np.array_equal(x, y), "an input was written"
    out = {}
    for f in fields:
        raw = bufs[f].view(np.uint8).reshape(bufs[f].shape[0], -1)
        assert (raw[:GUARD] == FILL_BYTE).all(), f"{f}: written in front of the first row"
        assert (raw[GUARD + Q * n:] == FILL_BYTE).all(), f"{f}: written behind the last row"
        out[f] = bufs[f][GUARD:GUARD + Q * n].reshape(Q, n, *rows[f][0])
    return out


def masks_of(board):
    from rollout_cases import pack_mask
    return np.stack([pack_mask(orc.effective_mask(b)[0]) for b in board])


def check_fields(dev, shape):
    """Every field of whole moves against the walk; with frames = NULL the same small arrays."""
    board, rng, acts, want = field_case(shape)
    dev.status_clear(shape)
    got = trace(dev, shape, board, rng, masks_of(board), 1, acts, ALL_STAGES, WHOLE)
    assert_trace_equal(got, want, str(shape))
    A = orc.num_actions(*shape[:2])
    assert dev.status_clear(shape) == (STATUS_CALLER if (acts >= A).any() else 0)
    assert (want["n_frames"][0] >= 4).all(), "row 0 holds an ineffective action"
    small = trace(dev, shape, board, rng, None, 0, acts, ALL_STAGES, WHOLE, fields=SMALL)
    assert_trace_equal(small, want, f"{shape} frames=NULL, untrusted", SMALL)
    dev.status_clear(shape)


def check_step(dev, shape):
    """The last frame and the sums of row 0 (an effective action per env) equal a real step on a copy."""
    board, rng, acts, want = field_case(shape)
    got = trace(dev, shape, board, rng, masks_of(board), 1, acts[:1], ALL_STAGES, WHOLE)
    sb, sg, rew, nn, na, fl = dev.step(shape, board, rng, acts[0])
    for i in range(board.shape[0]):
        nf = int(got["n_frames"][0, i])
        assert 0 < nf <= WHOLE
        assert np.array_equal(got["frames"][0, i, nf - 1], sb[i]), f"{shape} env {i}: last frame vs the stepped board"
    assert np.array_equal(got["out_rng"][0], sg)
    for f, w in (("reward", rew), ("n_new", nn), ("n_act", na)):
        assert np.array_equal(got[f][0], w), f
    assert np.array_equal(got["flags"][0] & (FLAG_COMBO | FLAG_SHUFFLED | FLAG_ERROR), fl & (FLAG_COMBO | FLAG_SHUFFLED | FLAG_ERROR))
    assert np.array_equal(got["frame_elim"][0].sum(axis=1) + got["n_new"][0], got["reward"][0])
    dev.status_clear(shape)


def check_cut(dev, shape, stage_mask, max_frames):
    """A stage mask and a cut: stop = 0 counts every selected stage and reports
    the whole move; stop = 1 is the prefix of the walk."""
    board, rng, acts, whole = field_case(shape)
    eff = masks_of(board)
    k, sm = shape[2:]
    for stop in (0, 1):
        want = expected(board, rng, acts, k, sm, stage_mask, max_frames, stop)
        got = trace(dev, shape, board, rng, eff, 1, acts, stage_mask, max_frames, stop)
        assert_trace_equal(got, want, f"{shape} mask={stage_mask:#x} F={max_frames} stop={stop}")
        if not stop:
            for f in ("reward", "n_new", "n_act", "flags", "out_rng"):
                assert np.array_equal(want[f], whole[f]), f
            sel = np.isin(whole["kind"], [s for s in KINDS if (stage_mask >> s) & 1]).sum(axis=2)
            assert np.array_equal(want["n_frames"], sel)
        elif stage_mask == 1 << FALL and max_frames == 1:          # the afterstate form
            on = want["n_frames"] == 1
            assert on.any() and (got["flags"][on] & FLAG_STOPPED).all()
            assert np.array_equal(got["out_rng"], np.broadcast_to(rng, got["out_rng"].shape)), "a draw was made"
            first = (whole["kind"] == FALL).argmax(axis=2)
            for q, i in zip(*np.nonzero(on)):
                assert np.array_equal(got["frames"][q, i, 0], whole["frames"][q, i, first[q, i]])
    dev.status_clear(shape)


def check_adversarial(dev, shape, mode, many):
    """Hand-written boards, trust_eff = 0 and eff = NULL: the mask is scanned,
    the whole board searched for lines, and a row that outgrows the LDS lists
    is re-run whole by the spill pass."""
    R, C, k, sm = shape
    n = peek_cases.MANY_SPILLS[shape][0] if many else peek_cases.envs_of(shape)
    b, words, acts = adversarial_case(shape, mode, n)
    want = expected(b, words, acts, k, sm, ALL_STAGES, WHOLE, 0)
    dev.status_clear(shape)
    s0 = dev.spills(shape)
    got = trace(dev, shape, b, words, None, 0, acts, ALL_STAGES, WHOLE)
    assert_trace_equal(got, want, f"{shape} {mode}")
    assert dev.status_clear(shape) == 0
    if mode == "combo_grid":
        assert (want["kind"][0, :, 1] == COMBO).all()
    if (R, C) in ((20, 20), (10, 10)) and mode != "stripes":
        assert dev.spills(shape) > s0, "the adversarial boards were meant to outgrow the LDS lists"
    if many:
        assert dev.spills(shape) - s0 > peek_cases.SPILL_WAVES
    # a stopped row that spills: the afterstate of the same boards
    want = expected(b, words, acts, k, sm, 1 << FALL, 1, 1)
    got = trace(dev, shape, b, words, None, 0, acts, 1 << FALL, 1, 1)
    assert_trace_equal(got, want, f"{shape} {mode} afterstate")
    dev.status_clear(shape)


def check_extent(dev, shape, n, seqs):
    """Nothing outside the rows is written (trace() checks the guard rows);
    frame slots from min(n_frames, max_frames) on keep the fill, kind and
    frame_elim there are 0; frames = NULL gives the same small arrays."""
    board, rng, acts = extent_state(shape, n)
    acts = acts[:seqs]
    k, sm = shape[2:]
    for stop in (0, 1):
        want = expected(board, rng, acts, k, sm, DEFAULT_STAGES, EXTENT_FRAMES, stop)
        got = trace(dev, shape, board, rng, masks_of(board), 1, acts, DEFAULT_STAGES, EXTENT_FRAMES, stop)
        assert_trace_equal(got, want, f"{shape} n={n} seqs={seqs} stop={stop}")
        small = trace(dev, shape, board, rng, masks_of(board), 1, acts, DEFAULT_STAGES, EXTENT_FRAMES, stop, fields=SMALL)
        assert_trace_equal(small, want, f"{shape} n={n} seqs={seqs} stop={stop} frames=NULL", SMALL)
    short = want["n_frames"] < EXTENT_FRAMES
    assert short.any(), "no row leaves a frame slot unwritten"
    dev.status_clear(shape)
