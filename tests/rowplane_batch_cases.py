"""Shared by tests/test_rowplane_batch_emulated.py and
tests/test_gpu_rowplane_batch.py: moves that exercise the move-level colour
batch of the row-plane cascade (tmg_rp.hip, RpBatch) — iterations served from
a batch an earlier iteration drew from, a second batch within one move, and
Lemire rejections inside and just beyond the colours a move takes.  Every case
is chosen with the oracle's own trace of the move (rowplane_cases.trace_move);
expected results are always the oracle's."""
import numpy as np

from rejection_states import words_rejecting_at
from rowplane_cases import K10, crafted, stream_words, trace_move

BATCH = 128                              # colours of one batch, a buffered half-word included
CARRY_BOARDS = ("six_iterations", "column_two_holes", "plus_cross")
BUF_VALUES = (0x9ABCDEF0, 0x13572468, 0x5A5A5A5A, 0xC0FFEE11, 0x2468ACE0, 0xFEDCBA98, 0x0F1E2D3C, 0x7B7B7B7B)
WIDE_SHAPES = [(16, 8, 4), (3, 28, 6)]     # 128 and 84 cells
REJECT_SHAPES = [(10, 10, 5), (5, 6, 7)]
ROLLOUT_POSITIONS = 16                   # injected rejections at draw indices 0..15


def draws(its):
    """Colours drawn per cascade iteration: the cells its lines clear."""
    return [len({c for ln in lines for c in ln}) for lines in its]


def bookkeeping(ts):
    """(iterations served from a carried batch, batches after the first) of a
    move drawing ts colours per iteration without a rejection: a batch holds
    BATCH colours and an iteration that needs more than is left starts a new one."""
    left, used, carry, again = BATCH, 0, 0, 0
    for t in ts:
        if left < t:
            again += 1
            left, used = BATCH, 0
        elif used:
            carry += 1
        left -= t
        used += t
    return carry, again


def with_buffered(words, v):
    w = np.array(words, dtype=np.uint64).copy()
    w[..., 4] = np.uint64((1 << 32) | v)
    return w


def carry_cases(orc):
    """[(name, board (2, 10, 10), action, state words)]: the crafted boards as
    seeded and with a buffered half-word (the first of BUF_VALUES with which
    the move still cascades past its first iteration)."""
    out = []
    cs = crafted()
    for nm in CARRY_BOARDS:
        col, a, seed = cs[nm]
        b = np.stack([col, np.ones_like(col)]).astype(np.int8)
        w = stream_words(seed)
        assert len(trace_move(orc, b, w, a, K10)[0]) >= 2, nm
        out.append((nm, b, a, w))
        for v in BUF_VALUES:
            wb = with_buffered(w, v)
            if len(trace_move(orc, b, wb, a, K10)[0]) >= 2:
                out.append((nm + "+buffered", b, a, wb))
                break
        else:
            raise AssertionError(f"{nm}: no buffered half-word of BUF_VALUES keeps the cascade going")
    return out


def striped_board(R, C):
    """Every column one colour from top to bottom (test_wide_refill_emulated):
    the first cascade iteration clears (nearly) the whole board."""
    col = np.tile((1 + np.arange(C) % 2).astype(np.int8), (R, 1))
    return np.stack([col, np.ones_like(col)])


def mask_words(mask):
    A = mask.size
    return np.packbits(np.pad(mask, (0, -A % 64)).reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()


def rebatch_cases(orc, shape, n=8, first_seed=40, tries=400):
    """(board, cached mask words, actions (n,), state words (n, 5)): n streams
    (every other one with a buffered half-word) whose move from the striped
    board cascades past its first iteration and, where the board has more
    cells than the batch has colours left after them (16x8: all 128 go in the
    first iteration), outruns its first batch.  The 84 cells of 3x28 leave 44
    colours, which no cascade found in 4000 streams uses up: there the later
    iterations are served from the batch after a refill of more than 64."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k = shape
    b = striped_board(R, C)
    mask = orc.effective_mask(b)[0]
    eff = np.nonzero(mask)[0]
    ws, acts = [], []
    for seed in range(first_seed, first_seed + tries):
        j = len(ws)
        w = batch_rng_words([seed])[0]
        if j % 2 == 1:
            w = with_buffered(w, BUF_VALUES[j % len(BUF_VALUES)])
        a = int(eff[j * 3 % eff.size])
        ts = draws(trace_move(orc, b, w, a, k)[0])
        if len(ts) >= 2 and (bookkeeping(ts)[1] > 0 or R * C < BATCH):
            ws.append(w)
            acts.append(a)
            if len(ws) == n:
                return b, mask_words(mask), np.array(acts, np.int32), np.stack(ws)
    raise AssertionError(f"{shape}: {len(ws)} of {n} re-batching moves in {tries} streams")


def rejection_cases(orc, shape, n=8, first_seed=900, envs=256):
    """From reset boards of `shape` (k with Lemire rejections) and each env's
    first effective action: (inside, beyond), each (env indices, actions, state
    words) of n envs, half with a buffered half-word.  inside: the rejected
    word is one the move's second iteration draws.  beyond: the rejected word
    is the first one the move does not draw (the move itself draws none)."""
    from tile_match_gym_amd.seeding import batch_rng_words
    R, C, k = shape
    o = orc.OracleBatch(R, C, k, 0, 30, batch_rng_words(range(first_seed, first_seed + envs)))
    o.reset()
    A = 2 * R * C - R - C
    inside, beyond = [], []
    for i in range(envs):
        m = np.unpackbits(o.eff[i].view(np.uint8), bitorder="little")[:A]
        if not m.any():
            continue
        a = int(np.nonzero(m)[0][0])
        t1 = draws(trace_move(orc, o.board[i], o.rng[i], a, k)[0])[0]      # the first iteration ignores the stream
        for want, buf in ((inside, len(inside) % 2 == 1), (beyond, len(beyond) % 2 == 1)):
            if len(want) == n:
                continue
            for p in range(t1, t1 + 24):
                w = words_rejecting_at(o.rng[i:i + 1], [p], buffered=[buf])[0]
                ts = draws(trace_move(orc, o.board[i], w, a, k)[0])
                ok = (len(ts) >= 2 and p < t1 + ts[1]) if want is inside else (sum(ts) == p)
                if ok:
                    want.append((i, a, w))
                    break
        if len(inside) == n and len(beyond) == n:
            break
    assert len(inside) == n and len(beyond) == n, (shape, len(inside), len(beyond))

    def pack(cs):
        return (np.array([c[0] for c in cs]), np.array([c[1] for c in cs], np.int32), np.stack([c[2] for c in cs]))
    return o, pack(inside), pack(beyond)
