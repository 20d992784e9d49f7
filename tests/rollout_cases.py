"""The oracle side of the tmg_rollout tests (tests/test_rollout_emulated.py on
the host wave emulator, tests/test_gpu_rollout.py on the device).

The expected values come from the oracle only: rollout (s, i, a) plays a with
oracle.move on a copy of board i and of the RNG words rng[s][i], then for ply
d = 1 .. H - 1 the action oracle.policy_np.sample_effective_np draws from
oracle.effective_mask of the board the ply before left, with key
(key + s * A + a) mod 2^64, global env first_env + i and step counter t + d.
H = min(depth, num_moves - timer[i]), or depth without a timer."""
import numpy as np

import peek_cases
from oracle import oracle as orc
from oracle.policy_np import sample_effective_np

FLAG_COMBO, FLAG_SHUFFLED, FLAG_ERROR = peek_cases.FLAG_COMBO, peek_cases.FLAG_SHUFFLED, peek_cases.FLAG_ERROR
FIELDS = ("ret", "plies", "flags", "total", "best_action", "best_total")
KEY, FIRST_ENV, T = 99, 5, 11


def pack_mask(mask):
    """(A,) bool -> (W,) uint64, action a at bit a & 63 of word a >> 6."""
    W = (mask.size + 63) // 64
    bits = np.zeros(W * 64, np.uint8)
    bits[:mask.size] = mask
    return np.packbits(bits, bitorder="little").view(np.uint64)


def oracle_rollout(board, rng, timer, num_moves, k, smask, depth, samples, key, first_env, t, shuffled_at=None):
    """board (n, 2, R, C) int8, rng (samples, n, 5) uint64, timer (n,) int32 or
    None -> dict of ret / plies (S, n, A) int32, flags (S, n, A) uint8, total
    (n, A), best_action / best_total (n,) int32.  The inputs are not changed.
    shuffled_at: a list that receives the ply index d of every shuffled move."""
    n, _, R, C = board.shape
    A = orc.num_actions(R, C)
    rng = np.asarray(rng, np.uint64).reshape(samples, n, 5)
    ret = np.zeros((samples, n, A), np.int32)
    plies = np.zeros((samples, n, A), np.int32)
    flags = np.zeros((samples, n, A), np.uint8)
    for i in range(n):
        H = depth if timer is None else min(depth, num_moves - int(timer[i]))
        if H <= 0:
            continue
        eff0, _ = orc.effective_mask(board[i])
        for s in range(samples):
            for a in np.nonzero(eff0)[0]:
                b, g, act = board[i], rng[s, i], int(a)
                for d in range(H):
                    if d > 0:
                        m, _ = orc.effective_mask(b)
                        act = int(sample_effective_np(pack_mask(m)[None], A, (key + s * A + int(a)) % 2 ** 64,
                                                      first_env + i, t + d)[0])
                    b, g, res, err = orc.move(b, g, act, k, smask)
                    assert err == 0, (s, i, int(a), d, err)
                    ret[s, i, a] += int(res[0])
                    plies[s, i, a] += 1
                    flags[s, i, a] |= (FLAG_COMBO if res[1] else 0) | (FLAG_SHUFFLED if res[4] else 0)
                    if res[4] and shuffled_at is not None:
                        shuffled_at.append(d)
    total = ret.sum(axis=0).astype(np.int32)
    return {"ret": ret, "plies": plies, "flags": flags, "total": total,
            "best_action": total.argmax(axis=1).astype(np.int32),          # the first of the maxima
            "best_total": total.max(axis=1).astype(np.int32)}


def assert_rollout_equal(got, want, what="", fields=FIELDS):
    for f in fields:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(np.asarray(got[f]) != np.asarray(want[f]))[:5]
            raise AssertionError(f"{what}: {f} differs at {bad.tolist()}: "
                                 f"got {[int(got[f][tuple(b)]) for b in bad]}, "
                                 f"want {[int(want[f][tuple(b)]) for b in bad]}")


def horizon_timers(o, finished=True):
    """The test's timers on OracleBatch o: env 0 two moves from the end and
    (finished) the last env at the end of its episode."""
    timer = o.timer.copy()
    timer[0] = o.num_moves - 2
    if finished:
        timer[-1] = o.num_moves
    return timer
