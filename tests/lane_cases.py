"""Shared by tests/test_lane_host.py and tests/test_gpu_lane.py: 10x10 states
on which the lane-per-board step (csrc/tmg_lane.h) takes its rare branches.

Random play on 10x10 boards with 4 or 5 colours practically never shuffles, so
the boards are crafted.  A pattern board colour(r, c) = (a r + b c) mod k + 1
(every tile normal) has no line and no effective action for the (a, b) below.
A candidate changes three of its cells so that one vertical swap completes a
horizontal triple X X X in row 0: gravity then moves nothing, the three refill
draws decide the board, and when they leave it moveless again the move
shuffles all 100 cells and redraws rows until the board is line-free and
playable (board.py:381-391).  Which envs do so is always the oracle's word:
the tests assert its flags, never the device's.
"""
import functools

import numpy as np

from oracle import oracle as orc

R = C = 10
A = 2 * R * C - R - C
SEED0 = 1000                # env i is seeded SEED0 + i
KEY = 4242                  # the policy's key
FIELDS = ("board", "rng", "timer", "eff", "reward", "n_new", "n_act", "flags")
# (a, b) of the moveless, line-free pattern boards
PATTERNS = {4: [(1, 1), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2), (3, 3)],
            5: [(a, b) for a in range(1, 5) for b in range(1, 5)]}
CANDIDATES = {4: 272, 5: 856}               # boards candidates(k) keeps
# envs of a 2048-env crafted batch whose first trusted move must shuffle (on the oracle)
MIN_SHUFFLED = {4: 16, 5: 128}


def pattern(a, b, k):
    r, c = np.mgrid[0:R, 0:C]
    return ((a * r + b * c) % k + 1).astype(np.int8)


def raw_candidates(k):
    """Every board the construction gives, before the oracle's filter."""
    out = []
    for a, b in PATTERNS[k]:
        P = pattern(a, b, k)
        for c in range(C - 2):
            for X in range(1, k + 1):
                for mirror in (False, True):
                    pair, lone = ((c + 1, c + 2), c) if mirror else ((c, c + 1), c + 2)
                    Y = P[1, lone]
                    if X == Y:
                        continue
                    B = P.copy()
                    B[0, pair[0]] = B[0, pair[1]] = X
                    B[0, lone] = Y
                    B[1, lone] = X
                    out.append(np.stack([B, np.ones_like(B)]))
    return out


@functools.lru_cache(maxsize=None)
def candidates(k):
    """(boards (m, 2, R, C) int8, idle (m,) int32): the candidates the oracle
    finds line-free with at least one effective action, and the first
    ineffective action of each."""
    keep, idle = [], []
    for B in raw_candidates(k):
        mask, playable = orc.effective_mask(B)
        if orc.get_colour_lines(B, k, 0) == [] and playable:
            keep.append(B)
            idle.append(int(np.nonzero(~mask)[0][0]))
    boards, idle = np.stack(keep), np.array(idle, np.int32)
    boards.setflags(write=False)
    idle.setflags(write=False)
    return boards, idle


def crafted_batch(k, n):
    """The candidates cycled over n envs: (boards, fresh PCG64 words, idle actions)."""
    from tile_match_gym_amd.seeding import batch_rng_words
    boards, idle = candidates(k)
    i = np.arange(n) % boards.shape[0]
    return boards[i].copy(), batch_rng_words(range(SEED0, SEED0 + n)), idle[i].copy()


def crafted_oracle(k, n, num_moves=30, threads=16):
    """The oracle on the crafted batch, before the idle step: (OracleBatch, idle actions)."""
    boards, words, idle = crafted_batch(k, n)
    o = orc.OracleBatch(R, C, k, 0, num_moves, words, threads=threads)
    o.board[:] = boards
    return o, idle


def redraw_positions(n, seed):
    """Draw positions of the crafted rejections on the crafted states: past
    the refill (3 draws) and the shuffle (>= 99), in the redraws after it."""
    rs = np.random.default_rng(seed)
    return rs.integers(100, 401, n), rs.random(n) < 0.5
