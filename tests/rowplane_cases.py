"""Shared by tests/test_rowplane_emulated.py and tests/test_gpu_rowplane.py: the
shapes of the row-plane lean cascade (tmg_rp.hip: lean kernels, R <= 16,
C <= 28), and 10x10 k4 boards whose next move shows one feature of that
cascade each.  Expected results are always the oracle's; `trace_move` replays
a move with the oracle's own primitives (get_colour_lines, gravity,
rng_colours) so that a test can assert the feature really occurs."""
import numpy as np

# R, C, k: one to three colour planes, even / odd C, k with (3, 5, 6, 7) and
# without (4) Lemire rejections, the R = 16 and C = 28 limits
SHAPES = [(4, 4, 3), (5, 6, 7), (10, 10, 4), (10, 10, 5), (16, 8, 4), (3, 28, 6)]
INJECTED = [(10, 10, 5), (5, 6, 7)]     # rollouts with crafted rejections in the refill range
MOVES = 10
STEPS = 40
FIELDS = ("board", "rng", "timer", "eff", "reward", "n_new", "n_act", "flags")

R10 = C10 = 10
K10 = 4


def action_cells(R, C, a):
    if a < C * (R - 1):
        return (a // C, a % C), (a // C + 1, a % C)
    i = a - C * (R - 1)
    return (i // (C - 1), i % (C - 1)), (i // (C - 1), i % (C - 1) + 1)


def vaction(r, c, C=C10):               # swap (r, c) with (r + 1, c)
    return r * C + c


def haction(r, c, R=R10, C=C10):        # swap (r, c) with (r, c + 1)
    return C * (R - 1) + r * (C - 1) + c


def trace_move(orc, board, rng, action, k):
    """Board.move (board.py:355-376) of a no-specials board with the oracle's
    primitives: per cascade iteration the lines get_colour_lines returns.
    Returns (iterations, final board, rng); the caller compares the last two
    with orc.move, which validates the trace itself."""
    b = np.array(board, dtype=np.int8).copy()
    rng = np.array(rng, dtype=np.uint64).copy()
    _, R, C = b.shape
    (r1, c1), (r2, c2) = action_cells(R, C, action)
    b[:, r1, c1], b[:, r2, c2] = b[:, r2, c2].copy(), b[:, r1, c1].copy()
    its = []
    while True:
        lines = orc.get_colour_lines(b, k, 0)
        if not lines:
            break
        its.append(lines)
        for ln in lines:
            for r, c in ln:
                b[:, r, c] = 0
        b = orc.gravity(b)
        holes = np.argwhere(b[1] == 0)                      # row-major
        cols, rng = orc.rng_colours(rng, k, len(holes))
        for (r, c), x in zip(holes, cols):
            b[0, r, c] = x
            b[1, r, c] = 1
    return its, b, rng


def _vertical(ln):
    return len({c for _, c in ln}) == 1


def _horizontal(ln):
    return len({r for r, _ in ln}) == 1


def _crossings(lines):
    """(vertical line, horizontal line, shared cell) of one iteration."""
    out = []
    for v in lines:
        for h in lines:
            if _vertical(v) and _horizontal(h):
                for cell in set(v) & set(h):
                    out.append((sorted(v), sorted(h), cell))
    return out


def _cleared(lines):
    return {cell for ln in lines for cell in ln}


# feature name -> predicate over the iterations of trace_move
def f_two_horizontal(its):
    return any(sum(1 for ln in lines if _horizontal(ln) and ln[0][0] == max(r for l in lines for r, _ in l)) >= 2
               for lines in its)


def f_vertical5_bottom(its, R=R10):
    return any(_vertical(ln) and len(ln) >= 5 and max(r for r, _ in ln) == R - 1 for lines in its for ln in lines)


def _cross(its, where_v, where_h):
    for lines in its:
        bottom = max(r for ln in lines for r, _ in ln)
        for v, h, cell in _crossings(lines):
            if cell[0] >= bottom:
                continue                                    # the crossing is above the bottom row
            iv, ih = v.index(cell), h.index(cell)
            top, mid_v = iv == 0, 0 < iv < len(v) - 1
            end_h, mid_h = ih in (0, len(h) - 1), 0 < ih < len(h) - 1
            if (where_v == "top" and top or where_v == "mid" and mid_v) and (where_h == "mid" and mid_h or where_h == "end" and end_h):
                return True
    return False


def f_T(its):
    return _cross(its, "top", "mid")


def f_L(its):
    return _cross(its, "top", "end")


def f_plus(its):
    return _cross(its, "mid", "mid")


def f_two_holes(its):
    for lines in its:
        cl = _cleared(lines)
        for c in {c for _, c in cl}:
            rows = sorted(r for r, cc in cl if cc == c)
            if any(b - a > 1 for a, b in zip(rows, rows[1:])):
                return True
    return False


def f_row0(its):
    return any(r == 0 for lines in its for r, _ in _cleared(lines))


def f_last_col(its, C=C10):
    return any(c == C - 1 for lines in its for _, c in _cleared(lines))


def f_six(its):
    return len(its) >= 6


FEATURES = {
    "two_horizontal_same_row": (f_two_horizontal, None),
    "vertical_5_bottom": (f_vertical5_bottom, "rp_vlong"),
    "T_cross": (f_T, "rp_perp"),
    "L_cross": (f_L, "rp_perp"),
    "plus_cross": (f_plus, "rp_perp"),
    "column_two_holes": (f_two_holes, "rp_passes"),
    "touches_row_0": (f_row0, None),
    "last_column": (f_last_col, None),
    "six_iterations": (f_six, None),
}


def _bg():
    """No line and no effective move: 1 + (r + c) % 4 differs from every cell at distance 1 and 2 in its row and column."""
    r, c = np.mgrid[0:R10, 0:C10]
    return (1 + (r + c) % 4).astype(np.int8)


def _rows(s):
    return np.array([[int(x) for x in row] for row in s.split()], np.int8)


def crafted():
    """name -> (colour plane (10, 10) int8, action, seed of the env's stream or its five state words)."""
    out = {}
    b = _bg()                                   # row 9: . 1 1 3 1 3 3 . -> swap (9,3),(9,4)
    b[9, 1:7] = [1, 1, 3, 1, 3, 3]
    b[9, 0], b[9, 7] = 2, 4
    b[8, 1:7] = [2, 4, 2, 4, 2, 4]
    out["two_horizontal_same_row"] = (b, haction(9, 3), 1)
    b = _bg()                                   # column 4: rows 5, 6, 8, 9 hold 2; (7,5) brings the fifth
    b[[5, 6, 8, 9], 4] = 2
    b[7, 4], b[7, 5], b[4, 4] = 3, 2, 1
    b[7, 6], b[6, 5], b[8, 5] = 4, 1, 1
    out["vertical_5_bottom"] = (b, haction(7, 4), 2)
    b = _bg()                                   # vertical rows 5..7 in column 4, its top cell comes from (4,4); run (5,3) (5,5)
    b[6, 4] = b[7, 4] = b[4, 4] = b[5, 3] = b[5, 5] = 3
    b[5, 4], b[3, 4], b[8, 4], b[5, 2], b[5, 6] = 1, 1, 1, 4, 4
    out["T_cross"] = (b, vaction(4, 4), 3)
    b = _bg()                                   # the same with the run to the right only: (5,5) (5,6)
    b[6, 4] = b[7, 4] = b[4, 4] = b[5, 5] = b[5, 6] = 3
    b[5, 4], b[3, 4], b[8, 4], b[5, 3], b[5, 7] = 1, 1, 1, 4, 4
    out["L_cross"] = (b, vaction(4, 4), 4)
    # plus: a vertical run of 4s in column 4 (rows 4..6, completed from (4,3)) goes; rows 2, 3 of the
    # column drop onto (7,4): a vertical line of 2s in rows 5..7 whose middle cell meets (6,3), (6,5)
    b = _bg()
    b[5, 4] = b[6, 4] = b[4, 3] = 4
    b[4, 4] = 1
    b[2, 4] = b[3, 4] = b[7, 4] = b[6, 3] = b[6, 5] = 2
    b[1, 4], b[8, 4], b[6, 2], b[6, 6], b[3, 3], b[3, 5] = 3, 3, 1, 1, 1, 3
    out["plus_cross"] = (b, haction(4, 3), 5)
    b = _bg()                                   # vertical rows 0..2 in column 7, completed from (2,8)
    b[0, 7] = b[1, 7] = b[2, 8] = 4
    b[2, 7], b[3, 7], b[1, 8], b[3, 8] = 1, 2, 1, 1
    out["touches_row_0"] = (b, haction(2, 7), 6)
    b = _bg()                                   # run (9,7) (9,8) completed in the last column from (8,9)
    b[9, 7] = b[9, 8] = b[8, 9] = 3
    b[9, 9], b[9, 6], b[7, 9], b[8, 8] = 1, 2, 4, 4
    out["last_column"] = (b, vaction(8, 9), 7)
    out["six_iterations"] = (out["T_cross"][0], out["T_cross"][1], 3)      # 12 iterations with this stream
    out["column_two_holes"] = (_rows(TWO_HOLES), 65, TWO_HOLES_RNG)
    return out


# Taken from an oracle rollout with its stream: in a later iteration of this
# move's cascade a column loses two cells that are not neighbours (a run in the
# bottom row of the lines and a crossing run above it).  One swap on a line-free
# board never does that in the first iteration (searched: 10^5 effective moves).
TWO_HOLES = ("2334424314 3321233443 1432431231 4424313134 2133223422 3123421412 3441232141 4221122411 "
             "3442414142 3131424344")
TWO_HOLES_RNG = (0x2035c5b5ac1f8316, 0x95a2b0f75243bca5, 0x7762b99bc055c961, 0x58912860c49791d1, 0x17f2e1fd)


def stream_words(seed):
    from tile_match_gym_amd.seeding import batch_rng_words
    if isinstance(seed, tuple):
        return np.array(seed, dtype=np.uint64)
    return batch_rng_words([seed])[0]
