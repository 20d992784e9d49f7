"""The special-tile matrix: hand-built moves that cover every ordered pair of
tiles that takes the combination branch (board.py:357-361, :600-719) at every
border distance, every passive activation chain (board.py:473-556) and the
cookie's "most common colour" rule, on the smallest shape of every general
kernel family.

Pure data and numpy: nothing here imports the reference, the oracle or the
library.  tests/golden/make_special_matrix.py records the reference's outputs
for these boards into tests/golden/matrix_<shape>.npz; tests/test_special_matrix.py
(oracle, host wave emulator) and tests/test_gpu_special_matrix.py (device) play
the recorded rows.  A row of a fixture is (cell index, attempt): board_of(shape,
cell index, attempt) rebuilds its input board and action.

Tile kinds: N normal, V vertical laser, H horizontal laser, B bomb, K colourless
cookie (type -1, colour 0), Kc coloured cookie (type -1, colour != 0; reachable
through remove_colour_lines, board.py:128-129, which redraws the colour plane
under a cookie).
"""
import functools
import os

import numpy as np

N, V, H, B, K, KC = "N", "V", "H", "B", "K", "Kc"
KINDS = (N, V, H, B, K, KC)
TYPE_OF = {N: 1, V: 2, H: 3, B: 4, K: -1, KC: -1}
BIT_OF = {V: 2, H: 4, B: 8, K: 1, KC: 1}
CLEAN, SEEDED = 0, 1
BG_NAMES = ("clean", "seeded")
P_SEEDED = 0.15                  # other specials on a seeded background
ROW_PAIR, ROW_CHAIN, ROW_COOKIE = 0, 1, 2
# crafted cookie rows
TIE, SPECIAL_MAJORITY, MID_CHAIN, MID_CHAIN_REVERSED, NONE_LEFT = 1, 2, 3, 4, 5
COOKIE_TAGS = (TIE, SPECIAL_MAJORITY, MID_CHAIN, MID_CHAIN_REVERSED, NONE_LEFT)

# (R, C, colours, specials mask): the smallest shapes that reach each general
# kernel family (tests/test_special_matrix.py checks the list against the
# dispatch rule)
SHAPES = [
    (10, 10, 4, 14),             # the fixed v/h-laser + bomb kernel
    (20, 20, 6, 15),             # the fixed all-specials 512-cell kernel
    (6, 6, 4, 15),               # bitboard, even C
    (5, 5, 3, 15),               # bitboard, odd C
    (7, 9, 10, 15),              # four colour planes
    (2, 64, 4, 15),              # no bitboard (C = 64)
    (3, 43, 5, 15),              # the generic 512-cell kernel
]
# 20x20: a seeded background carries one colour relation per position (they
# alternate), so that the fixture stays within the size of a committed file;
# every pair x orientation x position cell keeps both backgrounds.
THIN_SEEDED = {(20, 20, 6, 15)}


def shape_id(shape):
    R, C, k, sm = shape
    return f"{R}x{C}k{k}s{sm}"


def enabled_kinds(smask):
    return [x for x in (V, H, B, K, KC) if smask & BIT_OF[x]]


def kind_at(board, r, c):
    t, col = int(board[1, r, c]), int(board[0, r, c])
    if t == -1:
        return KC if col else K
    return {1: N, 2: V, 3: H, 4: B}[t]


def geometric(k1, k2):
    return k1 in (V, H, B) and k2 in (V, H, B)


def ordered_pairs(smask):
    """(tile at the action's first coordinate, tile at its second) of every move
    that takes the combination branch: both special, or at least one cookie."""
    ks = [N] + enabled_kinds(smask)
    return [(a, b) for a in ks for b in ks if (a != N and b != N) or a in (K, KC) or b in (K, KC)]


def action_of(R, C, r, c, vertical):
    """The action that swaps (r, c) with the cell below it / right of it (board.py:80-91)."""
    return r * C + c if vertical else C * (R - 1) + r * (C - 1) + c


def cells_of(R, C, a):
    if a < C * (R - 1):
        r, c = divmod(a, C)
        return (r, c), (r + 1, c)
    r, c = divmod(a - C * (R - 1), C - 1)
    return (r, c), (r, c + 1)


def line_class(i, n):
    """Distance of index i to both borders of an axis of n cells: 0, 1, or 2 for more."""
    return (min(i, 2), min(n - 1 - i, 2))


def place_class(r, c, R, C):
    on_r, on_c = r in (0, R - 1), c in (0, C - 1)
    return "corner" if on_r and on_c else "edge" if on_r or on_c else "interior"


def edge_class(r, c, R, C):
    """corner / top / bottom / left / right / interior of a single cell."""
    on_r, on_c = r in (0, R - 1), c in (0, C - 1)
    if on_r and on_c:
        return "corner"
    if on_r:
        return "top" if r == 0 else "bottom"
    if on_c:
        return "left" if c == 0 else "right"
    return "interior"


def _reps(n, limit):
    """One index per line_class over 0 .. limit - 1 of an axis of n cells: the
    member nearest to the middle of the class."""
    by = {}
    for i in range(limit):
        by.setdefault(line_class(i, n), []).append(i)
    return {cl: m[(len(m) - 1) // 2] for cl, m in by.items()}


def _place_reps(R, C, vertical):
    """One top-left cell per place_class that the swap admits: the middle member of the class."""
    by = {}
    for r in range(R - 1 if vertical else R):
        for c in range(C if vertical else C - 1):
            by.setdefault(place_class(r, c, R, C), []).append((r, c))
    return {cl: m[len(m) // 2] for cl, m in by.items()}


# ---------------------------------------------------------------- the cells of the matrix
@functools.lru_cache(maxsize=None)
def matrix_cells(shape):
    """Every cell of the matrix of a shape, as tuples:
      ("pair", k1, k2, vertical, same, (r, c), bg)   same: 1 / 0, -1 where not both tiles carry a colour
      ("chain", T, U or None, order, pos or None, bg)  order: 0, 1 U before T in the sweep, 2 after
      ("cookie", tag)
    The index in this list is a row's cell index."""
    R, C, k, sm = shape
    en = enabled_kinds(sm)
    out = []
    for (k1, k2) in ordered_pairs(sm):
        both = k1 != K and k2 != K
        for vertical in (0, 1):
            if geometric(k1, k2):
                rows, cols = _reps(R, R - 1 if vertical else R), _reps(C, C if vertical else C - 1)
                spots = [(r, c) for r in rows.values() for c in cols.values()]
            else:
                spots = list(_place_reps(R, C, vertical).values())
            for j, spot in enumerate(spots):
                for bg in (CLEAN, SEEDED):
                    sames = (1, 0) if both else (-1,)
                    if both and bg == SEEDED and shape in THIN_SEEDED:
                        sames = (j & 1,)
                    for same in sames:
                        out.append(("pair", k1, k2, vertical, same, spot, bg))
    ts = [t for t in en if t != K]                       # a colourless cookie is in no colour line
    for T in ts:
        for pos in ("corner", "top", "bottom", "left", "right", "interior"):
            if chain_pos_admitted(shape, T, pos):
                for bg in (CLEAN, SEEDED):
                    out.append(("chain", T, None, 0, pos, bg))
        for U in en:
            if T == KC and U in (K, KC):
                continue                                  # a cookie activates types > 1 only (board.py:547)
            for order in ((1, 2) if T in (V, H) else (0,)):
                if T == V and R < 2 or T == H and C < 2:
                    continue
                for bg in (CLEAN, SEEDED):
                    out.append(("chain", T, U, order, None, bg))
    if sm & 1:
        out += [("cookie", tag) for tag in COOKIE_TAGS]
    return out


def chain_pos_admitted(shape, T, pos):
    """Whether special T can sit at `pos` inside a line of three that a swap of
    two normal tiles completes.  A coloured cookie is found in a line only
    where it is not the line's first cell (the leftmost of a horizontal line,
    the bottom of a vertical one: board.py:164, :180) nor the cell
    is_move_effective tests for a type (the rightmost, the bottom: :770, :780)."""
    R, C = shape[:2]
    if pos == "interior" and (R < 3 or C < 3):
        return False
    if pos in ("left", "right") and R < 3 or pos in ("top", "bottom") and C < 3:
        return False
    return bool(_chain_candidates(shape, T, _pos_cells(shape, pos)[0]))


def _pos_cells(shape, pos):
    R, C = shape[:2]
    rm, cm = R // 2, C // 2
    return {"corner": [(0, 0), (0, C - 1), (R - 1, 0), (R - 1, C - 1)], "top": [(0, cm)], "bottom": [(R - 1, cm)],
            "left": [(rm, 0)], "right": [(rm, C - 1)], "interior": [(rm, cm)]}[pos]


def _chain_candidates(shape, T, tcell):
    """(line cells sorted, mover, partner) of every way a swap of mover and
    partner (both normal) completes a line of three through tcell."""
    R, C = shape[:2]
    r, c = tcell
    out = []
    for vertical in (0, 1):
        for j in range(3):
            line = [(r + i - j, c) if vertical else (r, c + i - j) for i in range(3)]
            if not all(0 <= a < R and 0 <= b < C for a, b in line):
                continue
            if T == KC and (j == 2 or (not vertical and j == 0)):
                continue
            for m in line:
                if m == tcell:
                    continue
                for d in ((0, 1), (1, 0), (0, -1), (-1, 0)):
                    p = (m[0] + d[0], m[1] + d[1])
                    if p not in line and 0 <= p[0] < R and 0 <= p[1] < C:
                        out.append((line, m, p))
    return out


# ---------------------------------------------------------------- colour planes without lines
def _runs(col):
    """Every window of three equal non-zero colours, as a tuple of its cells."""
    R, C = col.shape
    out = []
    if C >= 3:
        m = (col[:, :-2] == col[:, 1:-1]) & (col[:, 1:-1] == col[:, 2:]) & (col[:, :-2] != 0)
        out += [((r, c), (r, c + 1), (r, c + 2)) for r, c in np.argwhere(m).tolist()]
    if R >= 3:
        m = (col[:-2] == col[1:-1]) & (col[1:-1] == col[2:]) & (col[:-2] != 0)
        out += [((r, c), (r + 1, c), (r + 2, c)) for r, c in np.argwhere(m).tolist()]
    return out


def _repair(col, free, rs, k, allowed=()):
    """Recolour free cells until no window of three but those of `allowed` is left."""
    for _ in range(64):
        bad = [w for w in _runs(col) if w not in allowed]
        if not bad:
            return True
        for w in bad:
            cands = [p for p in w if free[p]]
            if not cands:
                return False
            p = cands[int(rs.integers(len(cands)))]
            for x in (rs.permutation(k) + 1).tolist():
                col[p] = x
                if not any(p in w2 and w2 not in allowed for w2 in _runs(col)):
                    break
    return False


def _background(shape, rs, bg, fixed, allowed=(), special_colour=None, p_seeded=P_SEEDED):
    """(2, R, C) int8: the tiles of `fixed` {cell: (type, colour)}, every other
    cell a normal tile, on a seeded background about P_SEEDED of them another
    enabled special; colours drawn at random, then repaired to hold no line
    (but `allowed`).  None when the repair does not end."""
    R, C, k, sm = shape
    typ = np.ones((R, C), np.int8)
    col = rs.integers(1, k + 1, (R, C)).astype(np.int8)
    free = np.ones((R, C), bool)
    if bg == SEEDED:
        en = enabled_kinds(sm) if special_colour is None else [x for x in enabled_kinds(sm) if x != K]
        sel = rs.random((R, C)) < p_seeded
        kinds = rs.integers(0, len(en), (R, C))
        for r, c in np.argwhere(sel).tolist():
            kind = en[int(kinds[r, c])]
            typ[r, c] = TYPE_OF[kind]
            if kind == K:
                col[r, c], free[r, c] = 0, False
            elif special_colour is not None:
                col[r, c], free[r, c] = special_colour, False
    for (r, c), (t, x) in fixed.items():
        typ[r, c], col[r, c], free[r, c] = t, x, False
    if not _repair(col, free, rs, k, allowed):
        return None
    return np.stack([col, typ]).astype(np.int8)


def _two_colours(rs, k):
    a = int(rs.integers(1, k + 1))
    b = int((a - 1 + rs.integers(1, k)) % k) + 1
    return a, b


# ---------------------------------------------------------------- builders
def _build_pair(shape, cell, rs):
    R, C, k, sm = shape
    _, k1, k2, vertical, same, (r, c), bg = cell
    r2, c2 = (r + 1, c) if vertical else (r, c + 1)
    a, b = _two_colours(rs, k)
    x1 = 0 if k1 == K else a
    x2 = 0 if k2 == K else (a if same == 1 or k1 == K else b if same == 0 else a)
    fixed = {(r, c): (TYPE_OF[k1], x1), (r2, c2): (TYPE_OF[k2], x2)}
    board = _background(shape, rs, bg, fixed)
    if board is None:
        return None
    return board, action_of(R, C, r, c, vertical), (-1, -1)


def _blast(shape, T, tcell, order, taken):
    """Cells special T at tcell reaches (not those of `taken`); for a laser,
    order 1: before tcell in the sweep (board.py:503, :511), 2: after it."""
    R, C = shape[:2]
    r, c = tcell
    if T == V:
        cells = [(i, c) for i in range(R) if (i < r if order == 1 else i > r)]
    elif T == H:
        cells = [(r, j) for j in range(C) if (j < c if order == 1 else j > c)]
    elif T == B:
        cells = [(i, j) for i in range(max(r - 1, 0), min(r + 1, R - 1) + 1)
                 for j in range(max(c - 1, 0), min(c + 1, C - 1) + 1) if (i, j) != tcell]
    else:                                                 # a cookie reaches every tile of the colour it picks
        cells = [(i, j) for i in range(R) for j in range(C) if (i, j) != tcell]
    return [p for p in cells if p not in taken]


def _chain_board(shape, rs, bg, T, tcell, cand, U=None, order=0, special_colour=None, line_colour=None, extra=None,
                 p_seeded=P_SEEDED):
    """The board before the swap, the action, and U's cell, of one candidate; None when it does not fit."""
    R, C, k, sm = shape
    line, mover, partner = cand
    a, b = _two_colours(rs, k)
    if line_colour is not None:
        a = line_colour
        b = a % k + 1
    fixed = {p: (1, a) for p in line}
    fixed[tcell] = (TYPE_OF[T], a)
    fixed[partner] = (1, b)
    ucell = None
    if U is not None:
        spots = _blast(shape, T, tcell, order, set(fixed))
        if not spots:
            return None
        ucell = spots[int(rs.integers(len(spots)))]
        fixed[ucell] = (TYPE_OF[U], 0 if U == K else int(rs.integers(1, k + 1)))
    for p, v in (extra or {}).items():
        if p in fixed:
            return None
        fixed[p] = v
    after = _background(shape, rs, bg, fixed, allowed=(tuple(line),), special_colour=special_colour, p_seeded=p_seeded)
    if after is None:
        return None
    before = after.copy()
    before[:, mover[0], mover[1]], before[:, partner[0], partner[1]] = after[:, partner[0], partner[1]], after[:, mover[0], mover[1]]
    if _runs(before[0]):
        return None
    (r1, c1), (r2, c2) = sorted([mover, partner])
    return before, action_of(R, C, r1, c1, r2 > r1), ucell


def _build_chain(shape, cell, rs):
    R, C, k, sm = shape
    _, T, U, order, pos, bg = cell
    for _ in range(40):
        if pos is not None:
            spots = _pos_cells(shape, pos)
            tcell = spots[int(rs.integers(len(spots)))]
        else:
            tcell = (int(rs.integers(R)), int(rs.integers(C)))
        cands = _chain_candidates(shape, T, tcell)
        if not cands:
            continue
        got = _chain_board(shape, rs, bg, T, tcell, cands[int(rs.integers(len(cands)))], U, order)
        if got is not None:
            board, action, ucell = got
            return board, action, (tcell[0] * C + tcell[1], -1 if ucell is None else ucell[0] * C + ucell[1])
    return None


def counts_at_hit(board, action, tcell):
    """The colour counts activate_special's cookie branch sees (board.py:532-537)
    when the special at tcell, a cell of the line of three that `action`
    completes, is the first special the resolve reaches: the board after the
    swap, less the line's cells in front of tcell (sorted, deleted before it)
    and tcell itself.  Returns (counts of every tile, counts of normal tiles)."""
    _, R, C = board.shape
    b = swapped(board, action)
    line = line_through(b, tcell)
    gone = [p for p in line if p <= tcell]
    for p in gone:
        b[:, p[0], p[1]] = 0
    k = int(board[0].max())
    return (np.bincount(b[0][b[0] != 0].astype(np.int64), minlength=k + 1),
            np.bincount(b[0][(b[0] != 0) & (b[1] == 1)].astype(np.int64), minlength=k + 1))


def swapped(board, action):
    b = np.array(board, np.int8)
    (r1, c1), (r2, c2) = cells_of(b.shape[1], b.shape[2], int(action))
    b[:, r1, c1], b[:, r2, c2] = board[:, r2, c2], board[:, r1, c1]
    return b


def line_through(b, tcell):
    """The sorted cells of the one window of three equal colours of b that holds tcell."""
    ws = [w for w in _runs(b[0]) if tuple(tcell) in w]
    assert len(ws) == 1, ws
    return list(ws[0])


def _first_cookie_chain(shape, rs, bg, special_colour=None):
    """A chain row whose line of three has a coloured cookie as its first cell
    in sorted order where the shape admits it (the top of a vertical line), else
    as its middle cell: the cookie is the first special the resolve reaches."""
    R, C, k, sm = shape
    for _ in range(40):
        tcell = (int(rs.integers(R)), int(rs.integers(C)))
        cands = [x for x in _chain_candidates(shape, KC, tcell) if R < 3 or x[0][0] == tcell]
        if not cands:
            continue
        # a few specials of one colour tip the count; more of them would clear the whole board
        got = _chain_board(shape, rs, bg, KC, tcell, cands[int(rs.integers(len(cands)))], special_colour=special_colour,
                           p_seeded=min(P_SEEDED, 8 / (R * C)))
        if got is not None:
            return got[0], got[1], tcell
    return None


def _build_cookie(shape, cell, rs):
    R, C, k, sm = shape
    tag = cell[1]
    if tag == TIE:
        for _ in range(2000):
            got = _first_cookie_chain(shape, rs, CLEAN)
            if got is None:
                continue
            board, action, tcell = got
            cnt = np.sort(counts_at_hit(board, action, tcell)[0][1:])
            if cnt[-1] == cnt[-2] and (len(cnt) < 3 or cnt[-2] > cnt[-3]):
                return board, action, (tcell[0] * C + tcell[1], -1)
        return None
    if tag == SPECIAL_MAJORITY:
        for _ in range(2000):
            got = _first_cookie_chain(shape, rs, SEEDED, special_colour=int(rs.integers(1, k + 1)))
            if got is None:
                continue
            board, action, tcell = got
            every, normal = counts_at_hit(board, action, tcell)
            e, n = np.sort(every[1:]), np.sort(normal[1:])
            if every[1:].argmax() != normal[1:].argmax() and e[-1] > e[-2] and n[-1] > n[-2]:
                return board, action, (tcell[0] * C + tcell[1], -1)
        return None
    if tag in (MID_CHAIN, MID_CHAIN_REVERSED):
        got = _build_mid_chain(shape, rs)
        if got is None:
            return None
        board, action, tcell, kcell = got
        if tag == MID_CHAIN_REVERSED:
            board, action, tcell, kcell = mirrored(board, action, tcell, kcell)
        return board, action, (tcell[0] * C + tcell[1], kcell[0] * C + kcell[1])
    assert tag == NONE_LEFT
    # every coloured tile sits inside the 5 x 5 of a bomb + bomb, in front of a colourless cookie; all else is cookies
    r, c = (R - 1) // 2, (C - 2) // 2
    typ = np.full((R, C), -1, np.int8)
    col = np.zeros((R, C), np.int8)
    region = [(i, j) for i in range(max(r - 2, 0), min(r + 2, R - 1) + 1)
              for j in range(max(c - 2, 0), min(c + 2, C - 1) + 1)]
    a, b = _two_colours(rs, k)
    typ[r, c], col[r, c], typ[r, c + 1], col[r, c + 1] = 4, a, 4, b
    spots = [p for p in region[:-1] if p not in ((r, c), (r, c + 1))]
    for i in rs.choice(len(spots), size=min(4, len(spots)), replace=False).tolist():
        typ[spots[i]], col[spots[i]] = 1, int(rs.integers(1, k + 1))
    if _runs(col):
        return None
    return np.stack([col, typ]).astype(np.int8), action_of(R, C, r, c, 0), (r * C + c, region[-1][0] * C + region[-1][1])


def _build_mid_chain(shape, rs):
    """A horizontal laser, the first cell of the horizontal line of three a swap
    completes, sweeps its row from column 0 on (board.py:511): tiles of colour A
    in front of a colourless cookie at the row's far end are deleted before the
    cookie is hit and counts.  On the mirrored board the cookie is hit first.
    The two cookies pick different colours."""
    R, C, k, sm = shape
    for _ in range(4000):
        r = int(rs.integers(R))
        c0 = int(rs.integers(0, C - 3))
        tcell, kcell = (r, c0), (r, C - 1)
        line = [(r, c0), (r, c0 + 1), (r, c0 + 2)]
        cands = [x for x in _chain_candidates(shape, H, tcell) if x[0] == line and x[2][0] != r]
        if not cands:
            continue
        L, A = _two_colours(rs, k)
        F = next(x for x in range(1, k + 1) if x not in (L, A))
        extra = {kcell: (-1, 0)}
        for j in range(C - 1):
            if (r, j) not in line:
                extra[(r, j)] = (1, A if (j & 1) == (c0 & 1) else F)
        got = _chain_board(shape, rs, CLEAN, H, tcell, cands[int(rs.integers(len(cands)))], line_colour=L, extra=extra)
        if got is None:
            continue
        board, action, _ = got
        b = swapped(board, action)
        every = np.bincount(b[0][b[0] != 0].astype(np.int64), minlength=k + 1)
        row = np.bincount(b[0, r][b[0, r] != 0].astype(np.int64), minlength=k + 1)
        first = every.copy()
        first[L] -= 3                                    # mirrored: the line, then the cookie at column 0
        last = every - row                               # as built: the whole row in front of the cookie
        if first[1:].argmax() != last[1:].argmax():
            return board, action, tcell, kcell
    return None


def mirrored(board, action, *cells):
    """The board flipped left to right, with the action and cells that go with it."""
    _, R, C = board.shape
    (r1, c1), (r2, c2) = cells_of(R, C, int(action))
    m1, m2 = sorted([(r1, C - 1 - c1), (r2, C - 1 - c2)])
    return (np.ascontiguousarray(board[:, :, ::-1]), action_of(R, C, m1[0], m1[1], m2[0] > m1[0]),
            *[(r, C - 1 - c) for r, c in cells])


def board_of(shape, cell_index, attempt):
    """(board (2, R, C) int8 before the move, action, (t_cell, u_cell)) of a
    cell's attempt-th candidate, or None when that attempt builds nothing.
    t_cell / u_cell: the flat cells of a chain row's specials T and U (-1: none)."""
    cell = matrix_cells(shape)[cell_index]
    rs = np.random.default_rng([*shape, cell_index, attempt])
    if cell[0] == "cookie" and cell[1] == MID_CHAIN_REVERSED:      # the mirror image of the MID_CHAIN row's board
        rs = np.random.default_rng([*shape, matrix_cells(shape).index(("cookie", MID_CHAIN)), attempt])
    build = {"pair": _build_pair, "chain": _build_chain, "cookie": _build_cookie}[cell[0]]
    return build(shape, cell, rs)


def rng_seed_of(shape, cell_index, attempt):
    """The seed of the row's PCG64 stream (np.random.default_rng(seed))."""
    return (sum(x * m for x, m in zip(shape, (1, 100, 10000, 1000000))) * 4096 + cell_index) * 64 + attempt % 64


# ---------------------------------------------------------------- the census: a row's cell, read off its board
def pair_key(shape, board, action):
    """("pair", k1, k2, vertical, same, row class, column class, background) for a
    pair of lasers / bombs, ("pair", k1, k2, vertical, same, place class, background)
    for a cookie pair, read off the row's input board and action; None when the
    action's tiles do not take the combination branch."""
    R, C = shape[:2]
    (r1, c1), (r2, c2) = cells_of(R, C, int(action))
    k1, k2 = kind_at(board, r1, c1), kind_at(board, r2, c2)
    if (k1, k2) not in ordered_pairs(15):
        return None
    both = k1 != K and k2 != K
    same = int(board[0, r1, c1] == board[0, r2, c2]) if both else -1
    others = int((board[1] != 1).sum()) - (k1 != N) - (k2 != N)
    bg = SEEDED if others else CLEAN
    if both and bg == SEEDED and tuple(shape) in THIN_SEEDED:
        same = "any"
    if geometric(k1, k2):
        return ("pair", k1, k2, int(r2 > r1), same, line_class(r1, R), line_class(c1, C), bg)
    return ("pair", k1, k2, int(r2 > r1), same, place_class(r1, c1, R, C), bg)


def required_pair_keys(shape):
    """The pair cells the issue asks for, written from the shape alone."""
    R, C, k, sm = shape
    out = set()
    for (k1, k2) in ordered_pairs(sm):
        both = k1 != K and k2 != K
        for vertical in (0, 1):
            rows = {(r, c) for r in range(R - 1 if vertical else R) for c in range(C if vertical else C - 1)}
            for bg in (CLEAN, SEEDED):
                thin = both and bg == SEEDED and tuple(shape) in THIN_SEEDED
                for same in (("any",) if thin else (1, 0) if both else (-1,)):
                    if geometric(k1, k2):
                        for rc, cc in {(line_class(r, R), line_class(c, C)) for r, c in rows}:
                            out.add(("pair", k1, k2, vertical, same, rc, cc, bg))
                    else:
                        for pc in {place_class(r, c, R, C) for r, c in rows}:
                            out.add(("pair", k1, k2, vertical, same, pc, bg))
    return out


def chain_key(shape, board, action, t_cell, u_cell):
    """("chain", T, U or None, order, pos or None, background) of a chain row,
    read off its input board, action and the two recorded cells; asserts what
    makes it one: two normal tiles swap, T sits in the line of three the swap
    completes, U sits where T's blast reaches it."""
    R, C = shape[:2]
    (r1, c1), (r2, c2) = cells_of(R, C, int(action))
    assert kind_at(board, r1, c1) == N and kind_at(board, r2, c2) == N
    assert not _runs(np.asarray(board[0])), "the board holds a line before the move"
    after = swapped(board, action)
    tcell = divmod(int(t_cell), C)
    T = kind_at(after, *tcell)
    assert T != N and tcell in line_through(after, tcell)
    others = int((np.asarray(board[1]) != 1).sum()) - 1
    if u_cell < 0:
        return ("chain", T, None, 0, edge_class(*tcell, R, C), SEEDED if others else CLEAN)
    ucell = divmod(int(u_cell), C)
    U = kind_at(after, *ucell)
    assert U != N and ucell not in line_through(after, tcell)
    order = 0
    if T == V:
        assert ucell[1] == tcell[1]
        order = 1 if ucell[0] < tcell[0] else 2
    elif T == H:
        assert ucell[0] == tcell[0]
        order = 1 if ucell[1] < tcell[1] else 2
    elif T == B:
        assert abs(ucell[0] - tcell[0]) <= 1 and abs(ucell[1] - tcell[1]) <= 1
    return ("chain", T, U, order, None, SEEDED if others - 1 else CLEAN)


def cell_key(shape, cell):
    """The census key a row built for `cell` must show."""
    R, C = shape[:2]
    if cell[0] == "pair":
        _, k1, k2, vertical, same, (r, c), bg = cell
        if same >= 0 and bg == SEEDED and tuple(shape) in THIN_SEEDED:
            same = "any"
        if geometric(k1, k2):
            return ("pair", k1, k2, vertical, same, line_class(r, R), line_class(c, C), bg)
        return ("pair", k1, k2, vertical, same, place_class(r, c, R, C), bg)
    return cell


def shows_feature(shape, cell, r, rows=()):
    """Whether record r (board, action, t_cell, u_cell, mid, mid_n_act: the
    reference's board and activation count right after the first stage) is a
    row of `cell`: what the cell is about did happen.  rows: the records so
    far (the mirrored mid-chain row is judged against its partner)."""
    R, C = shape[:2]
    board, mid = np.asarray(r["board"]).reshape(2, R, C), np.asarray(r["mid"]).reshape(2, R, C)
    if cell[0] == "pair":
        return True
    if cell[0] == "chain":
        t, u = divmod(int(r["t_cell"]), C), divmod(int(r["u_cell"]), C)
        if mid[1][t] != 0 or int(r["mid_n_act"]) < 1 + (cell[2] is not None):
            return False
        return cell[2] is None or mid[1][u] == 0
    tag = cell[1]
    if tag == NONE_LEFT:
        u = divmod(int(r["u_cell"]), C)
        return not mid[0].any() and mid[1][u] == -1 and int(r["mid_n_act"]) == 2
    tcell = divmod(int(r["t_cell"]), C)
    normal_left = lambda x: bool(((mid[0] == x) & (mid[1] == 1)).any())       # noqa: E731
    if tag in (TIE, SPECIAL_MAJORITY):
        every, normal = counts_at_hit(board, r["action"], tcell)
        top = np.nonzero(every[1:] == every[1:].max())[0] + 1
        if tag == TIE:
            return len(top) == 2 and not normal_left(top[0]) and normal_left(top[1])
        return (len(top) == 1 and normal[1:].argmax() + 1 != top[0] and not normal_left(top[0])
                and normal_left(normal[1:].argmax() + 1))
    if tag == MID_CHAIN:
        return True                                       # judged with its mirror image
    mates = [x for x in rows if matrix_cells(shape)[int(x["cell"])] == ("cookie", MID_CHAIN) and not x["err"]
             and int(x["attempt"]) == int(r["attempt"])]
    if len(mates) != 1:
        return False
    m = mates[0]
    mboard, mmid = np.asarray(m["board"]).reshape(2, R, C), np.asarray(m["mid"]).reshape(2, R, C)
    return np.array_equal(mboard[:, :, ::-1], board) and not np.array_equal(mmid[:, :, ::-1], mid)


# ---------------------------------------------------------------- the recorded rows and the checks every player runs
@functools.lru_cache(maxsize=None)
def load_matrix(shape):
    """The rows of tests/golden/matrix_<shape>.npz, read-only arrays stacked over
    the rows: board / mid / out (n, 2, R, C) int8, rng_in / rng_out (n, 5)
    uint64, res (n, 5) int32 (num_eliminations, is_combination_match,
    num_new_specials, num_specials_activated, shuffled), and the per-row
    scalars action, cell, attempt, kind, t_cell, u_cell, mid_n_act, mid_n_new, err."""
    from golden_io import GOLDEN
    R, C = shape[:2]
    with np.load(os.path.join(GOLDEN, f"matrix_{shape_id(shape)}.npz"), allow_pickle=False) as z:
        z = {f: z[f] for f in z.files}                   # the layout of make_goldens.pack_records; every row the same size
    n = int(z["n"])
    assert (z["shape"] == np.array(shape)).all() and len(z["shape"]) == n
    d = {f: z[f].reshape(n, 2, R, C).astype(np.int8) for f in ("board", "mid", "out")}
    d.update({f: z[f].reshape(n, 5).astype(np.uint64) for f in ("rng_in", "rng_out")})
    d["res"] = z["res"].reshape(n, 5).astype(np.int32)
    for f in ("action", "cell", "attempt", "kind", "t_cell", "u_cell", "mid_n_act", "mid_n_new", "err"):
        d[f] = z[f].reshape(n).astype(np.int32)
    d["swapped"] = np.stack([swapped(b, a) for b, a in zip(d["board"], d["action"])])
    for a in d.values():
        a.setflags(write=False)
    return d


def played_rows(d):
    """The rows a kernel plays: those the reference finished (test_oracle_golden.py skips the others the same way)."""
    return np.nonzero(d["err"] == 0)[0]


def seeded_rows(shape, d):
    """The played pair and chain rows on a seeded background."""
    cells = matrix_cells(shape)
    return np.array([i for i in played_rows(d) if cells[d["cell"][i]][0] != "cookie" and cells[d["cell"][i]][-1] == SEEDED])


FLAG_COMBO, FLAG_SHUFFLED, FLAG_ERROR = 2, 4, 0x80


def want_flags(res):
    return ((res[:, 1] != 0) * FLAG_COMBO + (res[:, 4] != 0) * FLAG_SHUFFLED).astype(np.uint8)


def _first_bad(got, want):
    bad = np.nonzero((np.asarray(got).reshape(len(want), -1) != np.asarray(want).reshape(len(want), -1)).any(axis=1))[0]
    return bad


def assert_rows_equal(shape, d, rows, got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.int64 and want.dtype == np.uint64:
        got = got.view(np.uint64)
    bad = _first_bad(got, want)
    if bad.size:
        i = int(rows[bad[0]])
        cell = matrix_cells(shape)[int(d["cell"][i])]
        raise AssertionError(f"{shape_id(shape)} {what}: {bad.size} rows differ, first row {i} (cell {cell}, attempt "
                             f"{int(d['attempt'][i])}, action {int(d['action'][i])})\ninput\n{d['board'][i]}\n"
                             f"got\n{got[bad[0]]}\nwant\n{want[bad[0]]}")


def check_trace(dev, shape):
    """tmg_trace with the swap, combo and clear stages, stopped after the second
    frame: the swapped board, then the reference's own board right after
    combination_match (a chain row: after the first resolve) and its
    activation count (a chain row: and its new specials) — no oracle in between."""
    import trace_cases as tc
    d = load_matrix(shape)
    rows = played_rows(d)
    mask = (1 << tc.SWAP) | (1 << tc.COMBO) | (1 << tc.CLEAR)
    dev.status_clear(shape)
    got = tc.trace(dev, shape, d["board"][rows], d["rng_in"][rows], None, 0, d["action"][rows][None, :], mask, 2, stop=1)
    combo = d["res"][rows, 1] != 0                      # is_combination_match: the first stage was combination_match
    assert_rows_equal(shape, d, rows, got["n_frames"][0], np.full(len(rows), 2), "trace n_frames")
    assert_rows_equal(shape, d, rows, got["kind"][0], np.stack([np.full(len(rows), tc.SWAP), np.where(combo, tc.COMBO, tc.CLEAR)], 1),
                      "trace frame kinds")
    assert_rows_equal(shape, d, rows, got["frames"][0, :, 0], d["swapped"][rows], "trace swap frame")
    assert_rows_equal(shape, d, rows, got["frames"][0, :, 1], d["mid"][rows], "trace combo / first clear frame vs the reference")
    assert_rows_equal(shape, d, rows, got["n_act"][0], d["mid_n_act"][rows], "trace n_act after the first stage")
    assert_rows_equal(shape, d, rows, got["n_new"][0], d["mid_n_new"][rows], "trace n_new after the first stage")
    assert_rows_equal(shape, d, rows, got["frame_elim"][0, :, 1], (d["mid"][rows][:, 1] == 0).sum(axis=(1, 2)), "trace frame_elim")
    assert_rows_equal(shape, d, rows, got["flags"][0] & (FLAG_COMBO | FLAG_ERROR), combo * FLAG_COMBO, "trace flags")
    assert (got["flags"][0] & tc.FLAG_STOPPED).all()
    assert dev.status_clear(shape) == 0


def check_step(dev, shape):
    """An untrusted tmg_step (the boards are hand-built) from the recorded RNG
    words: board, RNG words, reward, n_new, n_act and flags equal the
    reference's recorded Board.move."""
    d = load_matrix(shape)
    rows = played_rows(d)
    dev.status_clear(shape)
    board, rng, reward, n_new, n_act, flags = dev.step(shape, d["board"][rows], d["rng_in"][rows], d["action"][rows])
    assert_rows_equal(shape, d, rows, board, d["out"][rows], "step board")
    assert_rows_equal(shape, d, rows, rng, d["rng_out"][rows], "step rng words")
    res = d["res"][rows]
    assert_rows_equal(shape, d, rows, reward, res[:, 0], "step reward")
    assert_rows_equal(shape, d, rows, n_new, res[:, 2], "step n_new")
    assert_rows_equal(shape, d, rows, n_act, res[:, 3], "step n_act")
    assert_rows_equal(shape, d, rows, np.asarray(flags) & (FLAG_COMBO | FLAG_SHUFFLED | FLAG_ERROR), want_flags(res), "step flags")
    assert dev.status_clear(shape) == 0
