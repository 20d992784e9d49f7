"""Shared by tests/test_lean_levers_emulated.py and tests/test_gpu_lean_levers.py:
cases for the lean step's three-row gravity shift (rp_move, TMG_RP_VSHIFT) and
its two-plane effective-mask scan (rp_scan, TMG_RP_SCAN2).

A gravity case is a line-free board, a move and the env's stream, written down
as data; the feature it is there for is a predicate over the oracle's own
trace of that move (rowplane_cases.trace_move: per cascade iteration the lines
get_colour_lines returns), which the tests assert before they compare
anything.  Expected results are always the oracle's."""
import numpy as np

from rowplane_cases import _bg, haction

# rollouts: the row-plane shapes (rowplane_cases.SHAPES) and, for the scan,
# k = 2 and 8 (with 4: the new path, one plane fewer than the colour value
# needs), k = 3 and 5 (the old one), C = 3 (R = 16 keeps it a row-plane shape)
# beside C = 28, R = 3.  Two colours on a small board only: a line-free 10x10 board of two colours is
# never drawn.
GRAVITY_SHAPES = [(4, 4, 3), (5, 6, 7), (10, 10, 4), (10, 10, 5), (16, 8, 4), (3, 28, 6)]
SCAN_SHAPES = [(4, 4, 2), (10, 10, 4), (6, 6, 8), (6, 6, 3), (10, 10, 5), (16, 3, 4), (3, 28, 8), (3, 28, 6)]
SCAN_NEW_PATH = {2, 4, 8}                 # colour counts whose value needs a plane more than colour - 1
MOVES = 10
STEPS = 30
FIELDS = ("board", "rng", "timer", "eff", "reward", "n_new", "n_act", "flags")


def _vertical(ln):
    return len(ln) >= 3 and len({c for _, c in ln}) == 1


def _horizontal(ln):
    return len(ln) >= 3 and len({r for r, _ in ln}) == 1


def _parts(lines):
    """(cleared cells, bottom row rs, vertical lines: all end in row rs, horizontal lines)."""
    cleared = {tuple(cell) for ln in lines for cell in ln}
    rs = max(r for r, _ in cleared)
    vs = [sorted(tuple(x) for x in ln) for ln in lines if _vertical(ln)]
    hs = [sorted(tuple(x) for x in ln) for ln in lines if _horizontal(ln)]
    vs = [v for v in vs if v[-1][0] == rs]
    return cleared, rs, vs, hs


def _any_iteration(fn):
    def pred(its, R):
        return any(fn(*_parts(lines), R) for lines in its)
    return pred


def _vlen(n, where=None, exact=True):
    def fn(cleared, rs, vs, hs, R):
        ok = any((len(v) == n if exact else len(v) >= n) for v in vs)
        return ok and (where is None or rs == (2 if where == "top" else R - 1))
    return _any_iteration(fn)


def _whole_column(cleared, rs, vs, hs, R):
    return any(len(v) == R for v in vs)


def _v3_and_v5(cleared, rs, vs, hs, R):
    return any(len(v) == 3 for v in vs) and any(len(v) == 5 for v in vs)


def _cross_at_rs(where):
    def fn(cleared, rs, vs, hs, R):
        for v in vs:
            for h in hs:
                if h[0][0] == rs and v[-1] in h:
                    at = h.index(v[-1])
                    if (where == "end") == (at in (0, len(h) - 1)):
                        return True
        return False
    return _any_iteration(fn)


def _perp_mid(cleared, rs, vs, hs, R):
    """a perpendicular run through the middle of a vertical run: single holes in the neighbour columns"""
    for v in vs:
        for h in hs:
            for cell in v[1:-1]:
                if cell in h and h[0][0] < rs:
                    return True
    return False


def _two_holes_beside(cleared, rs, vs, hs, R):
    """two perpendicular runs at different rows meet one column outside the
    vertical runs: two separate holes there, beside a three-row shift"""
    vcols = {v[0][1] for v in vs}
    if not vcols:
        return False
    for c in {c for _, c in cleared} - vcols:
        rows = sorted(r for r, cc in cleared if cc == c)
        if any(b - a > 1 for a, b in zip(rows, rows[1:])):
            return True
    return False


def _perp_into_run_column(cleared, rs, vs, hs, R):
    """a perpendicular run's cell lies in the column of another vertical run, above that run"""
    for v in vs:
        c, top = v[0][1], v[0][0]
        if any(cc == c and r < top for r, cc in cleared):
            return True
    return False


# A vertical and a horizontal line of row rs can share a cell as an L (the end of the horizontal
# line) or a T (its middle); a plus cannot occur there, since a vertical line of the first pass ends in
# row rs.  A crossing above rs is a perpendicular run: "perp_through_middle".
PREDICATES = {
    "v3_reaches_row0": _vlen(3, "top"),
    "v3_last_row": _vlen(3, "bottom"),
    "v4": _vlen(4),
    "v5_or_more": _vlen(5, exact=False),
    "whole_column": _any_iteration(_whole_column),
    "v3_and_v5_same_row": _any_iteration(_v3_and_v5),
    "L_at_rs": _cross_at_rs("end"),
    "T_at_rs": _cross_at_rs("mid"),
    "perp_through_middle": _any_iteration(_perp_mid),
    "two_holes_beside_shift": _any_iteration(_two_holes_beside),
    "perp_into_run_column": _any_iteration(_perp_into_run_column),
}
# cover site a case must count beside rp_vshift (None: rp_vshift alone)
SITES = {
    "v3_reaches_row0": None, "v3_last_row": None, "v4": "rp_vmore", "v5_or_more": "rp_vmore", "whole_column": None,
    "v3_and_v5_same_row": "rp_vmore", "L_at_rs": None, "T_at_rs": None, "perp_through_middle": None,
    "two_holes_beside_shift": "rp_vmore", "perp_into_run_column": "rp_vmore",
}


def _v3_v5_board():
    """One horizontal swap, (5,4)-(5,5), completes a run of 3 in column 4 (rows
    5..7) and a run of 5 in column 5 (rows 3..7): both end in row 7."""
    b = _bg()
    b[5, 4], b[5, 5] = 1, 2
    b[[6, 7], 4] = 2
    b[[3, 4, 6, 7], 5] = 1
    return " ".join("".join(str(int(x)) for x in row) for row in b)


# name -> (predicate or predicates, (R, C, k), board rows, action, the stream's five state words or a seed).  All but
# the first were taken from oracle rollouts with their streams (the feature often shows in a later
# iteration of the move's cascade, where the refill decides it).
CASES = {
    "v3_and_v5_same_row": ("v3_and_v5_same_row", (10, 10, 4), _v3_v5_board(), haction(5, 4), 21),
    "v3_reaches_row0": ("v3_reaches_row0", (10, 10, 4),
        "2322314234 3133424422 4433211243 3124324141 3232233413 2434332424 1421241212 1341313424 2114322113 3413234343",
        91, (0xc69f310e77628721, 0x37f1beaed4b70e0a, 0x6e0197a4645cae1b, 0x9bde71a450c6b76e, 0x495f8b74)),
    "v3_last_row_and_v4": (("v3_last_row", "v4"), (10, 10, 4),        # one move, both features
        "2432213414 4341121422 2314323211 4123113123 1312241314 1212113313 3421123124 1212434243 4434423124 2414132234",
        61, (0x3b417c7801950e73, 0x18a4b2ad58eea72c, 0xaeb4a2f6917f7d9d, 0xaac109b5ec6fb840, 0x7c8f973b)),
    "v5_or_more": ("v5_or_more", (10, 10, 4),
        "3211223221 2421413113 2434211414 4221221442 4231314142 2442242334 4413231143 4313442121 1241221243 1432243132",
        77, (0xa37cad4ad0ac53cf, 0xbf80f89bc9c7d1a3, 0x50c57f88f8c53157, 0x6cfd0dead58ad41, 0xaba232d7)),
    "L_at_rs": ("L_at_rs", (10, 10, 4),
        "3232443241 1234434213 2144313421 2441242213 1324224243 4231132311 1122433114 2132321144 1343244223 4232323311",
        142, (0xa91ceaa3508938e6, 0x8e27bd4bbae59e35, 0xbc97c3eff8825fd1, 0x56b4e186a48263ce, 0x1d4d94da)),
    "T_at_rs": ("T_at_rs", (10, 10, 4),
        "2143144141 1413214221 1321143242 4243241313 4132322312 3112411234 1221331241 4343442442 1214331133 2313211342",
        73, (0xfe4855c9b5c28803, 0x891a2d49769d862a, 0x48b1a089c5ff5da7, 0x34d67f7ea293a9c9, 0x30d7c38a)),
    "perp_through_middle": ("perp_through_middle", (10, 10, 4),
        "4412432121 2332344212 3133221344 2142343431 4332131231 4224224314 3341441142 3124224112 4411434324 1122122114",
        14, (0xcb5baaf9b5dc7623, 0x5ed57d3973724c12, 0x588deb91591ff853, 0x42aa62a5db364d16, 0x5c74632b)),
    "two_holes_beside_shift": ("two_holes_beside_shift", (10, 10, 4),
        "4121243231 2141242232 3224413143 2314134221 4433244231 1214121434 3212214423 3344323141 2311413324 1132314433",
        10, (0x9be390776046889e, 0x58b812f9823aa05, 0x970e8b6c7cfbb61f, 0x7d47e1545d1ae6f6, 0x1cf3408ac)),
    "perp_into_run_column": ("perp_into_run_column", (10, 10, 4),
        "2423143211 3313232334 1241332233 4243411311 3432432244 3224234334 4113341441 2342334234 4411441241 2231413323",
        138, (0xe08efec96939684d, 0x529f99cc893ea463, 0x2209ab144eaa1f03, 0x6efb5c18a317e2b5, 0x17cc2eb21)),
    "whole_column_3x28": ("whole_column", (3, 28, 6),
        "6213522646255446536164613526 4242562151525161122532411553 6361236645466566115221141246",
        70, (0x13ae1083d17b5323, 0x9ce1377a1ff9de6e, 0x976d2c9a5532e9c5, 0xcde76ed9be9e2b9d, 0xf39d051a)),
    "whole_column_4x4": ("whole_column", (4, 4, 3), "1321 1133 2321 3223",
        5, (0x36882a80487d809c, 0xbc7eb0e00c29413a, 0xaeb4a2f6917f7d9d, 0xaac109b5ec6fb840, 0x34c088a9)),
}
CASE_SHAPES = sorted({c[1] for c in CASES.values()})


def case_predicates(name):
    """The names (PREDICATES, SITES) of the features a case is there for."""
    pred = CASES[name][0]
    return (pred,) if isinstance(pred, str) else tuple(pred)


def case_arrays(name):
    """(predicate name, shape, board (2, R, C) int8 with types 1, action, stream words (5,) uint64)."""
    from rowplane_cases import stream_words
    pred, shape, rows, action, seed = CASES[name]
    col = np.array([[int(x) for x in row] for row in rows.split()], np.int8)
    assert col.shape == shape[:2], name
    return pred, shape, np.stack([col, np.ones_like(col)]).astype(np.int8), int(action), stream_words(seed)
