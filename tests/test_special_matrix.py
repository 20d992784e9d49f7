"""The special-tile matrix (tests/special_matrix_cases.py) without a GPU: the
census of the fixtures recorded from the reference (tests/golden/matrix_*.npz,
tests/golden/make_special_matrix.py), the CPU oracle on every row, and the host
wave emulator on every row.  Everything is compared as integers and bytes;
nothing here has a tolerance.

The census is computed from the fixtures: each row's cell is read off its
recorded input board and action, and the cells that must be there are written
from the shape alone (special_matrix_cases.required_pair_keys and
required_chain_keys below), not from the generator's list."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import special_matrix_cases as sm
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")
SHAPES = sm.SHAPES


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    L = emu.load()
    L.emu_status_clear()
    return emu, L


# ---------------------------------------------------------------- the shapes reach the kernels they are named for
def _fix(R, C, k, smask):
    return R << 24 | C << 16 | k << 8 | smask


# <MAXN, GEN, NB, CODD, FIX> of an untrusted step, written out by hand from csrc/tmg_dispatch.h
STEP_OF = {
    (10, 10, 4, 14): (128, 1, 2, 0, _fix(10, 10, 4, 14)),     # kFixC3
    (20, 20, 6, 15): (512, 1, 0, 0, _fix(20, 20, 6, 15)),     # kFixC5
    (6, 6, 4, 15): (128, 1, 2, 0, 0),                         # bitboard, even C
    (5, 5, 3, 15): (128, 1, 2, 1, 0),                         # bitboard, odd C
    (7, 9, 10, 15): (128, 1, 4, 1, 0),                        # four colour planes
    (2, 64, 4, 15): (128, 1, 0, 0, 0),                        # no bitboard
    (3, 43, 5, 15): (512, 1, 0, 0, 0),                        # the generic 512-cell kernel
}


def test_shapes_reach_every_general_family(emu_lib):
    emu, L = emu_lib
    assert list(STEP_OF) == SHAPES
    for shape, want in STEP_OF.items():
        st, _ = emu.route(L, *shape, trust_eff=0, mode=0)
        assert tuple(st[f] for f in ("MAXN", "GEN", "NB", "CODD", "FIX")) == want, shape
        assert (st["lean"], st["lane"], st["spill"]) == (0, 0, 1), shape
        pk = emu.peek_route(L, *shape, trust_eff=0)
        assert (pk["MAXN"], pk["GEN"], pk["NB"], pk["CODD"]) == want[:4], shape
    assert len({w[:4] + (w[4] != 0,) for w in STEP_OF.values()}) == len(SHAPES), "two shapes reach the same kernel"


# ---------------------------------------------------------------- census
POSITIONS = ("corner", "top", "bottom", "left", "right", "interior")
# where a special cannot sit inside a line of three that a swap completes: a board of two rows has no vertical line,
# so nothing of its side columns but the corners, and no interior; its coloured cookie is found only in the middle of
# a horizontal line (special_matrix_cases.chain_pos_admitted), never in a corner
NO_CHAIN_POS = {(2, 64, 4, 15): {(T, p) for T in (sm.V, sm.H, sm.B, sm.KC) for p in ("left", "right", "interior")}
                | {(sm.KC, "corner")}}


def required_chain_keys(shape):
    """The chain cells the issue asks for, from the shape alone: every enabled T
    at corner / each edge / interior, every ordered (T, U) with U inside T's
    blast, for a laser both before and after T in its sweep; both backgrounds.
    A colourless cookie is in no colour line, and a cookie activates no cookie
    (board.py:547), so those cells do not exist."""
    en = sm.enabled_kinds(shape[3])
    out = set()
    for T in en:
        if T == sm.K:
            continue
        for bg in (sm.CLEAN, sm.SEEDED):
            out |= {("chain", T, None, 0, p, bg) for p in POSITIONS if (T, p) not in NO_CHAIN_POS.get(shape, ())}
            for U in en:
                if T == sm.KC and U in (sm.K, sm.KC):
                    continue
                out |= {("chain", T, U, order, None, bg) for order in ((1, 2) if T in (sm.V, sm.H) else (0,))}
    return out


def required_keys(shape):
    out = sm.required_pair_keys(shape) | required_chain_keys(shape)
    if shape[3] & 1:
        out |= {("cookie", tag) for tag in sm.COOKIE_TAGS}
    return out


def row_key(shape, d, i):
    """Row i's cell, read off what the fixture holds for it."""
    kind = int(d["kind"][i])
    if kind == sm.ROW_PAIR:
        return sm.pair_key(shape, d["board"][i], d["action"][i])
    if kind == sm.ROW_CHAIN:
        return sm.chain_key(shape, d["board"][i], d["action"][i], d["t_cell"][i], d["u_cell"][i])
    return sm.matrix_cells(shape)[int(d["cell"][i])]


def _record(d, i):
    return {f: d[f][i] for f in ("board", "action", "t_cell", "u_cell", "mid", "mid_n_act", "cell", "attempt", "err")}


def census(shape, d, keep=None):
    """{cell: number of rows that cover it}: rows the reference finished
    (err = 0) that show the cell's feature.  keep: the row indices counted."""
    rows = range(len(d["err"])) if keep is None else keep
    recs = [_record(d, i) for i in rows]
    cover = collections.Counter()
    for r, i in zip(recs, rows):
        if r["err"]:
            continue
        key = row_key(shape, d, i)
        cell = key if key[0] != "pair" else None
        ok = key[0] == "pair" or sm.shows_feature(shape, cell, r, recs)
        if key == ("cookie", sm.MID_CHAIN):                # counts with its mirror image only
            ok = any(sm.shows_feature(shape, ("cookie", sm.MID_CHAIN_REVERSED), x, recs) for x in recs
                     if not x["err"] and x["attempt"] == r["attempt"]
                     and sm.matrix_cells(shape)[int(x["cell"])] == ("cookie", sm.MID_CHAIN_REVERSED))
        if ok:
            cover[key] += 1
    return cover


@pytest.fixture(scope="module")
def covers():
    return {shape: census(shape, sm.load_matrix(shape)) for shape in SHAPES}


@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_census_every_cell_is_covered(covers, shape):
    missing = required_keys(shape) - set(covers[shape])
    assert not missing, f"{len(missing)} cells without a finished row, e.g. {sorted(missing, key=str)[:5]}"
    extra = set(covers[shape]) - required_keys(shape)
    assert not extra, f"rows of cells the matrix does not name: {sorted(extra, key=str)[:5]}"


def test_census_cell_counts():
    """The counts DESIGN.md states, per shape: required cells."""
    assert [len(required_keys(s)) for s in SHAPES] == [1506, 1483, 1897, 1897, 1897, 783, 1249]
    assert len(sm.ordered_pairs(15)) == 29 and len(sm.ordered_pairs(14)) == 9


@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_census_rows_are_the_generators(shape):
    """Every row is board_of(shape, cell, attempt), under the key of its cell."""
    d = sm.load_matrix(shape)
    cells = sm.matrix_cells(shape)
    for i in range(len(d["err"])):
        board, action, (t, u) = sm.board_of(shape, int(d["cell"][i]), int(d["attempt"][i]))
        assert np.array_equal(board, d["board"][i]) and (action, t, u) == (d["action"][i], d["t_cell"][i], d["u_cell"][i]), i
        assert row_key(shape, d, i) == sm.cell_key(shape, cells[int(d["cell"][i])]), i
        assert int(d["kind"][i]) == {"pair": sm.ROW_PAIR, "chain": sm.ROW_CHAIN, "cookie": sm.ROW_COOKIE}[cells[d["cell"][i]][0]]


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] & 1], ids=sm.shape_id)
def test_census_cookie_rows_show_their_feature(shape):
    """Read off the recorded boards alone: the tie is a tie and the lower colour
    went; the majority exists only with the specials' colours counted; the
    mirrored mid-chain boards are mirror images and their results differ; the
    last special of the bomb + bomb survives on a board without a colour."""
    d = sm.load_matrix(shape)
    R, C, k, _ = shape
    cells = sm.matrix_cells(shape)
    row = {cells[int(d["cell"][i])][1]: i for i in range(len(d["err"])) if d["kind"][i] == sm.ROW_COOKIE and not d["err"][i]}
    assert set(row) == set(sm.COOKIE_TAGS)

    def normals(i, x):
        return int(((d["mid"][i][0] == x) & (d["mid"][i][1] == 1)).sum())

    i = row[sm.TIE]
    every, _ = sm.counts_at_hit(d["board"][i], d["action"][i], divmod(int(d["t_cell"][i]), C))
    lo, hi = np.nonzero(every[1:] == every[1:].max())[0] + 1
    assert lo < hi and normals(i, lo) == 0 and normals(i, hi) > 0
    i = row[sm.SPECIAL_MAJORITY]
    every, normal = sm.counts_at_hit(d["board"][i], d["action"][i], divmod(int(d["t_cell"][i]), C))
    a, b = int(normal[1:].argmax()) + 1, int(every[1:].argmax()) + 1
    assert a != b and (every[1:] == every[b]).sum() == 1 and normals(i, b) == 0 and normals(i, a) > 0
    i, j = row[sm.MID_CHAIN], row[sm.MID_CHAIN_REVERSED]
    assert np.array_equal(d["board"][i][:, :, ::-1], d["board"][j])
    assert not np.array_equal(d["mid"][i][:, :, ::-1], d["mid"][j]) and not np.array_equal(d["out"][i][:, :, ::-1], d["out"][j])
    gone = lambda r: {x for x in range(1, k + 1) if ((d["swapped"][r][0] == x) & (d["swapped"][r][1] == 1)).any()  # noqa: E731
                      and normals(r, x) == 0}
    assert gone(i) != gone(j), "both cookies picked the same colour"
    i = row[sm.NONE_LEFT]
    assert not d["mid"][i][0].any() and d["mid"][i][1].reshape(-1)[d["u_cell"][i]] == -1 and d["mid_n_act"][i] == 2


@pytest.mark.parametrize("shape", [(5, 5, 3, 15), (10, 10, 4, 14)], ids=sm.shape_id)
def test_census_fails_when_a_cells_only_row_is_deleted(covers, shape):
    """Every cell is covered by exactly one finished row here, so deleting any
    row must leave its cell uncovered: one pair row at a border, one chain row,
    and (where there are cookies) the mirrored mid-chain row, whose deletion
    also takes the cover of its partner."""
    d = sm.load_matrix(shape)
    n = len(d["err"])
    assert set(covers[shape].values()) == {1}
    picks = [0, int(np.nonzero(d["kind"] == sm.ROW_CHAIN)[0][3])]
    if shape[3] & 1:
        picks.append(int(np.nonzero(d["kind"] == sm.ROW_COOKIE)[0][3]))
    for i in picks:
        left = census(shape, d, keep=[j for j in range(n) if j != i])
        missing = required_keys(shape) - set(left)
        assert row_key(shape, d, i) in missing, i
        assert len(missing) == (2 if d["kind"][i] == sm.ROW_COOKIE else 1)


# ---------------------------------------------------------------- oracle
@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_oracle_equals_the_reference(shape):
    """orc.combination / orc.detect_resolve on the swapped board against the
    reference's recorded board right after that stage, and orc.move against its
    recorded Board.move, on every row the reference finished."""
    d = sm.load_matrix(shape)
    _, _, k, smask = shape
    rows = sm.played_rows(d)
    assert len(rows) >= len(required_keys(shape))
    for i in rows:
        what = f"row {i} cell {sm.matrix_cells(shape)[int(d['cell'][i])]}"
        if d["res"][i, 1]:                               # is_combination_match: the first stage was combination_match
            mid, na, err = orc.combination(d["swapped"][i], d["action"][i], k, smask)
            nn = 0
        else:
            mid, na, nn, err = orc.detect_resolve(d["swapped"][i], k, smask)
        assert err == 0, what
        assert np.array_equal(mid, d["mid"][i]), f"{what}\ninput\n{d['board'][i]}\ngot\n{mid}\nwant\n{d['mid'][i]}"
        assert (na, nn) == (d["mid_n_act"][i], d["mid_n_new"][i]), what
        out, rng, res, err = orc.move(d["board"][i], d["rng_in"][i], d["action"][i], k, smask)
        assert err == 0, what
        assert np.array_equal(out, d["out"][i]), what
        assert np.array_equal(rng, d["rng_out"][i]), what
        assert np.array_equal(res, d["res"][i]), what


# ---------------------------------------------------------------- host wave emulator
@pytest.fixture(scope="module")
def dev(emu_lib):
    from test_trace_emulated import EmuDev
    return EmuDev(*emu_lib)


@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_emulated_trace_equals_the_reference(dev, shape):
    sm.check_trace(dev, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_emulated_step_equals_the_reference(dev, shape):
    sm.check_step(dev, shape)


def test_emulated_seeded_20x20_rows_spill(dev):
    """Some seeded 20x20 rows outgrow the LDS lists and are re-run by the spill
    pass (test_emulated_step_equals_the_reference compares them all the same):
    the prediction tests/test_gpu_special_matrix.py holds the device's count to."""
    shape = (20, 20, 6, 15)
    d = sm.load_matrix(shape)
    rows = sm.seeded_rows(shape, d)
    s0 = dev.spills(shape)
    board = dev.step(shape, d["board"][rows], d["rng_in"][rows], d["action"][rows])[0]
    assert np.array_equal(board, d["out"][rows])
    assert dev.spills(shape) - s0 > 0
    dev.status_clear(shape)


# ---------------------------------------------------------------- the lean step's type check (tests/lean_type_cases.py)
import lean_type_cases as lt    # noqa: E402


def _emu_lean_step(emu, L):
    def step(shape, board, rng, timer, eff, actions, fused):
        R, C, k, smask = shape
        e = emu.EmuBatch(L, R, C, k, smask, lt.MOVES, rng)
        e.board[:], e.timer[:], e.eff[:] = board, timer, eff
        e.trust = True
        term = np.full((len(actions), 4), 0x55, np.uint8)
        L.emu_status_clear()
        e.step(actions, autoreset=False, outputs={"terminated": term} if fused else None)
        return dict(board=e.board, rng=e.rng, timer=e.timer, reward=e.reward, n_new=e.n_new, n_act=e.n_act, flags=e.flags,
                    status=L.emu_status_clear(), terminated=term)
    return step


@pytest.mark.parametrize("name", list(lt.CASES))
def test_emulated_lean_step_checks_the_type_plane(emu_lib, name):
    emu, L = emu_lib
    shape, fused, inst, plain = lt.CASES[name]
    st, _ = emu.route(L, *shape, trust_eff=1, mode=0, n=lt.N_ENVS, have_lane=True, fused=("terminated",) if fused else ())
    assert tuple(st[f] for f in ("MAXN", "GEN", "NB", "CODD", "FIX")) == inst and (st["lean"], st["lane"], st["plain"]) == (1, 0, plain)
    lt.check(_emu_lean_step(emu, L), name)
