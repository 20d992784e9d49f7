#!/usr/bin/env python3
"""Recorder of the special-tile matrix (tests/special_matrix_cases.py).  Like
make_goldens.py it runs only where the reference package is present, imports it
behind the same stubs, and writes data only: tests/golden/matrix_<shape>.npz.

Per row, from the reference: the input board, the action and the input RNG
words; the board right after combination_match (board.py:600-719) — for a chain
row the board after the first detect_colour_matches + resolve_colour_matches
(board.py:133-147, :397-427) with num_specials_activated / num_new_specials;
and the whole Board.move (board.py:330-395): output board, output RNG words
and the five results.

Every cell of the matrix gets one row the reference finished without raising
and that shows what the cell is about (a chain row's T and U were activated, a
tie is a tie, ...).  Attempts 0, 1, 2, ... of a cell are tried in order until
one does; a row where the reference raised is kept with err = 1.  A cell no
attempt satisfies ends the run with an error.  The output is a function of this
tree alone: a second run writes the same bytes.

Usage:  python tests/golden/make_special_matrix.py [RxCkKsM ...]
"""
from __future__ import annotations

import io
import os
import signal
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import make_goldens as mg                    # noqa: E402
import special_matrix_cases as sm            # noqa: E402

MAX_ATTEMPTS = 400
ALARM = 20


def takes_combination(board, c1, c2):
    t1, t2 = int(board[1][c1]), int(board[1][c2])
    return (t1 not in (0, 1) and t2 not in (0, 1)) or t1 < 0 or t2 < 0          # board.py:357-359


def record(shape, ci, att):
    """One attempt of a cell -> a record, or None when the attempt builds no board of the cell."""
    from tile_match_gym.board import Board, swap_coords
    R, C, k, smask = shape
    cell = sm.matrix_cells(shape)[ci]
    got = sm.board_of(shape, ci, att)
    if got is None:
        return None
    board, action, (t_cell, u_cell) = got
    if cell[0] == "pair" and sm.pair_key(shape, board, action) != sm.cell_key(shape, cell):
        return None
    if cell[0] == "chain" and sm.chain_key(shape, board, action, t_cell, u_cell) != sm.cell_key(shape, cell):
        return None
    cl, co = mg.specials_lists(smask)
    s = Board(R, C, k, cl, co, np.random.default_rng(0), board=board.astype(np.int32))
    c1, c2 = s.action_to_coords[action]
    s.num_specials_activated = 0
    s.num_new_specials = 0
    swap_coords(s.board, c1, c2)
    combo = takes_combination(s.board, c1, c2)
    assert combo == (cell[0] == "pair" or cell == ("cookie", sm.NONE_LEFT))
    err = 0
    try:
        signal.alarm(ALARM)
        if combo:
            s.combination_match(c1, c2)
        else:
            locs, names, cols = s.detect_colour_matches()
            assert locs
            s.resolve_colour_matches(locs, names, cols)
        signal.alarm(0)
    except mg.Timeout:
        signal.alarm(0)
        return None
    except Exception:
        signal.alarm(0)
        err = 1
    g = np.random.default_rng(sm.rng_seed_of(shape, ci, att))
    rng_in = mg.rng_state_words(g)
    b = Board(R, C, k, cl, co, g, board=board.astype(np.int32))
    try:
        signal.alarm(ALARM)
        out = b.move(c1, c2)
        signal.alarm(0)
    except mg.Timeout:
        signal.alarm(0)
        return None
    except Exception:
        signal.alarm(0)
        out, err = (0, False, 0, 0, False), 1
    return dict(shape=shape, cell=ci, attempt=att, kind={"pair": 0, "chain": 1, "cookie": 2}[cell[0]],
                t_cell=t_cell, u_cell=u_cell, board=board.astype(np.int8), action=action, rng_in=rng_in,
                mid=s.board.astype(np.int8), mid_n_act=int(s.num_specials_activated), mid_n_new=int(s.num_new_specials),
                out=b.board.astype(np.int8), rng_out=mg.rng_state_words(b.np_random),
                res=np.array([int(x) for x in out], np.int32), err=err)


def shape_records(shape):
    """The rows of a shape: per cell, its attempts in order up to the first
    that the reference finished and that shows the cell's feature."""
    cells = sm.matrix_cells(shape)
    recs = []
    chosen = {}
    for ci, cell in enumerate(cells):
        first = chosen[("cookie", sm.MID_CHAIN)] if cell == ("cookie", sm.MID_CHAIN_REVERSED) else 0
        for att in range(first, MAX_ATTEMPTS):
            r = record(shape, ci, att)
            if r is None:
                continue
            recs.append(r)
            if r["err"] == 0 and sm.shows_feature(shape, cell, r, recs):
                chosen[cell] = att
                break
            if cell == ("cookie", sm.MID_CHAIN_REVERSED):
                raise SystemExit(f"{shape}: the mirrored mid-chain row of attempt {att} does not show its feature")
            if r["err"] == 0:
                recs.pop()                   # finished, but not a row of this cell: not recorded
        else:
            raise SystemExit(f"{shape}: no attempt below {MAX_ATTEMPTS} covers cell {ci} {cell}")
    return recs


def write_deterministic(recs, path):
    """make_goldens.pack_records' layout, written as a zip whose bytes do not depend on the clock."""
    buf = io.BytesIO()
    mg.pack_records(recs, buf)
    buf.seek(0)
    z = np.load(buf, allow_pickle=False)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as out:
        for name in sorted(z.files):
            a = z[name]
            if a.dtype == np.int64 and name not in ("n",) and not name.endswith("_off"):
                a = a.astype(np.int32)
            raw = io.BytesIO()
            np.lib.format.write_array(raw, np.ascontiguousarray(a) if a.ndim else a, version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            out.writestr(info, raw.getvalue(), compresslevel=9)


def main():
    mg.install_stubs()
    import tile_match_gym  # noqa: F401
    want = set(sys.argv[1:])
    for shape in sm.SHAPES:
        if want and sm.shape_id(shape) not in want:
            continue
        t0 = time.time()
        recs = shape_records(shape)
        path = os.path.join(HERE, f"matrix_{sm.shape_id(shape)}.npz")
        write_deterministic(recs, path)
        print(f"matrix_{sm.shape_id(shape)}: {len(sm.matrix_cells(shape))} cells, {len(recs)} rows, "
              f"{sum(r['err'] for r in recs)} with err = 1, {os.path.getsize(path)} bytes, {time.time() - t0:.1f}s",
              flush=True)


if __name__ == "__main__":
    main()
