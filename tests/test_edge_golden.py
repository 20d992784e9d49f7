"""Pins the CPU oracle (oracle/tmg_oracle.c) to the reference at the shape
limits: the fixtures of tests/golden/edge/ (tests/edge_cases.py, recorded by
tests/golden/make_edge_goldens.py) through the checks of
tests/test_oracle_golden.py, and a census of what those fixtures cover.  No
GPU needed."""
import os

import numpy as np
import pytest

import edge_cases as ec
import test_oracle_golden as tog
from golden_io import GOLDEN, load_records, load_traj, traj_names, replay_trajectory


def edge_records(kind, group):
    return load_records(kind, f"fn_{group}", ec.SUB)


@pytest.mark.parametrize("group", list(ec.GROUPS))
def test_edge_function_records_oracle(group):
    """lines, process, effective, gravity, activate, combo, resolve, move and
    generate records of every shape of the group.  The counts: 8 records of
    each of lines / effective / gravity / resolve / move per shape were
    recorded and the reference raised in none of them, so every one is
    compared; half the line records are drawn from k - 1 colours, which is
    where the bound of one processed line per two records comes from."""
    shapes = ec.fn_shapes(group)
    n = ec.FN_PER_SHAPE * len(shapes)
    recs = {kind: edge_records(kind, group) for kind in ec.FN_KINDS}
    for kind in ("lines", "effective", "gravity", "resolve", "move"):
        assert len(recs[kind]) == n, kind
        assert {(r["R"], r["C"], r["k"], r["smask"]) for r in recs[kind]} == set(shapes), kind
    tog.check_get_colour_lines(recs["lines"])
    assert not any(r["perr"] for r in recs["lines"]) and not any(r["err"] for r in recs["resolve"] + recs["move"])
    tog.check_process_colour_lines(recs["lines"], n // 2)
    tog.check_is_move_effective(recs["effective"])
    tog.check_gravity(recs["gravity"])
    tog.check_activate_special(recs["activate"])
    tog.check_combination_match(recs["combo"])
    tog.check_detect_resolve(recs["resolve"], n - 1)
    tog.check_move(recs["move"], n - 1)
    tog.check_generate_board(recs["generate"])
    assert len(recs["generate"]) == 2 * len(shapes)
    with_specials = sum(1 for s in shapes if s[3])
    assert len(recs["activate"]) > 4 * with_specials and len(recs["combo"]) > 4 * with_specials


@pytest.mark.parametrize("name,shape", ec.traj_cases(), ids=[n for n, _ in ec.traj_cases()])
@pytest.mark.parametrize("autoreset", [False, True])
def test_edge_trajectory_oracle(name, shape, autoreset):
    """tile_match_env.py:84-124 whole trajectories (RNG-exact), two resets in each."""
    d = load_traj(name, ec.SUB)
    assert (d["R"], d["C"], d["k"], d["smask"]) == shape and d["num_moves"] == ec.NUM_MOVES
    n = replay_trajectory(d, tog._OracleBackend(d, threads=2), autoreset)
    seeds, steps = ec.TRAJ[name[0]]
    assert n >= len(seeds) * steps


def test_edge_census():
    """What the files of tests/golden/edge/ cover, counted from the files
    themselves: deleting a fixture fails here (or in the list comparison)
    instead of silently shrinking the cover."""
    names = traj_names(ec.SUB)
    assert names == sorted(n for n, _ in ec.traj_cases())
    shapes = []
    for n in names:
        R, C, k, sm, _ = (int(x) for x in np.load(os.path.join(GOLDEN, ec.SUB, f"traj_{n}.npz"))["shape"])
        shapes.append((R, C, k, sm))
    assert sorted(shapes) == sorted(ec.GROUP_A + ec.GROUP_B)
    files = {f for f in os.listdir(os.path.join(GOLDEN, ec.SUB)) if f.startswith("fn_")}
    assert files == {f"fn_{g}_{kind}.npz" for g in ec.GROUPS for kind in ec.FN_KINDS}

    def some(pred):
        return any(pred(*s) for s in shapes)

    assert some(lambda R, C, k, sm: R == 1 and sm == 0) and some(lambda R, C, k, sm: R == 1 and sm == 15)
    assert some(lambda R, C, k, sm: C == 1 and sm == 0) and some(lambda R, C, k, sm: C == 1 and sm != 0)
    assert some(lambda R, C, k, sm: R == 64 and sm == 0) and some(lambda R, C, k, sm: R == 64 and sm == 15)
    assert some(lambda R, C, k, sm: R > 42 and R * C <= 128)             # past dispatch_cases' tallest
    assert (2, 64, 4, 0) in shapes and (2, 64, 4, 15) in shapes          # C = 64 where a row fills a word
    assert some(lambda R, C, k, sm: C == 64 and R == 1)
    assert some(lambda R, C, k, sm: R * C == 512 and sm == 0) and some(lambda R, C, k, sm: R * C == 512 and sm == 15)
    assert some(lambda R, C, k, sm: ec.mask_words((R, C)) == 16)
    assert some(lambda R, C, k, sm: k == 15 and sm == 0) and some(lambda R, C, k, sm: k == 15 and sm == 15)
    assert some(lambda R, C, k, sm: k == 15 and R * C == 512)
    # the function-level records reach the same limits
    fn = {(r["R"], r["C"], r["k"], r["smask"]) for g in ec.GROUPS for r in edge_records("move", g)}
    assert fn == set(ec.fn_shapes("a")) | set(ec.fn_shapes("b"))
    for s in ec.LOOKAHEAD_DEVICE:
        assert s in ec.GROUP_B
    # recorded shuffles inside moves (flags bit 2), where k makes them likely
    for s in [(2, 63, 9, 0), (7, 9, 10, 15), (6, 8, 12, 0), (6, 20, 15, 15), (9, 15, 15, 0)]:
        d = load_traj(ec.traj_name("a", s), ec.SUB)
        assert (d["flags"][d["kind"] == 1] & 4).any(), s
