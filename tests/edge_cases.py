"""Shapes at the limits of what tmg_create accepts (R <= 64, C <= 64,
R * C <= 512, k <= 15) and at the boundaries the kernels change on, recorded
from the reference itself by tests/golden/make_edge_goldens.py into
tests/golden/edge/.  Shared by the recorder, tests/test_edge_golden.py (the
oracle and the census), tests/test_kernel_emulated.py (the host wave emulator)
and tests/test_gpu_edge.py (the device).

Group A: the dispatch boundaries (tests/dispatch_cases.py), until now compared
with the oracle only.  Group B: one-row and one-column boards, 64 rows, 64
columns, 512 cells, the 16-word action mask, k = 15.

Not recorded, the reference's generate_board (board.py:95-131) not finishing in
240 s: 8x64 (k 5 and 6; the only 512-cell board with C = 64) and 1x4 / 4x1 k3.
The oracle's reset of 8x64 does not finish either (make_edge_goldens.py
--probe-8x64: OracleBatch.reset() of one board, seed 100, was still redrawing
after 60 s for k 5 and for k 6), so no test runs 8x64; C = 64 is covered by
2x64 and 1x64."""
import dispatch_cases as dc

SUB = "edge"            # the fixtures' folder under tests/golden/

# (R, C, k, smask)
GROUP_A = list(dc.CASES) + [dc.ROW_PLANE_CONTROL, (9, 15, 15, 0), (6, 20, 15, 15), (16, 28, 8, 0)]
GROUP_B = [
    (1, 13, 2, 0), (1, 20, 4, 15), (1, 64, 5, 0), (1, 64, 5, 15),       # one row: A = C - 1, all horizontal
    (20, 1, 4, 0), (64, 1, 3, 14),                                      # one column: A = R - 1, all vertical
    (64, 2, 4, 15), (64, 3, 4, 0), (43, 3, 3, 14),                      # 64 rows; the first R past 42
    (64, 8, 6, 15), (64, 8, 5, 0), (64, 8, 15, 15),                     # 512 cells, 64 rows
    (16, 32, 7, 15), (32, 16, 7, 0),                                    # 512 cells, 16 mask words
    (22, 23, 6, 15),                                                    # 506 cells, 967 actions: 16 mask words
]
GROUPS = {"a": GROUP_A, "b": GROUP_B}
# trajectories: seeds, steps; num_moves 12 and p_eff 0.7 for both
TRAJ = {"a": (range(100, 104), 30), "b": (range(100, 103), 26)}
NUM_MOVES, P_EFF = 12, 0.7
FN_PER_SHAPE = 8
FN_KINDS = ("lines", "effective", "gravity", "activate", "combo", "resolve", "move", "generate")

case_id = dc.case_id


def traj_name(group, shape):
    return f"{group}_{case_id(shape)}"


def traj_cases():
    """[(fixture name, shape)] of every recorded trajectory."""
    return [(traj_name(g, s), s) for g, shapes in GROUPS.items() for s in shapes]


def fn_shapes(group):
    """The shapes of a group's function-level records: two colours on <= 16
    cells are left out (most such boards have no line-free arrangement for
    generate_board to find, dispatch_cases.py)."""
    return [s for s in GROUPS[group] if not (s[0] * s[1] <= 16 and s[2] == 2)]


def mask_words(shape):
    R, C = shape[:2]
    return (2 * R * C - R - C + 63) // 64


# Trajectories the host wave emulator does not replay (tests/test_kernel_emulated.py):
# name -> seconds one replay took on the build machine (the limit is about 20 s).
# Every board of <= 128 cells is replayed; the oracle and the device skip none.
# Measured, both autoreset settings: 22x23 k6 19.6 / 17.6 s, 16x32 k7 10.7 / 10.1 s,
# every other one under 2 s: none is left out.
EMU_SLOW = {}

# tmg_peek / tmg_rollout / tmg_expand against the oracle, on the device only:
# A = 63 all horizontal, A = 63 all vertical, 64 rows of 8, and 16 mask words
# (peek's best action, expand's mask rows)
LOOKAHEAD_DEVICE = [(1, 64, 5, 15), (64, 1, 3, 14), (64, 8, 6, 15), (22, 23, 6, 15)]
