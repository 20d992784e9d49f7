"""Shapes that run the kernel instantiations and boundaries no other parity
list reaches (csrc/tmg_dispatch.h names the instantiations, tmg_rp.hip /
tmg_sb.hip the boundaries).  Shared by tests/test_gpu_dispatch_cover.py (the
device), tests/test_kernel_emulated.py and tests/test_overflow.py (the host
wave emulator) and the census of tests/test_dispatch_route.py, which fails
when a row that is the only cover of an instantiation is deleted.
tests/fused_cases.py takes the whole list again for the fused step outputs
(tests/test_gpu_fused.py, tests/test_fused_emulated.py and a census of their own).

The row-plane cascade (rp_move) takes every lean move with R <= 16 and
C <= 28; sb_move keeps the other no-specials boards of <= 128 cells with
C <= 63, i.e. the tall and the wide ones.

k = 2 only on boards of <= 16 cells: on larger ones generate_board
(board.py:95-109) redraws almost forever, a line-free two-colour board being
so rare (3x42 k2 does not finish in 25 s on the host; 12x12 k2 neither)."""

# (R, C, k, smask); step<MAXN, GEN, NB, CODD> / reset<MAXN, NB, CODD> in the comments
LEAN_TALL_WIDE = [
    (17, 7, 4, 0),      # first R past the row-plane limit (kRpMaxR = 16); odd C, 2 planes: <128,0,2,1>
    (42, 3, 3, 0),      # tallest board of <= 128 cells: vertical runs up to 42
    (32, 4, 5, 0),      # 128 cells exactly, even C, sb_row's largest shift, 3 planes: <128,0,3,0>
    (21, 6, 9, 0),      # 4 planes, even C: <128,0,4,0>, reset<128,4,0>
    (4, 29, 4, 0),      # first C past kRowScanMaxC = 28: scan_effective_clean instead of scan_rows
    (4, 32, 7, 0),      # last C of bp_generate, 128 cells
    (3, 33, 5, 0),      # first C of sb_generate_exact in the inline autoreset; <128,0,3,1>
    (2, 63, 9, 0),      # 4 planes at the word limit; shuffles in moves: <128,0,4,1>
]
GENERAL_TALL_WIDE = [   # the same boundaries on the general bitboard kernels (sb_simple_step, closures, lists)
    (17, 7, 4, 15),     # <128,1,2,1>; vertical runs and v-laser columns of 17
    (42, 3, 3, 14),     # v-laser columns of 42
    (3, 33, 5, 15),     # generate_board draw by draw in reset<128,3,1>; h-laser rows of 33
    (2, 63, 6, 15),     # rows at the word limit
    (4, 32, 7, 9),      # <128,1,3,0>, 128 cells
    (21, 6, 9, 14),     # 4 planes, even C: <128,1,4,0>
    (7, 9, 10, 15),     # 4 planes, odd C: <128,1,4,1>; shuffles
]
PLANES = [              # plane counts no other list runs
    (3, 5, 2, 0),       # lean, 1 plane, odd C: <128,0,1,1>, reset<128,1,1>
    (4, 4, 2, 15),      # general, 1 plane, even C: <128,1,1,0>
    (3, 5, 2, 15),      # general, 1 plane, odd C: <128,1,1,1>
    (6, 8, 12, 0),      # lean (row planes), 4 planes, even C; many shuffles
]
NO_BITBOARD = [         # C = 64: a row does not fit a word
    (2, 64, 4, 0),      # <128,0,0,0>, reset<128,0,0>
    (2, 64, 4, 15),     # <128,1,0,0>
]
FAMILY_512 = [
    (3, 43, 5, 0),      # 129 cells, the smallest board of the family, C > 32; <512,0,0,0>, reset<512,3>
    (3, 43, 5, 15),     # <512,1,0,0>
    (12, 12, 4, 0),     # reset<512,2>
]
# reset<512,1> needs k = 2 on a board of > 128 cells, whose generate_board does
# not end (above); a masked reset of hand-set boards regenerates them just the
# same.  It is the one instantiation no test launches.
NEVER_RUN_RESETS = {(512, 1, 0, 0)}

ROW_PLANE_CONTROL = (10, 10, 5, 0)      # R <= 16, C <= 28: rp_move, never sb_move

CASES = LEAN_TALL_WIDE + GENERAL_TALL_WIDE + PLANES + NO_BITBOARD + FAMILY_512
LEAN = [s for s in CASES if s[3] == 0]
SHUFFLES = [(2, 63, 9, 0), (7, 9, 10, 15), (6, 8, 12, 0)]              # CV_SHUFFLE must count
# boards of <= 128 cells with C > 32 on the bitboard kernels: generate_board
# runs draw by draw (sb_generate_exact), crafted rejections are replayed there
WIDE_EXACT = [(3, 33, 5, 0), (2, 63, 9, 0), (3, 33, 5, 15), (2, 63, 6, 15)]
# hand-built boards (test_crafted_tall_wide): their first step runs untrusted,
# i.e. on the general kernel of the shape
CRAFTED_SHAPES = [(42, 3, 3, 0), (17, 7, 4, 0), (2, 63, 6, 0), (4, 32, 7, 0), (17, 7, 4, 14), (3, 33, 5, 15)]
MASKED_RESET = [(2, 64, 4, 0), (42, 3, 3, 0), (3, 33, 5, 0), (12, 12, 4, 0), (3, 43, 5, 15)]


def case_id(s):
    return "{}x{}k{}s{}".format(*s)
