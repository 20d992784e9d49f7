"""The kernel-dispatch rule (csrc/tmg_dispatch.h): which step_kernel /
reset_kernel instantiation a call gets, and the route around it (lean or
general, the lane kernel, inline or deferred autoreset, the spill launch, the
envs per wave of a reset).  The library and the host wave emulator both run
this one rule; emu_route reports what it picks without launching anything.

The expected values are written out here, read off the dispatch code as it
stood when the rule was still spread over tmg_capi.hip, tmg_kernels.hip and
the emulator; none is computed by the code under test."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    return emu, emu.load()


def fix(R, C, k, smask):
    """A shape-specialised instantiation's FIX argument (shape_fix)."""
    return R << 24 | C << 16 | k << 8 | smask


NOFIX = 0
FIX_C2 = fix(10, 10, 4, 0)
FIX_C3 = fix(10, 10, 4, 14)          # vertical laser | horizontal laser | bomb
FIX_C5 = fix(20, 20, 6, 15)          # every special
FIX_RESET10 = fix(10, 10, 4, 255)    # any specials
FIX_RESET20 = fix(20, 20, 6, 255)
LANE = (0, 0, 0, 0, 0)               # no step_kernel instantiation: the lane kernel runs
LANE_MIN = 131072
FUSED = ("onehot", "terminated", "action_mask", "moves_left", "final_board", "board32")

# route fields: lean, lane, deferred, kernel_autoreset, spill, reset_epw
LEAN_INLINE = dict(lean=1, lane=0, deferred=0, kernel_autoreset=1, spill=0, reset_epw=0)
LANE_DEFERRED = dict(lean=1, lane=1, deferred=1, kernel_autoreset=2, spill=0, reset_epw=2)
GEN128 = dict(lean=0, lane=0, deferred=1, kernel_autoreset=2, spill=1, reset_epw=8)
GEN512 = dict(lean=0, lane=0, deferred=1, kernel_autoreset=2, spill=1, reset_epw=2)
LEAN512 = dict(lean=1, lane=0, deferred=1, kernel_autoreset=2, spill=0, reset_epw=2)

C2 = (10, 10, 4, 0)
# (R, C, k, smask), call (keyword arguments of emu.route), <MAXN, GEN, NB, CODD, FIX>, route
STEPS = [
    (C2, {}, (128, 0, 2, 0, FIX_C2), LEAN_INLINE),
    (C2, dict(mode=2), (128, 0, 2, 0, FIX_C2), dict(LEAN_INLINE, kernel_autoreset=3)),
    (C2, dict(n=LANE_MIN, have_lane=True), LANE, LANE_DEFERRED),
    (C2, dict(n=LANE_MIN, have_lane=True, mode=2), LANE, dict(LANE_DEFERRED, kernel_autoreset=4)),
    (C2, dict(n=LANE_MIN - 1, have_lane=True), (128, 0, 2, 0, FIX_C2), LEAN_INLINE),
    (C2, dict(policy=True, have_lane=True), LANE, LANE_DEFERRED),
    *[(C2, dict(policy=True, have_lane=True, fused=(f,)), (128, 0, 2, 0, FIX_C2), LEAN_INLINE) for f in FUSED],
    (C2, dict(n=LANE_MIN, have_lane=True, fused=("onehot",)), (128, 0, 2, 0, FIX_C2), LEAN_INLINE),
    (C2, dict(n=LANE_MIN, have_lane=False), (128, 0, 2, 0, FIX_C2), LEAN_INLINE),
    (C2, dict(policy=True, have_lane=False), (128, 0, 2, 0, FIX_C2), LEAN_INLINE),
    ((10, 10, 5, 0), dict(policy=True, have_lane=True), LANE, LANE_DEFERRED),
    ((10, 10, 6, 0), dict(policy=True, have_lane=True), (128, 0, 3, 0, NOFIX), LEAN_INLINE),
    (C2, dict(trust_eff=0), (128, 1, 2, 0, NOFIX), GEN128),
    (C2, dict(trust_eff=0, policy=True, n=LANE_MIN, have_lane=True), (128, 1, 2, 0, NOFIX), GEN128),
    ((10, 10, 4, 14), {}, (128, 1, 2, 0, FIX_C3), GEN128),
    ((10, 10, 4, 14), dict(mode=2), (128, 1, 2, 0, FIX_C3), dict(GEN128, kernel_autoreset=4)),
    ((10, 10, 4, 15), {}, (128, 1, 2, 0, NOFIX), GEN128),
    ((7, 5, 5, 0), {}, (128, 0, 3, 1, NOFIX), LEAN_INLINE),
    ((7, 5, 5, 15), {}, (128, 1, 3, 1, NOFIX), GEN128),
    ((8, 8, 3, 0), {}, (128, 0, 2, 0, NOFIX), LEAN_INLINE),
    ((6, 9, 9, 0), {}, (128, 0, 4, 1, NOFIX), LEAN_INLINE),
    ((3, 4, 2, 0), {}, (128, 0, 1, 0, NOFIX), LEAN_INLINE),
    ((2, 63, 6, 0), {}, (128, 0, 3, 1, NOFIX), LEAN_INLINE),        # bitboards up to C = 63
    ((2, 64, 4, 0), {}, (128, 0, 0, 0, NOFIX), LEAN_INLINE),        # none at C = 64
    ((2, 64, 4, 15), {}, (128, 1, 0, 0, NOFIX), GEN128),
    ((20, 20, 6, 15), {}, (512, 1, 0, 0, FIX_C5), GEN512),
    ((20, 20, 6, 0), {}, (512, 0, 0, 0, NOFIX), LEAN512),           # lean, but no inline generate at 512 cells
    ((20, 20, 6, 0), dict(mode=2), (512, 0, 0, 0, NOFIX), dict(LEAN512, kernel_autoreset=4)),
    ((16, 24, 7, 9), {}, (512, 1, 0, 0, NOFIX), GEN512),
    # no autoreset: code 0, nothing deferred, whatever the kernel
    (C2, dict(mode=0), (128, 0, 2, 0, FIX_C2), dict(LEAN_INLINE, kernel_autoreset=0)),
    (C2, dict(mode=0, n=LANE_MIN, have_lane=True), LANE,
     dict(LANE_DEFERRED, deferred=0, kernel_autoreset=0, reset_epw=0)),
    ((10, 10, 4, 14), dict(mode=0), (128, 1, 2, 0, FIX_C3), dict(GEN128, deferred=0, kernel_autoreset=0, reset_epw=0)),
    ((20, 20, 6, 15), dict(mode=0), (512, 1, 0, 0, FIX_C5), dict(GEN512, deferred=0, kernel_autoreset=0, reset_epw=0)),
    ((20, 20, 6, 0), dict(mode=0), (512, 0, 0, 0, NOFIX), dict(LEAN512, deferred=0, kernel_autoreset=0, reset_epw=0)),
]

# (R, C, k, smask), <MAXN, NB, CODD, FIX>, envs per wave of a masked reset
RESETS = [
    ((10, 10, 4, 0), (128, 2, 0, FIX_RESET10), 8),
    ((10, 10, 4, 14), (128, 2, 0, FIX_RESET10), 8),
    ((10, 10, 5, 0), (128, 3, 0, NOFIX), 8),
    ((20, 20, 6, 0), (512, 3, 0, FIX_RESET20), 2),
    ((20, 20, 6, 15), (512, 3, 0, FIX_RESET20), 2),
    ((7, 5, 5, 0), (128, 3, 1, NOFIX), 8),
    ((6, 9, 9, 0), (128, 4, 1, NOFIX), 8),
    ((3, 4, 2, 0), (128, 1, 0, NOFIX), 8),
    ((2, 64, 4, 0), (128, 0, 0, NOFIX), 8),
    ((16, 24, 7, 9), (512, 3, 0, NOFIX), 2),
    ((9, 15, 15, 0), (512, 4, 0, NOFIX), 2),
    ((12, 12, 2, 0), (512, 1, 0, NOFIX), 2),
    ((12, 12, 4, 0), (512, 2, 0, NOFIX), 2),
]


@pytest.mark.parametrize("case", range(len(STEPS)))
def test_step_route(emu_lib, case):
    emu, L = emu_lib
    shape, call, inst, want = STEPS[case]
    got, _ = emu.route(L, *shape, **call)
    what = f"{shape} {call}"
    assert tuple(got[f] for f in ("MAXN", "GEN", "NB", "CODD", "FIX")) == inst, what
    assert {f: got[f] for f in want} == want, what


@pytest.mark.parametrize("case", range(len(RESETS)))
def test_reset_route(emu_lib, case):
    emu, L = emu_lib
    shape, inst, masked = RESETS[case]
    for call in ({}, dict(trust_eff=0), dict(mode=0), dict(policy=True, have_lane=True)):   # a reset is none of their business
        _, got = emu.route(L, *shape, **call)
        assert tuple(got[f] for f in ("MAXN", "NB", "CODD", "FIX")) == inst, shape
        assert (got["epw_full"], got["epw_masked"]) == (1, masked), shape


# Every instantiation the ladders of csrc/tmg_dispatch.h name, written out by
# hand from that file.  step: <MAXN, GEN, NB, CODD, FIX>
ALL_STEPS = {
    # step_lean128_ladder: no bitboards (C = 64), c2, then NB x CODD
    (128, 0, 0, 0, NOFIX), (128, 0, 2, 0, FIX_C2),
    (128, 0, 1, 0, NOFIX), (128, 0, 2, 0, NOFIX), (128, 0, 3, 0, NOFIX), (128, 0, 4, 0, NOFIX),
    (128, 0, 1, 1, NOFIX), (128, 0, 2, 1, NOFIX), (128, 0, 3, 1, NOFIX), (128, 0, 4, 1, NOFIX),
    # step_gen128_even_ladder: no bitboards, c3, NB
    (128, 1, 0, 0, NOFIX), (128, 1, 2, 0, FIX_C3),
    (128, 1, 1, 0, NOFIX), (128, 1, 2, 0, NOFIX), (128, 1, 3, 0, NOFIX), (128, 1, 4, 0, NOFIX),
    # step_gen128_odd_ladder
    (128, 1, 1, 1, NOFIX), (128, 1, 2, 1, NOFIX), (128, 1, 3, 1, NOFIX), (128, 1, 4, 1, NOFIX),
    # step512_ladder: lean, c5, general
    (512, 0, 0, 0, NOFIX), (512, 1, 0, 0, FIX_C5), (512, 1, 0, 0, NOFIX),
}
# reset: <MAXN, NB, CODD, FIX>
ALL_RESETS = {
    # reset128_ladder: no bitboards, 10x10 k4, NB x CODD
    (128, 0, 0, NOFIX), (128, 2, 0, FIX_RESET10),
    (128, 1, 0, NOFIX), (128, 2, 0, NOFIX), (128, 3, 0, NOFIX), (128, 4, 0, NOFIX),
    (128, 1, 1, NOFIX), (128, 2, 1, NOFIX), (128, 3, 1, NOFIX), (128, 4, 1, NOFIX),
    # reset512_ladder: 20x20 k6, NB
    (512, 3, 0, FIX_RESET20),
    (512, 1, 0, NOFIX), (512, 2, 0, NOFIX), (512, 3, 0, NOFIX), (512, 4, 0, NOFIX),
}


def test_every_instantiation_is_run(emu_lib):
    """The shape lists of the GPU parity suites (test_gpu_parity's random-action
    rollouts, test_gpu_paths, the row-plane shapes, tests/dispatch_cases.py),
    with an untrusted mask where a test steps hand-set boards, launch every
    step_kernel and reset_kernel instantiation the ladders name, but for the
    one documented in dispatch_cases.NEVER_RUN_RESETS; and the bitboard lean
    cascade (sb_move: lean shapes outside the row-plane limits) keeps at least
    four shapes that can hold a vertical line."""
    import dispatch_cases as dc
    import rowplane_cases
    import test_gpu_parity
    import test_gpu_paths
    emu, L = emu_lib
    assert len(ALL_STEPS) == 23 and len(ALL_RESETS) == 15
    trusted = [c[:4] for c in test_gpu_parity.RANDOM_ACTION_CFGS]
    trusted += [v[:4] for v in test_gpu_paths.VARIANTS.values()]
    trusted += [(R, C, k, 0) for R, C, k in rowplane_cases.SHAPES]
    trusted += dc.CASES + [dc.ROW_PLANE_CONTROL]
    # test_gpu_rowplane.test_crafted_boards, test_gpu_dispatch_cover.test_crafted_tall_wide: the mask step
    untrusted = [(rowplane_cases.R10, rowplane_cases.C10, rowplane_cases.K10, 0)] + dc.CRAFTED_SHAPES
    steps, resets, sb_move = set(), set(), set()
    for shape, call in [(s, {}) for s in trusted] + [(s, dict(trust_eff=0)) for s in untrusted]:
        st, rt = emu.route(L, *shape, **call)
        assert not st["lane"]
        steps.add(tuple(st[f] for f in ("MAXN", "GEN", "NB", "CODD", "FIX")))
        resets.add(tuple(rt[f] for f in ("MAXN", "NB", "CODD", "FIX")))
        R, C = shape[:2]
        if st["lean"] and st["MAXN"] == 128 and st["NB"] > 0 and not (R <= 16 and C <= 28) and R >= 3:
            sb_move.add(shape)
    never = {(m, nb, codd, NOFIX) for m, nb, codd, _ in dc.NEVER_RUN_RESETS}
    assert len(never) <= 1 and never <= ALL_RESETS
    assert steps == ALL_STEPS, f"never launched: {sorted(ALL_STEPS - steps)}, not in the ladders: {sorted(steps - ALL_STEPS)}"
    assert resets == ALL_RESETS - never, (f"never launched: {sorted(ALL_RESETS - never - resets)}, "
                                          f"not expected: {sorted(resets - (ALL_RESETS - never))}")
    assert len(sb_move) >= 4, sorted(sb_move)


def test_every_instantiation_runs_with_fused_outputs(emu_lib):
    """tests/fused_cases.py (test_gpu_fused.py on the device, test_fused_emulated.py
    on the emulator) attaches every fused output of tmg_plan_config, in every
    autoreset mode, and steps twice untrusted after a hand edit: together those
    calls launch every step_kernel instantiation, and reach every reset_kernel
    one as a deferred autoreset (but for dispatch_cases.NEVER_RUN_RESETS), with
    the outputs attached.  None goes to the lane kernel, which writes no fused
    output: the policy steps stay on the wave kernels."""
    import dispatch_cases as dc
    import fused_cases as fc
    emu, L = emu_lib
    assert fc.MODE_CODE == {"none": 0, "same_step": 1, "next_step": 2}
    steps, deferred = set(), set()
    for shape in fc.SHAPES:
        for mode in fc.MODES:
            calls = [dict(), dict(policy=True), dict(trust_eff=0)]      # the plain, the policy and the hand-edit steps
            for call in calls:
                for n in (67, 203, LANE_MIN):                            # the tests' batches; and were they large
                    st, rt = emu.route(L, *shape, mode=fc.MODE_CODE[mode], n=n, have_lane=True, fused=FUSED, **call)
                    assert not st["lane"], (shape, mode, call, n)
                    if n == LANE_MIN:
                        continue
                    steps.add(tuple(st[f] for f in ("MAXN", "GEN", "NB", "CODD", "FIX")))
                    if st["deferred"]:
                        assert mode != "none"
                        deferred.add(tuple(rt[f] for f in ("MAXN", "NB", "CODD", "FIX")))
    never = {(m, nb, codd, NOFIX) for m, nb, codd, _ in dc.NEVER_RUN_RESETS}
    assert len(ALL_STEPS) == 23
    assert steps == ALL_STEPS, f"never launched: {sorted(ALL_STEPS - steps)}, not in the ladders: {sorted(steps - ALL_STEPS)}"
    assert deferred == ALL_RESETS - never, (f"never deferred: {sorted(ALL_RESETS - never - deferred)}, "
                                            f"not expected: {sorted(deferred - (ALL_RESETS - never))}")


# The route classes tests/extent_cases.py EXTENT_SHAPES are there for, written out by
# hand: name -> what one of the shapes has to reach.  step / untrusted / reset / peek:
# the instantiation of a trusted step, of a step with trust_eff = 0, of a reset, of a
# trusted peek; route: fields of the trusted same-step route; A, bytes2N: the action
# count and the bytes of a board; lane: the lane kernel takes the in-kernel policy at
# every batch size of the shape and at LANE_SMALL + 1, and given actions at LANE_MIN + 1.
EXTENT_CLASSES = {
    "lean bitboard, odd C, byte stores": dict(step=(128, 0, 1, 1, NOFIX), reset=(128, 1, 1, NOFIX), route=LEAN_INLINE,
                                              peek=(128, 0, 1, 1), A=22, bytes2N=30),
    "general bitboard, odd C": dict(step=(128, 1, 3, 1, NOFIX), reset=(128, 3, 1, NOFIX), route=GEN128,
                                    peek=(128, 1, 3, 1), bytes2N=126),
    "c2 and the lane kernel, k = 4": dict(step=(128, 0, 2, 0, FIX_C2), reset=(128, 2, 0, FIX_RESET10), route=LEAN_INLINE,
                                          lane=True),
    "the lane kernel, k = 5": dict(step=(128, 0, 3, 0, NOFIX), reset=(128, 3, 0, NOFIX), route=LEAN_INLINE, lane=True),
    "c3, deferred reset at 8 envs per wave, spill": dict(step=(128, 1, 2, 0, FIX_C3), reset=(128, 2, 0, FIX_RESET10),
                                                         route=GEN128),
    "A = 64, lean": dict(step=(128, 0, 2, 0, NOFIX), route=LEAN_INLINE, A=64),
    "A = 64, general": dict(step=(128, 1, 2, 0, NOFIX), route=GEN128, A=64),
    "no bitboards": dict(step=(128, 0, 0, 0, NOFIX), untrusted=(128, 1, 0, 0, NOFIX), reset=(128, 0, 0, NOFIX),
                         peek=(128, 0, 0, 0)),
    "c5, deferred reset at 2 envs per wave, spill": dict(step=(512, 1, 0, 0, FIX_C5), reset=(512, 3, 0, FIX_RESET20),
                                                         route=GEN512, peek=(512, 1, 0, 0)),
    "lean 512-cell": dict(step=(512, 0, 0, 0, NOFIX), reset=(512, 4, 0, NOFIX), route=LEAN512, peek=(512, 0, 0, 0)),
}


def _reaches(emu, L, shape, sizes, want):
    """Whether the shape reaches the class `want` of EXTENT_CLASSES."""
    R, C = shape[:2]
    st, rt = emu.route(L, *shape)
    ut, _ = emu.route(L, *shape, trust_eff=0)
    inst = lambda r: tuple(r[f] for f in ("MAXN", "GEN", "NB", "CODD", "FIX"))      # noqa: E731
    ok = inst(st) == want["step"]
    if "untrusted" in want:
        ok &= inst(ut) == want["untrusted"] and ut["spill"] == 1
    if "reset" in want:
        ok &= tuple(rt[f] for f in ("MAXN", "NB", "CODD", "FIX")) == want["reset"]
    if "route" in want:
        ok &= {f: st[f] for f in want["route"]} == want["route"]
    if "peek" in want:
        ok &= tuple(emu.peek_route(L, *shape)[f] for f in emu.PEEK_ROUTE) == want["peek"]
    if "A" in want:
        ok &= 2 * R * C - R - C == want["A"]
    if "bytes2N" in want:
        ok &= 2 * R * C == want["bytes2N"]
    lane = all(emu.route(L, *shape, n=n, have_lane=True, policy=True, mode=mode)[0]["lane"] == 1
               for n in sizes + (32769,) for mode in (1, 2))
    given = emu.route(L, *shape, n=LANE_MIN + 1, have_lane=True)[0]
    return ok and lane == (given["lane"] == 1) == want.get("lane", False)


def test_extent_shapes_reach_every_route_class(emu_lib):
    """tests/extent_cases.py EXTENT_SHAPES (test_gpu_extent.py on the device,
    tools/wave_emu/extent_asan.cpp on the host) has one row per class of
    EXTENT_CLASSES, and each class is reached by exactly one row: deleting a row
    leaves a class without a shape.  The batch sizes are the ragged ones (1, 9,
    65; 1, 3, 9 on 512-cell boards; 1, 9 where the oracle generates slowly), the
    masked resets run at 8 and at 2 envs per wave, 2 also behind the lane kernel,
    and the lane cases of the device test are the lane kernel's."""
    import extent_cases as ec
    import fused_cases as fc
    emu, L = emu_lib
    assert len(set(ec.EXTENT_SHAPES)) == len(ec.EXTENT_SHAPES)
    for name, want in EXTENT_CLASSES.items():
        hits = [s for s in ec.EXTENT_SHAPES if _reaches(emu, L, s, ec.batch_sizes(s), want)]
        assert len(hits) == 1, f"{name}: reached by {hits}"
    for s in ec.EXTENT_SHAPES:
        want = (1, 9) if s in fc.SLOW else (1, 9, 65) if s[0] * s[1] <= 128 else (1, 3, 9)
        assert ec.batch_sizes(s) == want, s
    assert {(s, n) for s in ec.EXTENT_SHAPES for n in ec.batch_sizes(s)} == set(ec.CASES)
    assert set(ec.GROUPS) == set(ec.RUN) and len(ec.GROUPS) == 7
    # envs per wave of the deferred resets: 8 and 2 behind the wave kernels, 2 behind the lane kernel
    epw = {(bool(st["lane"]), st["reset_epw"]) for s in ec.EXTENT_SHAPES for pol in (False, True)
           for st in [emu.route(L, *s, n=9, have_lane=True, policy=pol)[0]] if st["deferred"]}
    assert epw == {(False, 8), (False, 2), (True, 2)}, epw
    assert {emu.route(L, *s)[1]["epw_masked"] for s in ec.EXTENT_SHAPES} == {8, 2}
    # the lane cases: 32 envs per wave below LANE_SMALL, 64 from there on, and the given-action route past LANE_MIN
    assert (ec.LANE_SMALL, ec.LANE_MIN) == (32768, LANE_MIN)
    assert set(ec.LANE_CASES) == {(s, n) for s in [(10, 10, 4, 0), (10, 10, 5, 0)] for n in (1, 9, 65, 32769)}
    for s, n in ec.LANE_CASES:
        for mode in (1, 2):
            st, _ = emu.route(L, *s, n=n, have_lane=True, policy=True, mode=mode)
            assert (st["lane"], st["deferred"], st["reset_epw"]) == (1, 1, 2), (s, n, mode)
    st, _ = emu.route(L, 10, 10, 4, 0, n=ec.LANE_MIN + 1, have_lane=True)        # test_extent_lane_given_actions
    assert (st["lane"], st["deferred"], st["reset_epw"]) == (1, 1, 2)
    assert set(ec.SPILL_SHAPES) == {(10, 10, 4, 14), (20, 20, 6, 15)} <= set(ec.EXTENT_SHAPES)
    for s in ec.SPILL_SHAPES:
        assert emu.route(L, *s, trust_eff=0)[0]["spill"] == 1
