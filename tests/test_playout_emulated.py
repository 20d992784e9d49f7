"""tmg_playout on the host wave emulator (CPU): the playout kernels of
csrc/tmg_playout.hip, picked by peek_ladder (csrc/tmg_dispatch.h) and followed
by the playout spill pass and the reduce kernel of csrc/tmg_aux.hip, against
the oracle's mask and move of every (sequence, env, ply)
(tests/playout_cases.py oracle_playout).  Everything is compared as integers
and bytes; nothing here has a tolerance.  The cases are those of
tests/test_gpu_playout.py that need no device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import peek_cases
import playout_cases as pc
from playout_cases import assert_playout_equal, oracle_playout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")
MOVES = pc.MOVES


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    L = emu.load()
    L.emu_status_clear()
    return emu, L


def _playout(emu, L, shape, board, rng, timer, eff, trust_eff, actions, **kw):
    R, C, k, sm = shape
    return emu.playout(L, R, C, k, sm, MOVES, board, rng, timer, eff, trust_eff, actions, **kw)


@pytest.mark.parametrize("shape", peek_cases.SHAPES + peek_cases.LIMIT_SHAPES, ids=pc.case_id)
def test_playout_vs_oracle(emu_lib, shape):
    """Case 1, and case 3 on the same calls.  After 7 uniform-random steps
    (boards that hold specials) and after a reset; env 0 two moves from the end
    of its episode and, after the reset, the last env at its end; the five
    sequences of playout_cases.sequences_of, the last with RNG words of its
    own.  Every output and final-state array; no input is written."""
    emu, L = emu_lib
    for steps in (7, 0):
        case = pc.vs_oracle_case(shape, steps)
        o, timer, acts, rng, want, _ = case
        pc.check_vs_oracle_conditions(shape, case)
        ins = (o.board.copy(), rng.copy(), timer.copy(), o.eff.copy(), acts.copy())
        before = [x.copy() for x in ins]
        got = _playout(emu, L, shape, *ins[:4], 1, ins[4])
        assert_playout_equal(got, want, f"{shape} steps={steps}")
        assert all(np.array_equal(x, y) for x, y in zip(ins, before)), "an input was written"
    assert L.emu_status() == 0


def test_playout_shared_words(emu_lib):
    """rng (n, 5): every sequence of an env starts from the same words, so two
    equal sequences give equal rows; timer None: no horizon, no DONE."""
    emu, L = emu_lib
    shape = (10, 10, 4, 14)
    o, timer, acts, rng, _, _ = pc.vs_oracle_case(shape, 7)
    acts = np.stack([acts[0], acts[1], acts[0]])
    want = oracle_playout(o.board, o.rng, None, MOVES, o.k, o.smask, acts)
    fields = tuple(f for f in pc.FIELDS if f != "out_timer")
    got = _playout(emu, L, shape, o.board, o.rng, None, o.eff, 1, acts, fields=fields)
    assert_playout_equal(got, want, str(shape), fields)
    assert (want["plies"][:, 0] == pc.D).all() and not (want["flags"] & pc.FLAG_DONE).any()
    assert np.array_equal(got["out_board"].reshape(3, o.n, -1)[0], got["out_board"].reshape(3, o.n, -1)[2])
    assert L.emu_status() == 0


@pytest.mark.parametrize("shape", [(10, 10, 4, 0), (10, 10, 4, 14), (20, 20, 6, 15)], ids=pc.case_id)
def test_playout_bad_action(emu_lib, shape):
    """Case 5: an action >= A at ply 2 of sequence 0 of env 1.  That row carries
    ERROR and plies == 2 with the state as ply 1 left it (the oracle's walk of
    the first two actions); STATUS_CALLER; every other row as without it."""
    emu, L = emu_lib
    o, timer, acts, rng, clean, _ = pc.vs_oracle_case(shape, 7)
    bad = acts.copy()
    bad[0, 1, 2] = o.A
    want = oracle_playout(o.board, rng, timer, MOVES, o.k, o.smask, bad)
    assert want["flags"][0, 1] & pc.FLAG_ERROR and want["plies"][0, 1] == 2
    cut = acts.copy()
    cut[0, 1, 2:] = -1                                       # the same state by padding instead
    padded = oracle_playout(o.board, rng, timer, MOVES, o.k, o.smask, cut)
    assert np.array_equal(want["out_board"], padded["out_board"]) and np.array_equal(want["out_rng"], padded["out_rng"])
    got = _playout(emu, L, shape, o.board, rng, timer, o.eff, 1, bad)
    assert_playout_equal(got, want, str(shape))
    assert L.emu_status_clear() == pc.STATUS_CALLER
    others = np.ones((pc.Q, o.n), bool)
    others[0, 1] = False
    for f in ("ret", "plies", "flags"):
        assert np.array_equal(got[f][others], clean[f][others]), f
    assert np.array_equal(got["out_board"][others.reshape(-1)], clean["out_board"][others.reshape(-1)])


@pytest.mark.parametrize("shape,seed0,n", pc.SHUFFLE_CASES, ids=[pc.case_id(c[0]) for c in pc.SHUFFLE_CASES])
def test_playout_shuffle_at_later_ply(emu_lib, shape, seed0, n):
    """Case 6: boards that go dead inside a sequence (asserted on the oracle first)."""
    emu, L = emu_lib
    o, acts, want, at = pc.shuffle_case(shape, seed0, n)
    assert any(d >= 1 for d in at), f"{shape}: no move at a ply >= 1 shuffles on the oracle"
    assert (want["flags"] & pc.FLAG_SHUFFLED).any()
    got = _playout(emu, L, shape, o.board, o.rng, o.timer, o.eff, 1, acts)
    assert_playout_equal(got, want, str(shape))
    assert L.emu_status() == 0


@pytest.mark.parametrize("shape,mode,many", peek_cases.spill_params(device=False))
def test_playout_untrusted_and_spill(emu_lib, shape, mode, many):
    """Case 7: hand-written boards (they may hold lines and any special),
    trust_eff = 0 and no mask given: the frame scans its own mask, ply 0
    searches the whole board for lines, the general kernels run, and a virtual
    env one of whose plies outgrows the LDS lists is re-run whole by the spill
    pass.  Sequence 0 follows the oracle's masks, sequence 1 is uniform, and
    with `many` there are more spilling virtual envs than the spill pass has
    waves."""
    emu, L = emu_lib
    R, C, k, sm = shape
    n = peek_cases.MANY_SPILLS[shape][1] if many else peek_cases.envs_of(shape)
    b, words, acts = pc.adversarial_case(shape, mode, n)
    want = oracle_playout(b, words, None, MOVES, k, sm, acts)
    fields = tuple(f for f in pc.FIELDS if f != "out_timer")
    s0 = L.emu_spills()
    got = _playout(emu, L, shape, b, words, None, None, 0, acts, fields=fields)
    assert_playout_equal(got, want, f"{shape} {mode}", fields)
    assert L.emu_status() == 0
    if (R, C) in ((20, 20), (10, 10)) and mode != "stripes":
        assert L.emu_spills() > s0, "the adversarial boards were meant to outgrow the LDS lists"
    if many:
        assert L.emu_spills() - s0 > peek_cases.SPILL_WAVES


@pytest.mark.parametrize("shape", pc.LINE_SHAPES, ids=pc.case_id)
def test_playout_line_after_ineffective_ply(emu_lib, shape):
    """Case 7, the boards that already hold a line: trust_eff = 0, an
    ineffective first ply, then an effective one, which still starts from the
    caller's board and has to search all of it for lines."""
    emu, L = emu_lib
    case = pc.line_case(shape)
    pc.check_line_conditions(shape, case)
    b, words, acts, want, _ = case
    fields = tuple(f for f in pc.FIELDS if f != "out_timer")
    got = _playout(emu, L, shape, b, words, None, None, 0, acts, fields=fields)
    assert_playout_equal(got, want, str(shape), fields)
    assert L.emu_status() == 0


def test_playout_reduce(emu_lib):
    """Case 8: Q = 130, ties planted on the oracle's best (same lane of the
    reduce kernel and another), the lowest q wins; an env whose sequences are
    all ineffective reports sequence 0, return 0."""
    emu, L = emu_lib
    case = pc.reduce_case()
    pc.check_reduce_conditions(case)
    o, acts, want = case
    got = _playout(emu, L, pc.REDUCE_SHAPE, o.board, o.rng, o.timer, o.eff, 1, acts)
    assert_playout_equal(got, want, "reduce")
    assert L.emu_status() == 0


def test_playout_refusals_and_noops(emu_lib):
    """Case 10, the argument checks the emulator's entry point shares with the
    library: each refusal of the list, and n == 0."""
    emu, L = emu_lib
    shape = (10, 10, 4, 0)
    R, C, k, sm = shape
    o, timer, acts, rng, want, _ = pc.vs_oracle_case(shape, 7)
    n, A, W = o.n, o.A, o.W
    acts = np.ascontiguousarray(acts)
    ret, best = np.zeros((pc.Q, n), np.int32), np.zeros(n, np.int32)
    ot = np.zeros(pc.Q * n, np.int32)
    ob = np.zeros(pc.Q * n * 2 * R * C + 8, np.int8)
    ob = ob[(-ob.ctypes.data) % 8:]                          # 8-byte aligned

    def call(n=n, board=o.board, rng=o.rng, timer=timer, eff=o.eff, trust=1, q=pc.Q, d=pc.D, acts=acts, ret=ret,
             out_board=None, out_timer=None, best_seq=None):
        p = lambda a: None if a is None else a.ctypes.data          # noqa: E731
        return L.emu_playout(R, C, k, sm, MOVES, n, p(board), p(rng), 0, p(timer), p(eff), trust, q, d, p(acts),
                             p(ret), None, None, None, None, None, p(out_board), None, p(out_timer), None,
                             p(best_seq), None)

    assert call() == 0
    assert np.array_equal(ret, oracle_playout(o.board, o.rng, timer, MOVES, k, sm, acts)["ret"])
    assert call(n=-1) == -2
    assert call(q=0) == -2 and call(d=0) == -2
    assert call(n=2 ** 26 - 8, q=2) == -2
    assert call(board=None) == -1 and call(rng=None) == -1 and call(acts=None) == -1
    assert call(eff=None) == -1
    assert call(eff=None, trust=0) == 0
    assert call(timer=None, out_timer=ot) == -1
    assert call(ret=None, best_seq=best) == -1
    assert call(out_board=ob[1:]) == -2 and call(out_board=ob) == 0
    ret[:] = -7
    assert call(n=0, board=None, rng=None, acts=None, eff=None) == 0 and (ret == -7).all()
    assert L.emu_status() == 0
