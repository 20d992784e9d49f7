"""tmg_expand_count / tmg_expand on the host wave emulator (CPU): the count /
scan and gather kernels of csrc/tmg_expand.hip, then emu_step on the child
rows, against the oracle's children (tests/expand_cases.py oracle_expand: numpy
placement, OracleBatch.step on the copies).  Both store variants of the gather
run.  Everything is compared with np.array_equal; nothing here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import expand_cases
import peek_cases
from expand_cases import assert_expand_equal, oracle_expand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    return emu, emu.load()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000])
@pytest.mark.parametrize("shape", [(3, 5), (10, 10), (20, 20)], ids=["W1", "W3", "W12"])
def test_count_scan(emu_lib, shape, n):
    """Synthetic mask rows, no boards: random words with bits at and above A in
    the last word, random select words and none, timers on both sides of
    num_moves; 5 000 envs are more than one workgroup's tile."""
    emu, L = emu_lib
    R, C = shape
    A = 2 * R * C - R - C
    W = (A + 63) // 64
    assert W == {(3, 5): 1, (10, 10): 3, (20, 20): 12}[shape]
    moves = 9
    rs = np.random.default_rng(1000 * W + n)
    eff = rs.integers(0, 2 ** 64, (n, W), dtype=np.uint64)
    sel = rs.integers(0, 2 ** 64, (n, W), dtype=np.uint64)
    timer = rs.integers(0, 2 * moves, n).astype(np.int32)
    if n:
        assert A % 64 and (eff[:, -1] >> np.uint64(A % 64)).any(), "bits above A are part of the case"
    before = (eff.copy(), sel.copy(), timer.copy())
    for select in (None, sel):
        bits = expand_cases.unpack_mask(eff if select is None else eff & select, A)
        counts = bits.sum(axis=1) * (timer < moves)
        want = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        got = emu.expand_count(L, R, C, moves, timer, eff, select)
        assert np.array_equal(got, want)
    assert all(np.array_equal(x, y) for x, y in zip(before, (eff, sel, timer)))


@pytest.mark.parametrize("shape", expand_cases.EMULATED_SHAPES + expand_cases.EMULATED_LIMIT_SHAPES, ids=expand_cases.case_id)
def test_expand_vs_oracle(emu_lib, shape):
    """After a reset and after 7 uniform-random steps, with the envs' own RNG
    words and with words of other seeds; every env has at least two children."""
    from tile_match_gym_amd.seeding import batch_rng_words
    emu, L = emu_lib
    R, C, k, sm = shape
    n = 5
    other = batch_rng_words(range(7000, 7000 + n))
    for steps in (0, 7):
        o = peek_cases.rolled_batch(shape, range(500, 500 + n), steps=steps)
        before = tuple(getattr(o, f).copy() for f in expand_cases.STATE)
        for rng in (o.rng, other):
            want = oracle_expand(o.board, rng, o.timer, o.eff, None, k, sm, 30)
            assert np.diff(want["first_child"]).min() >= 2
            for pack in (1, 0):
                got = emu.expand(L, R, C, k, sm, 30, o.board, rng, o.timer, o.eff, pack=pack)
                assert_expand_equal(got, want, f"{shape} steps={steps} pack={pack}")
        assert all(np.array_equal(x, getattr(o, f)) for x, f in zip(before, expand_cases.STATE))
    assert L.emu_status() == 0


@pytest.mark.parametrize("pack", [1, 0])
def test_expand_select_horizon_and_m(emu_lib, pack):
    """3x5 with num_moves = 8: parents at timers 3, 7 and 8 (finished: no
    child), a random select that also names ineffective actions; then m below
    and above the total: a prefix, and tail rows that the step refuses."""
    emu, L = emu_lib
    shape = (3, 5, 2, 0)
    R, C, k, sm = shape
    n, moves = 6, 8
    o = peek_cases.rolled_batch(shape, range(500, 500 + n), steps=3, num_moves=moves)
    o.timer[:] = [3, 7, 8, 3, 8, 7]
    sel = np.random.default_rng(5).random((n, o.A)) < 0.6
    want = oracle_expand(o.board, o.rng, o.timer, o.eff, sel, k, sm, moves)
    total = int(want["first_child"][n])
    assert total >= 8 and (sel & ~expand_cases.unpack_mask(o.eff, o.A)).any()
    counts = np.diff(want["first_child"])
    assert counts[2] == 0 and counts[4] == 0
    got = emu.expand(L, R, C, k, sm, moves, o.board, o.rng, o.timer, o.eff, expand_cases.pack_mask(sel), pack=pack)
    assert_expand_equal(got, want, "select")
    last = want["parent"] % 3 != 0                              # children of the timer-7 parents (envs 1 and 5)
    assert last.any() and (got["flags"][last] & expand_cases.FLAG_DONE).all() and not got["eff"][last].any()
    assert not (got["flags"][~last] & expand_cases.FLAG_DONE).any()
    assert L.emu_status() == 0
    fields = [f for f in expand_cases.FIELDS if f != "first_child"]
    # a prefix: the rows from m on are not part of the call
    got = emu.expand(L, R, C, k, sm, moves, o.board, o.rng, o.timer, o.eff, expand_cases.pack_mask(sel), m=total - 3,
                     pack=pack)
    assert_expand_equal(got, {f: want[f][:total - 3] for f in fields}, "prefix", fields)
    # past the total: rows the step treats as steps after done
    got = emu.expand(L, R, C, k, sm, moves, o.board, o.rng, o.timer, o.eff, expand_cases.pack_mask(sel), m=total + 5,
                     pack=pack)
    assert_expand_equal({f: got[f][:total] for f in fields}, {f: want[f] for f in fields}, "head", fields)
    assert (got["flags"][total:] == expand_cases.FLAG_ERROR).all() and (got["parent"][total:] == -1).all()
    assert (got["timer"][total:] == moves).all() and (got["action"][total:] == 0).all()
    assert not got["eff"][total:].any() and not got["reward"][total:].any()
    assert (got["board"][total:] == -7).all() and (got["rng"][total:] == 0xA5A5A5A5A5A5A5A5).all()
    assert L.emu_status_clear() == 4                            # TMG_STATUS_CALLER


def test_expand_refusals(emu_lib):
    emu, L = emu_lib
    shape = (3, 5, 2, 0)
    o = peek_cases.rolled_batch(shape, range(500, 502), steps=0)
    with pytest.raises(ValueError):
        emu.expand(L, 3, 5, 2, 0, 30, o.board, o.rng, o.timer, o.eff, m=-1)
    got = emu.expand(L, 3, 5, 2, 0, 30, o.board, o.rng, o.timer, o.eff, m=0)
    assert got["board"].shape[0] == 0
