"""The special-tile matrix (tests/special_matrix_cases.py) on the MI355X: every
recorded row of tests/golden/matrix_<shape>.npz, one batch per shape, through
tmg_trace, tmg_step and tmg_peek on every general kernel family, against the
outputs the reference itself produced (tests/golden/make_special_matrix.py).
The fixtures hold data only and nothing here reads the reference.  Boards are
compared as bytes and counts as integers; nothing here has a tolerance.

tmg_trace's combo / first clear frame is compared with the reference's own board
right after that stage: a kernel against the reference with no oracle in
between.  tests/test_special_matrix.py runs the same checks on the oracle and
on the host wave emulator, and the census of the fixtures."""
import numpy as np
import pytest
import torch

import lean_type_cases as lt
import special_matrix_cases as sm
from deep_rollouts import COVER_LIB
from oracle import oracle as orc
from test_gpu_trace import DEV, GpuDev, _p, _t

pytestmark = pytest.mark.gpu
SHAPES = sm.SHAPES
FIXED = [(10, 10, 4, 14), (20, 20, 6, 15)]         # kFixC3, kFixC5


@pytest.fixture(scope="module")
def dev():
    d = GpuDev()
    yield d
    d.close()


@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_trace_frames_equal_the_reference_gpu(dev, shape):
    sm.check_trace(dev, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_step_equals_the_reference_gpu(dev, shape):
    """Untrusted, from the recorded RNG words: the reference's recorded move; and orc.move of the same rows."""
    sm.check_step(dev, shape)
    d = sm.load_matrix(shape)
    rows = sm.played_rows(d)
    board, rng, reward, n_new, n_act, flags = dev.step(shape, d["board"][rows], d["rng_in"][rows], d["action"][rows])
    for j, i in enumerate(rows):
        out, words, res, err = orc.move(d["board"][i], d["rng_in"][i], d["action"][i], shape[2], shape[3])
        assert err == 0 and np.array_equal(board[j], out) and np.array_equal(rng[j].view(np.uint64), words), i
        assert (reward[j], n_new[j], n_act[j]) == (res[0], res[2], res[3]), i
        assert flags[j] & 0x86 == 2 * res[1] + 4 * res[4], i
    dev.status_clear(shape)


@pytest.mark.parametrize("shape", FIXED, ids=sm.shape_id)
def test_peek_action_column_equals_the_reference_gpu(dev, shape):
    """tmg_peek, untrusted: the column of the row's action holds the recorded
    results (the lookahead kernels share the move call, so one entry point
    stands for them); board and RNG words are only read.  Every row on 10x10.
    On 20x20 a row costs 760 moves, so the seeded rows and the crafted cookie
    rows play: every pair x orientation x position cell and every chain cell
    has a seeded row, the ones that chain and spill."""
    d = sm.load_matrix(shape)
    rows = sm.played_rows(d)
    if shape == (20, 20, 6, 15):
        rows = np.union1d(sm.seeded_rows(shape, d), rows[d["kind"][rows] == sm.ROW_COOKIE])
        assert 500 < len(rows) < 600
    ctx = dev.ctx(shape)
    n, A = len(rows), orc.num_actions(*shape[:2])
    b, g = _t(d["board"][rows]), _t(d["rng_in"][rows])
    out = torch.full((3, n, A), -7, dtype=torch.int32, device=DEV)
    fl = torch.full((n, A), 0x55, dtype=torch.uint8, device=DEV)
    ctx.status(clear=True)
    ctx.peek(n, _p(b), _p(g), None, 0, _p(out[0]), _p(out[1]), _p(out[2]), _p(fl), None, None,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    col = torch.from_numpy(d["action"][rows].astype(np.int64)).to(DEV)
    got = out[:, torch.arange(n, device=DEV), col].cpu().numpy()
    gfl = fl[torch.arange(n, device=DEV), col].cpu().numpy()
    res = d["res"][rows]
    sm.assert_rows_equal(shape, d, rows, got[0], res[:, 0], "peek reward")
    sm.assert_rows_equal(shape, d, rows, got[1], res[:, 2], "peek n_new")
    sm.assert_rows_equal(shape, d, rows, got[2], res[:, 3], "peek n_act")
    sm.assert_rows_equal(shape, d, rows, gfl, sm.want_flags(res), "peek flags")
    assert np.array_equal(b.cpu().numpy(), d["board"][rows]) and np.array_equal(g.cpu().numpy().view(np.uint64), d["rng_in"][rows])
    assert ctx.status(clear=True) == 0


def test_spilled_rows_are_compared_all_the_same_gpu(dev, record_property):
    """The seeded 20x20 rows alone: rows whose cascade outgrows the LDS lists go
    through the spill tier and equal the reference like the others.  The host
    wave emulator, which runs the same kernels on the same list sizes, spills on
    these rows (tests/test_special_matrix.py asserts it), so the device must."""
    shape = (20, 20, 6, 15)
    d = sm.load_matrix(shape)
    rows = sm.seeded_rows(shape, d)
    assert len(rows) > 400
    s0 = dev.spills(shape)
    board, rng, reward, _, n_act, _ = dev.step(shape, d["board"][rows], d["rng_in"][rows], d["action"][rows])
    spilled = dev.spills(shape) - s0
    sm.assert_rows_equal(shape, d, rows, board, d["out"][rows], "step board, seeded rows")
    sm.assert_rows_equal(shape, d, rows, rng, d["rng_out"][rows], "step rng words, seeded rows")
    sm.assert_rows_equal(shape, d, rows, reward, d["res"][rows, 0], "step reward, seeded rows")
    sm.assert_rows_equal(shape, d, rows, n_act, d["res"][rows, 3], "step n_act, seeded rows")
    record_property("spills_seeded_20x20", int(spilled))
    print(f"tmg_spills over the {len(rows)} seeded 20x20 rows: {spilled}")
    assert spilled > 0
    assert dev.status_clear(shape) == 0


# ---------------------------------------------------------------- coverage (the TMG_COVER build)
class CoverDev(GpuDev):
    def ctx(self, shape):
        from tile_match_gym_amd import _native
        if shape not in self.ctxs:
            R, C, k, smask = shape
            self.ctxs[shape] = _native.Context(0, R, C, k, smask, 1 << 20, lib_path=COVER_LIB)
        return self.ctxs[shape]


# the branch counters (CV_* of csrc/tmg_board.hip) the matrix must reach, where they apply: the closure and the
# decline of the scalar-bitboard step on boards of up to 128 cells whose rows fit a word; bomb_plan and the decline
# of the LDS step in the kernels without bitboards (a bomb needs two crossing lines, so three rows); a cookie on the
# lane-0 path wherever cookies are enabled
def applicable(shape):
    R, C, _, smask = shape
    bitboard = R * C <= 128 and C <= 63
    return (["combo"] + (["sb_closure", "sb_fallback"] if bitboard else ["lds_fallback"] + ["lds_bomb"] * (R >= 3))
            + (["serial_cookie"] if smask & 1 else []))


@pytest.mark.parametrize("shape", SHAPES, ids=sm.shape_id)
def test_matrix_reaches_the_special_tile_branches_gpu(shape):
    from tile_match_gym_amd import _native
    assert _native.build_info(COVER_LIB).get("variant") == "cover", "build() makes libtmg_cover.so"
    cdev = CoverDev()
    try:
        cdev.ctx(shape).cover(clear=True)
        sm.check_step(cdev, shape)                                  # the diagnostic build computes the same
        c = cdev.ctx(shape).cover()
        counts = {nm: int(c[i]) for i, nm in enumerate(_native.COVER_NAMES)}
        print(sm.shape_id(shape), {nm: counts[nm] for nm in ("combo", "sb_closure", "sb_fallback", "serial_cookie", "lds_bomb",
                                                             "lds_fallback", "serial_act", "spill")})
        low = {nm: counts[nm] for nm in applicable(shape) if counts[nm] <= 0}
        assert not low, f"never taken: {low}"
    finally:
        cdev.close()


# ---------------------------------------------------------------- the lean step's type check (tests/lean_type_cases.py)
def _gpu_lean_step(shape, board, rng, timer, eff, actions, fused):
    from tile_match_gym_amd import _native
    R, C, k, smask = shape
    n = len(actions)
    ctx = _native.Context(0, R, C, k, smask, lt.MOVES)
    b, g, t, e, a = _t(board), _t(rng), _t(timer), _t(eff), _t(np.asarray(actions, np.int32))
    out = torch.full((3, n), -7, dtype=torch.int32, device=DEV)
    fl = torch.full((n,), 0x55, dtype=torch.uint8, device=DEV)
    term = torch.full((n, 4), 0x55, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.status(clear=True)
    if fused:
        plan = _native.Plan(ctx, n, _p(b), _p(g), _p(t), _p(out[0]), _p(out[1]), _p(out[2]), _p(fl), _p(e), [0, n], [stream])
        plan.config("none", terminated=_p(term))
        plan.step(_p(a), 0, 1, stream)
        plan.join(stream)
        torch.cuda.synchronize()
        plan.close()
    else:
        ctx.step(n, _p(b), _p(g), _p(t), _p(a), _p(out[0]), _p(out[1]), _p(out[2]), _p(fl), _p(e), 1, 0, stream)
        torch.cuda.synchronize()
    o = out.cpu().numpy()
    got = dict(board=b.cpu().numpy(), rng=g.cpu().numpy().view(np.uint64), timer=t.cpu().numpy(), reward=o[0], n_new=o[1],
               n_act=o[2], flags=fl.cpu().numpy(), terminated=term.cpu().numpy(), status=ctx.status(clear=True))
    ctx.close()
    return got


@pytest.mark.parametrize("name", list(lt.CASES))
def test_lean_step_checks_the_type_plane_gpu(name):
    lt.check(_gpu_lean_step, name)
