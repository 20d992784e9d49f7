"""The kernels against the reference at the shape limits (tests/edge_cases.py):
the recordings of tests/golden/edge/, never the oracle.  Trajectories through
TileMatchVecEnv with the mask trusted (the lean kernels for the no-specials
shapes) and untrusted at every step (the general instantiation of every
shape); the move, effective and generate records through the C ABI with the
checks of tests/test_gpu_parity.py.  Bit-exact everywhere (integer work)."""
import pytest

import edge_cases as ec
import test_gpu_parity as tgp
from golden_io import load_records, load_traj, replay_trajectory

pytestmark = pytest.mark.gpu

TRAJ = ec.traj_cases()
TRAJ_IDS = [n for n, _ in TRAJ]


class _UntrustedBackend(tgp._VecBackend):
    """The effective-action mask dropped before every step: each step scans its own."""

    def step(self, a, autoreset):
        self.env.invalidate_effective_cache()
        super().step(a, autoreset)


@pytest.mark.parametrize("name,shape", TRAJ, ids=TRAJ_IDS)
@pytest.mark.parametrize("autoreset", [False, True])
def test_edge_trajectory_gpu(name, shape, autoreset):
    """Whole reference trajectories (tile_match_env.py:84-124), RNG-exact, two resets in each."""
    d = load_traj(name, ec.SUB)
    assert (d["R"], d["C"], d["k"], d["smask"]) == shape
    b = tgp._VecBackend(d)
    assert replay_trajectory(d, b, autoreset) > 0
    assert b.env.status() == 0
    b.env.close()


@pytest.mark.parametrize("name,shape", TRAJ, ids=TRAJ_IDS)
def test_edge_trajectory_untrusted_gpu(name, shape):
    """The same with invalidate_effective_cache() before every step: the
    no-specials shapes then run their general instantiation too, and every
    autoreset is the deferred reset launch."""
    d = load_traj(name, ec.SUB)
    b = _UntrustedBackend(d)
    assert replay_trajectory(d, b, True) > 0
    assert b.env.status() == 0
    b.env.close()


@pytest.mark.parametrize("group", list(ec.GROUPS))
def test_edge_move_gpu(group):
    """Board.move (board.py:330-395) from arbitrary boards with specials,
    RNG-exact: every record (the reference raised in none)."""
    recs = load_records("move", f"fn_{group}", ec.SUB)
    assert len(recs) == ec.FN_PER_SHAPE * len(ec.fn_shapes(group))
    tgp.check_move_gpu(recs, len(recs) - 1)


@pytest.mark.parametrize("group", list(ec.GROUPS))
def test_edge_effective_gpu(group):
    recs = load_records("effective", f"fn_{group}", ec.SUB)
    assert len(recs) == ec.FN_PER_SHAPE * len(ec.fn_shapes(group))
    tgp.check_effective_gpu(recs)


@pytest.mark.parametrize("group", list(ec.GROUPS))
def test_edge_generate_gpu(group):
    recs = load_records("generate", f"fn_{group}", ec.SUB)
    assert len(recs) == 2 * len(ec.fn_shapes(group))
    tgp.check_generate_gpu(recs)
