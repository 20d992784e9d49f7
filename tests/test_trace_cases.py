"""The reference walk of the tmg_trace tests, pinned on the CPU (no emulator, no
device): tests/trace_cases.py oracle_trace composes a move from the oracle's
primitives, stage by stage; here its last board, RNG words and results must
equal oracle.move's on every state the other trace tests use, the stage
eliminations must add up to the reward, and the cases together must reach every
stage kind.  This file passes without tmg_trace: it checks the expected values,
not the kernels."""
import numpy as np
import pytest

import trace_cases as tc
from oracle import oracle as orc

_SEEN = set()


def _check_state(name, board, rng, acts, k, smask):
    n = board.shape[0]
    A = orc.num_actions(*board.shape[2:])
    moves = 0
    for q in range(acts.shape[0]):
        for i in range(n):
            a = int(acts[q, i])
            if not 0 <= a < A:
                continue
            stages, b1, g1, res = tc.oracle_trace(board[i], rng[i], a, k, smask)
            wb, wg, wres, err = orc.move(board[i], rng[i], a, k, smask)
            assert err == 0
            what = f"{name} q={q} env={i} a={a}"
            assert np.array_equal(b1, wb), f"{what}: board after the move"
            assert np.array_equal(g1, wg), f"{what}: RNG words after the move"
            assert tuple(int(x) for x in res) == tuple(int(x) for x in wres), f"{what}: results {res} vs {wres}"
            assert sum(s.elim for s in stages) + res[2] == res[0], f"{what}: stage eliminations do not add up"
            if stages:
                moves += 1
                assert np.array_equal(stages[-1].board, wb) and np.array_equal(stages[-1].rng, wg), what
                assert stages[0].kind == tc.SWAP and all(s.elim == 0 for s in stages if s.kind not in (tc.COMBO, tc.CLEAR))
                first_fall = next(s for s in stages if s.kind == tc.FALL)
                assert np.array_equal(first_fall.rng, rng[i]), f"{what}: a draw before the afterstate"
            _SEEN.update(s.kind for s in stages)
    return moves


@pytest.mark.parametrize("case", list(tc.all_cases()), ids=lambda c: c[0])
def test_walk_equals_oracle_move(case):
    assert _check_state(*case) > 0, "the case traces no effective move"


def test_shuffling_shapes_shuffle():
    """Every traced first-row move of a shuffling shape shuffles."""
    for s in tc.SHUFFLING:
        _, _, _, want = tc.field_case(s)
        assert (want["flags"][0] & tc.FLAG_SHUFFLED).all(), s
        assert (want["kind"][0] == tc.SHUFFLE).any(axis=1).all(), s


def test_combo_grid_moves_are_combos():
    from adversarial import adversarial_boards
    shape = (10, 10, 4, 14)
    b, words, acts = tc.adversarial_case(shape, "combo_grid", 4)
    want = tc.expected(b, words, acts[:1], shape[2], shape[3], tc.ALL_STAGES, tc.WHOLE, 0)
    assert (want["flags"][0] & tc.FLAG_COMBO).all() and (want["kind"][0, :, 1] == tc.COMBO).all()
    assert adversarial_boards is not None


def test_whole_moves_fit_and_cases_reach_every_kind():
    """max_frames = WHOLE holds every whole-move case; the parametrised test
    above has seen every stage kind (it runs first in this file)."""
    for s in tc.FIELD_SHAPES:
        assert tc.field_case(s)[3]["n_frames"].max() <= tc.WHOLE, s
    kinds = set(_SEEN)
    for s in tc.FIELD_SHAPES + [(10, 10, 4, 14)]:
        kinds.update(np.unique(tc.field_case(s)[3]["kind"]).tolist())
    b, words, acts = tc.adversarial_case((10, 10, 4, 14), "combo_grid", 4)
    kinds.update(np.unique(tc.expected(b, words, acts, 4, 14, tc.ALL_STAGES, tc.WHOLE, 0)["kind"]).tolist())
    assert kinds >= set(tc.KINDS), f"stage kinds never reached: {set(tc.KINDS) - kinds}"


def test_prefix_rule_of_stopped_rows():
    """expected(stop = 1) on the afterstate form: one FALL frame, the input
    words, the deterministic reward; a row whose move has no such frame left is
    the stop = 0 row."""
    shape = (10, 10, 4, 14)
    board, rng, acts, whole = tc.field_case(shape)
    want = tc.expected(board, rng, acts, shape[2], shape[3], 1 << tc.FALL, 1, 1)
    eff = whole["n_frames"] > 0
    assert eff.any() and not eff.all()
    assert (want["n_frames"][eff] == 1).all() and (want["flags"][eff] & tc.FLAG_STOPPED).all()
    assert np.array_equal(want["out_rng"], np.broadcast_to(rng, want["out_rng"].shape))
    assert (want["reward"] <= whole["reward"]).all() and (want["reward"][eff] >= 3).all()
    assert not want["n_frames"][~eff].any() and not (want["flags"][~eff] & tc.FLAG_STOPPED).any()
