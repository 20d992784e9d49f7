"""The `plain` field of the step route (csrc/tmg_dispatch.h: plain_step,
StepRoute::plain): which calls get plain_step_kernel, the plain form of
step_kernel<128, false, 2, false, kFixC2>.  emu_route reports the rule's
choice without launching anything; the expected values are written out here.

plain is 1 exactly for c2-shape (10x10 k4, no specials), trusted, given-action
calls with no fused output and n <= kPlainMaxEnvs that the wave-per-board
ladder takes.  The instantiation tuple is the same either way."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")

C2 = (10, 10, 4, 0)
FIX_C2 = 10 << 24 | 10 << 16 | 4 << 8
C2_KERNEL = (128, 0, 2, 0, FIX_C2)
PLAIN_MAX = 1 << 23                     # kPlainMaxEnvs
LANE_MIN = 131072                       # kLaneMinEnvs
FUSED = ("onehot", "terminated", "action_mask", "moves_left", "final_board", "board32")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.run(["make", "-C", EMU_DIR, "libwave_emu.so"], check=True, stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU_DIR)
    import emu
    return emu, emu.load()


def _inst(st):
    return tuple(st[f] for f in ("MAXN", "GEN", "NB", "CODD", "FIX"))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 9, 65, 21845, 65536, LANE_MIN, PLAIN_MAX])
def test_plain_for_c2_given_actions(emu_lib, n, mode):
    emu, L = emu_lib
    st, _ = emu.route(L, *C2, mode=mode, n=n)
    assert st["plain"] == 1 and _inst(st) == C2_KERNEL and st["lean"] == 1 and st["lane"] == 0, st
    assert st["kernel_autoreset"] == (0, 1, 3)[mode] and st["deferred"] == 0, st


def test_not_plain_past_the_32_bit_offsets(emu_lib):
    emu, L = emu_lib
    st, _ = emu.route(L, *C2, n=PLAIN_MAX + 1)
    assert st["plain"] == 0 and _inst(st) == C2_KERNEL, st
    # the largest byte offsets of the largest plain launch: board, RNG state, mask row, int32 outputs
    assert all(PLAIN_MAX * row < 1 << 31 for row in (2 * 100, 5 * 8, 3 * 8, 4))


def test_not_plain_with_the_policy(emu_lib):
    emu, L = emu_lib
    st, _ = emu.route(L, *C2, policy=True)
    assert st["plain"] == 0 and _inst(st) == C2_KERNEL, st


@pytest.mark.parametrize("fused", FUSED)
def test_not_plain_with_a_fused_output(emu_lib, fused):
    emu, L = emu_lib
    for mode in (0, 1, 2):
        st, _ = emu.route(L, *C2, mode=mode, fused=(fused,))
        assert st["plain"] == 0 and _inst(st) == C2_KERNEL, (fused, mode, st)


def test_not_plain_untrusted(emu_lib):
    emu, L = emu_lib
    st, _ = emu.route(L, *C2, trust_eff=0)
    assert st["plain"] == 0 and st["lean"] == 0 and st["GEN"] == 1, st


@pytest.mark.parametrize("shape", [(10, 10, 5, 0), (10, 10, 4, 14), (10, 10, 3, 0), (10, 12, 4, 0), (8, 8, 4, 0),
                                   (20, 20, 6, 0)])
def test_not_plain_for_other_shapes(emu_lib, shape):
    emu, L = emu_lib
    st, _ = emu.route(L, *shape)
    assert st["plain"] == 0 and st["FIX"] != FIX_C2, (shape, st)


def test_the_lane_kernel_comes_first(emu_lib):
    """Where the library has the lane kernel, a given-action launch of kLaneMinEnvs envs goes there: no ladder, not plain."""
    emu, L = emu_lib
    st, _ = emu.route(L, *C2, n=LANE_MIN, have_lane=True)
    assert st["lane"] == 1 and st["plain"] == 0, st
    st, _ = emu.route(L, *C2, n=LANE_MIN - 1, have_lane=True)
    assert st["lane"] == 0 and st["plain"] == 1, st
