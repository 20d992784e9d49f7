"""The stand-alone sanitizer programs of tools/wave_emu on the host: expand_asan
(tmg_expand's count / scan and gather kernels) and extent_asan (every other
entry point at ragged batch sizes, exactly sized heap blocks of n rows, so
AddressSanitizer sees the loads past a row as well as the stores; the device
test tests/test_gpu_extent.py sees stores only).  Each has its own main and is
built with -fsanitize=address,undefined by its make target; it runs as a plain
program in an unchanged environment, nothing is loaded into Python and nothing
is preloaded.  A report makes the program abort; a wrong row makes it exit 1.

ASan's notice about the emulator's fiber stacks ("ignoring requested
__asan_handle_no_return") on stderr is expected and is no failure."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")

# program, its last line
PROGRAMS = [("expand_asan", r"expand_asan ok: (\d+) child rows checked"), ("extent_asan", r"extent_asan ok: (\d+) cases")]


@pytest.mark.parametrize("prog,ok_line", PROGRAMS, ids=[p for p, _ in PROGRAMS])
def test_sanitizer_program(prog, ok_line):
    subprocess.run(["make", "-C", EMU_DIR, prog], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, prog)], capture_output=True, text=True, cwd=EMU_DIR)
    tail = (r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    lines = r.stdout.strip().splitlines()
    m = re.fullmatch(ok_line, lines[-1]) if lines else None
    assert m and int(m.group(1)) > 0, tail
