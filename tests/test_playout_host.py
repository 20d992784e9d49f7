"""The stand-alone sanitizer program of tmg_playout on the host:
tools/wave_emu/playout_asan (the playout kernels and their reduce kernel on the
wave emulator, n in {1, 3} envs and Q in {1, 3} sequences of 3 actions, with
and without the final-state outputs, every array a heap block of exactly its
rows, each row compared with a host loop of emulated steps on a one-env copy).
It has its own main and is built with -fsanitize=address,undefined by its make
target; it runs as a plain program in an unchanged environment, as
tests/test_extent_host.py runs its programs: nothing is loaded into Python and
nothing is preloaded.  A report makes the program abort; a wrong row makes it
exit 1.

ASan's notice about the emulator's fiber stacks ("ignoring requested
__asan_handle_no_return") on stderr is expected and is no failure."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


def test_playout_sanitizer_program():
    subprocess.run(["make", "-C", EMU_DIR, "playout_asan"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "playout_asan")], capture_output=True, text=True, cwd=EMU_DIR)
    tail = (r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    lines = r.stdout.strip().splitlines()
    m = re.fullmatch(r"playout_asan ok: (\d+) rows checked", lines[-1]) if lines else None
    assert m and int(m.group(1)) > 0, tail
