"""The stand-alone sanitizer program of tmg_trace on the host:
tools/wave_emu/trace_asan (the trace kernels on the wave emulator, n in {1, 3}
envs, seqs in {1, 2} action rows, max_frames in {1, 4}, with and without
`frames`, every array a heap block of exactly its rows, each row's sums, RNG
words and, where the move fits, last frame compared with an emulated step on a
one-env copy).  It has its own main and is built with
-fsanitize=address,undefined by its make target; it runs as a plain program in
an unchanged environment, as tests/test_playout_host.py runs its program:
nothing is loaded into Python and nothing is preloaded.  A report makes the
program abort; a wrong row makes it exit 1.

ASan's notice about the emulator's fiber stacks ("ignoring requested
__asan_handle_no_return") on stderr is expected and is no failure."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "wave_emu")


def test_trace_sanitizer_program():
    subprocess.run(["make", "-C", EMU_DIR, "trace_asan"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "trace_asan")], capture_output=True, text=True, cwd=EMU_DIR)
    tail = (r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    lines = r.stdout.strip().splitlines()
    m = re.fullmatch(r"trace_asan ok: (\d+) rows checked", lines[-1]) if lines else None
    assert m and int(m.group(1)) > 0, tail
