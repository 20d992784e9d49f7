#!/usr/bin/env python3
"""Golden vectors at the shape limits (tests/edge_cases.py), recorded from the
reference itself like make_goldens.py's, whose stand-ins, gen_trajectory,
gen_function_goldens and pack_records it reuses.  Runs by hand and ONLY where
the reference tree is (make_goldens.REF_SRC), like that script.  Writes data-only .npz fixtures to
tests/golden/edge/: traj_<group>_<shape>.npz and fn_<group>_<kind>.npz.

Usage:
    python tests/golden/make_edge_goldens.py            # (re)write tests/golden/edge/
    python tests/golden/make_edge_goldens.py --check    # record into a temporary folder and
                                                        # compare every array with the committed one
    python tests/golden/make_edge_goldens.py --probe-8x64   # the oracle's reset of 8x64 under a 60 s cap

Every recording runs under a time limit (SIGALRM); a shape that times out is
reported and dropped, never retried.  About 80 s in all."""
from __future__ import annotations

import argparse
import os
import shutil
import signal
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (HERE, TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_goldens as mg          # noqa: E402
import edge_cases as ec            # noqa: E402

EDGE_DIR = os.path.join(HERE, ec.SUB)
TRAJ_LIMIT = 120       # s per trajectory (measured: at most 11 s)
FN_SEED = {"a": 778, "b": 779}

# Dropped, with the reason (none of the listed shapes timed out when this was last run):
#   8x64 k5 / k6, 1x4 k3, 4x1 k3: generate_board did not finish in 240 s; never listed.


def record(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    mg.OUT_DIR = out_dir
    mg.install_stubs()
    import tile_match_gym  # noqa: F401
    dropped = []
    t0 = time.time()
    for group, shapes in ec.GROUPS.items():
        seeds, steps = ec.TRAJ[group]
        for (R, C, k, sm) in shapes:
            name = ec.traj_name(group, (R, C, k, sm))
            t1 = time.time()
            try:
                signal.alarm(TRAJ_LIMIT)
                mg.gen_trajectory(name, R, C, k, ec.NUM_MOVES, sm, list(seeds), steps, 4242 + R * 31 + C, p_eff=ec.P_EFF)
                signal.alarm(0)
            except mg.Timeout:
                signal.alarm(0)
                dropped.append(name)
                print(f"traj_{name}: DROPPED after {TRAJ_LIMIT} s")
                continue
            print(f"traj_{name}: {time.time() - t1:.1f}s")
    for group in ec.GROUPS:
        t1 = time.time()
        mg.SHAPES = ec.fn_shapes(group)
        # its two unbounded calls (generate_board, move) run under its own 20 s alarms; a record
        # that times out is left out
        recs = mg.gen_function_goldens(ec.FN_PER_SHAPE, seed=FN_SEED[group])
        for key, rs in recs.items():
            mg.pack_records(rs, os.path.join(out_dir, f"fn_{group}_{key}.npz"))
            print(f"fn_{group}_{key}: {len(rs)} records")
        print(f"fn_{group}: {time.time() - t1:.1f}s")
    print(f"total {time.time() - t0:.1f}s, dropped: {dropped or 'none'}")
    return dropped


def check():
    tmp = tempfile.mkdtemp(prefix="tmg_edge_")
    try:
        record(tmp)
        names = sorted(f for f in os.listdir(EDGE_DIR) if f.endswith(".npz"))
        assert names == sorted(f for f in os.listdir(tmp) if f.endswith(".npz")), "the file lists differ"
        for f in names:
            a, b = np.load(os.path.join(EDGE_DIR, f)), np.load(os.path.join(tmp, f))
            assert a.files == b.files, f
            for key in a.files:
                assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (f, key)
        print(f"{len(names)} files: every array identical")
    finally:
        shutil.rmtree(tmp)


def probe_8x64(cap=60):
    """OracleBatch.reset() of one 8x64 board, k 5 and k 6, each in a child process under `cap` seconds."""
    import subprocess
    for k, sm in ((5, 0), (6, 15)):
        code = ("import sys; sys.path[:0] = %r\n"
                "from oracle import oracle as orc\n"
                "from tile_match_gym_amd.seeding import batch_rng_words\n"
                "orc.OracleBatch(8, 64, %d, %d, 12, batch_rng_words([100])).reset()\n"
                % ([os.path.dirname(TESTS), os.path.join(os.path.dirname(TESTS), "tile-match-gym_amd")], k, sm))
        t = time.time()
        try:
            subprocess.run([sys.executable, "-c", code], check=True, timeout=cap)
            print(f"8x64 k{k}: oracle reset finished in {time.time() - t:.1f}s")
        except subprocess.TimeoutExpired:
            print(f"8x64 k{k}: oracle reset did not finish in {cap} s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--probe-8x64", action="store_true")
    args = ap.parse_args()
    if args.probe_8x64:
        probe_8x64()
    elif args.check:
        check()
    else:
        record(EDGE_DIR)
