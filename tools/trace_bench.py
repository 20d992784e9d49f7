"""Trace throughput: two measurements of tmg_trace, with HIP events, after warm-up.

1. afterstates   The afterstate of every action (trace of kind "fall", one
                 frame, stop: TileMatchVecEnv.afterstates' call, Q = A action
                 rows) against playout(depth 1, final=True) on the same (Q = A,
                 N) rows: the closest thing the library had (the board after the
                 whole move).  The afterstate does a strict subset of that
                 playout's work (no refill, no further iteration, no
                 ensure-playable, no mask scan), but always on the general
                 kernels, where playout runs the lean ones on c2.  The two
                 alternate within one process and each is timed in two separate
                 runs, so the spread of the baseline's two runs is the noise the
                 comparison is read against.  Shapes c2 and c3, N in {64, 4096},
                 envs after a reset and 10 steps of the effective-action policy.
2. full_trace    The default stages ("clear", "fall", "refill"), max_frames =
                 32, one effective action per env (the in-kernel policy's draw),
                 at c2's 65 536 envs: bytes written (sum over rows of
                 min(n_frames, 32) * 2RC frame bytes, plus kind, frame_elim, the
                 five (Q, N) arrays and out_rng) over the time, against the HBM
                 peak given with --hbm-peak (bytes per second).  A reported
                 number, not a bar.

Prints one JSON line per case with [median, min, max] in ms per run, and a final
JSON line with all of them.

    python tools/trace_bench.py [--shapes c2,c3] [--envs 64,4096] [--full-envs 65536] [--repeats 20] [--warmup 3]
                                [--hbm-peak 8e12] [--lib PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tile-match-gym_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SHAPES = {
    # name: (R, C, k, colourless specials, colour specials)
    "c2": (10, 10, 4, [], []),
    "c3": (10, 10, 4, [], ["vertical_laser", "horizontal_laser", "bomb"]),
}
KEY = 12345
MOVES = 30
POLICY_STEPS = 10
BUDGET_MS = 4000            # per variant and run: fewer repeats (never below 5) once a call is slower than budget / repeats


def make_env(name, n, args, torch):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, cl, co = SHAPES[name]
    env = TileMatchVecEnv(n, R, C, k, MOVES, cl, co, seed=0, device="cuda:0", groups=1, lib_path=args.lib)
    env.reset()
    for t in range(POLICY_STEPS):
        env.step_effective(t, key=KEY)
    env.join()
    torch.cuda.synchronize()
    return env


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def afterstates_case(name, n, args, torch, info):
    env = make_env(name, n, args, torch)
    A = env.num_actions
    acts = torch.arange(A, dtype=torch.int32, device=env.device).unsqueeze(1).expand(A, n).contiguous()
    acts3 = acts.unsqueeze(2).contiguous()                        # playout's (Q, N, D = 1)
    variants = {"afterstates": lambda: env.trace(acts, stages=("fall",), max_frames=1, stop=True),
                "playout_final": lambda: env.playout(acts3, outputs=("ret",), final=True)}
    # the same rows: a row has an afterstate exactly where the playout's ply was an effective move
    tr = env.trace(acts, stages=("fall",), max_frames=1, stop=True)
    po = env.playout(acts3, outputs=("ret", "flags"))
    torch.cuda.synchronize()
    eff = tr["n_frames"] > 0
    assert bool((tr["reward"] <= po["ret"]).all()) and bool(((po["ret"] > 0) == eff).all())
    assert not int((tr["flags"] & 0x80).any()) and not int((po["flags"] & 0x80).any())
    del tr, po
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    runs = {f"{v}_run{j}": [] for v in variants for j in (1, 2)}
    for j in (1, 2):
        repeats = args.repeats
        for r in range(args.repeats):
            if r >= repeats:
                break
            first = []
            for v, fn in variants.items():                          # alternating
                ms = timed(fn, torch)
                runs[f"{v}_run{j}"].append(ms)
                first.append(ms)
            if r == 0:
                repeats = max(5, min(args.repeats, int(BUDGET_MS / max(first))))
    assert env.status() == 0, "device status"
    res = {"case": "afterstates", "shape": name, "envs": n, "rows": A * n, "effective_rows": int(eff.sum()),
           "lib_variant": info["variant"], "src": info["src"][:16]}
    res.update({k: stats(v) for k, v in runs.items()})
    a = min(res["afterstates_run1"][0], res["afterstates_run2"][0])
    a_hi = max(res["afterstates_run1"][0], res["afterstates_run2"][0])
    b_lo = min(res["playout_final_run1"][0], res["playout_final_run2"][0])
    b_hi = max(res["playout_final_run1"][0], res["playout_final_run2"][0])
    res["baseline_spread_ms"] = round(b_hi - b_lo, 4)
    res["afterstates_over_playout"] = round((a + a_hi) / (b_lo + b_hi), 4)
    res["not_slower_beyond_spread"] = bool(a_hi <= b_hi + (b_hi - b_lo))
    env.close()
    print(json.dumps(res), flush=True)
    return res


def full_trace_case(name, n, args, torch, info):
    env = make_env(name, n, args, torch)
    R, C, F = env.num_rows, env.num_cols, 32
    env.step_effective(POLICY_STEPS, key=KEY)                     # the policy's draw: an effective action per env ...
    env.join()
    acts = env.actions.clone()
    env.close()
    env = make_env(name, n, args, torch)                          # ... of the state before that step
    fn = lambda: env.trace(acts, max_frames=F)                    # noqa: E731
    out = fn()
    torch.cuda.synchronize()
    nf = out["n_frames"].to(torch.int64)
    assert bool((nf >= 3).all()) and not int((out["flags"] & 0x80).any())
    frame_bytes = int(nf.clamp(max=F).sum()) * 2 * R * C
    small = n * (F * (1 + 4) + 4 * 4 + 1 + 40)                    # kind, frame_elim, four int32, flags, out_rng
    cut = int((nf > F).sum())
    del out
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    runs = {}
    for j in (1, 2):
        runs[f"run{j}"] = [timed(fn, torch) for _ in range(args.repeats)]
    assert env.status() == 0, "device status"
    res = {"case": "full_trace", "shape": name, "envs": n, "max_frames": F, "frames_written": frame_bytes // (2 * R * C),
           "rows_cut": cut, "bytes_written": frame_bytes + small, "lib_variant": info["variant"], "src": info["src"][:16]}
    res.update({k: stats(v) for k, v in runs.items()})
    med = min(res["run1"][0], res["run2"][0])
    res["write_gb_per_s"] = round((frame_bytes + small) / (med * 1e-3) / 1e9, 2)
    res["fraction_of_hbm_peak"] = round((frame_bytes + small) / (med * 1e-3) / args.hbm_peak, 5)
    env.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--envs", default="64,4096")
    ap.add_argument("--full-envs", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-peak", type=float, default=8e12, help="HBM peak bandwidth in bytes per second")
    ap.add_argument("--lib", default=None, help="another build of libtmg.so (an A/B variant)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trace_bench needs a HIP device: there is no CPU fallback")
    from tile_match_gym_amd import _native
    info = _native.build_info(args.lib)
    out = []
    for name in args.shapes.split(","):
        for n in (int(x) for x in args.envs.split(",")):
            out.append(afterstates_case(name, n, args, torch, info))
    if args.full_envs > 0:
        out.append(full_trace_case("c2", args.full_envs, args, torch, info))
    print(json.dumps({"trace_bench": out}))


if __name__ == "__main__":
    main()
