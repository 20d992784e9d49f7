"""Playout throughput: tmg_playout against the way the same sequences are played
with the stepping API alone.

For each shape (c2: 10x10 k4 without specials; c3: 10x10 k4 with v/h-laser +
bomb; c5: 20x20 k6 with all specials), n envs after a reset and 10 steps of the
effective-action policy, Q sequences of D actions per env and two kinds of
sequences (uniform: every action uniform over [0, A), so most plies are
ineffective; masked: every action drawn from the effective mask of the board
the ply before left, recorded from a run of the stepping side with the
in-kernel policy, so every ply is a move), it times with HIP events, after
warm-up:

  (a) playout        tmg_playout writing the (Q, N) return table;
  (a') playout_final the same with the final-state rows (final=True: the Q * N
                     boards, RNG words, timers and masks, and the env over them);
  (b) step_copies    the stepping API only: board / rng / timer / eff tiled Q
                     times with torch into a second batch of Q * N rows, D
                     step_raw calls with autoreset off, the rewards summed (the
                     second batch's buffers and the per-ply action rows are
                     laid out once, outside the timing).

All play the same sequences from the same RNG words, so the return tables and
the final states are compared exactly before anything is timed.  The three are
measured in turn within each repeat, so drift of the machine falls on all
alike.  A call plays Q * N * D plies.  Prints one JSON line per (shape, n, Q,
D, kind) with each variant's [median, min, max] in ms, and a final JSON line
with all of them.

    python tools/playout_bench.py [--shapes c2,c3,c5] [--envs 64,4096] [--seqs 16,256] [--depths 4,16]
                                  [--kinds uniform,masked] [--repeats 20] [--warmup 3] [--lib PATH]
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
    "c5": (20, 20, 6, ["cookie"], ["vertical_laser", "horizontal_laser", "bomb"]),
}
KEY = 12345
MOVES = 30
POLICY_STEPS = 10
BUDGET_MS = 4000            # per variant and case: fewer repeats (never below 5) once a call is slower than budget / repeats


class StepCopies:
    """(b): a second batch of Q * N rows, row q * N + i a copy of env i."""

    def __init__(self, env, Q, torch):
        from tile_match_gym_amd.vec_env import TileMatchVecEnv
        self.env, self.Q, self.torch = env, Q, torch
        self.sim = TileMatchVecEnv(Q * env.num_envs, env.num_rows, env.num_cols, env.num_colours, env.num_moves,
                                   env.colourless_specials, env.colour_specials, seed=0, device=env.device,
                                   autoreset=False, groups=1)

    def tile(self):
        env, sim, Q = self.env, self.sim, self.Q
        sim.board.copy_(env.board.repeat(Q, 1, 1, 1))
        sim.rng.copy_(env.rng.repeat(Q, 1))
        sim.timer.copy_(env.timer.repeat(Q))
        sim.eff.copy_(env.eff.repeat(Q, 1))
        sim._eff_valid = True

    def __call__(self, rows):
        """rows: (D, Q * N) int32, the actions of ply d in row d.  The summed rewards (Q * N,)."""
        sim = self.sim
        self.tile()
        ret = self.torch.zeros(sim.num_envs, dtype=self.torch.int32, device=sim.device)
        for d in range(rows.shape[0]):
            sim.step_raw(rows[d])
            ret += sim.reward
        return ret

    def record_masked(self, D):
        """(D, Q * N) int32: D steps of the in-kernel effective-action policy on the tiled batch, its draws kept."""
        sim = self.sim
        self.tile()
        rows = []
        for d in range(D):
            sim.step_effective(d, key=KEY)
            rows.append(sim.actions.clone())
        return self.torch.stack(rows).contiguous()

    def close(self):
        self.sim.close()


def run_case(env, copies, name, Q, D, kind, args, torch, info):
    n, A = env.num_envs, env.num_actions
    if kind == "uniform":
        g = torch.Generator(device=env.device)
        g.manual_seed(Q * 1000 + D)
        rows = torch.randint(0, A, (D, Q * n), dtype=torch.int32, device=env.device, generator=g)
    else:
        rows = copies.record_masked(D)
    acts = rows.t().contiguous().view(Q, n, D)                   # tmg_playout's layout
    variants = {"playout": lambda: env.playout(acts, outputs=("ret",)),
                "playout_final": lambda: env.playout(acts, outputs=("ret",), final=True),
                "step_copies": lambda: copies(rows)}
    # the same plies exactly, before anything is timed
    out = env.playout(acts, outputs=("ret", "plies", "flags"), final=True)
    ret = copies(rows)
    torch.cuda.synchronize()
    assert torch.equal(out["ret"].view(-1), ret), "playout and step-on-copies disagree"
    assert int(out["plies"].sum()) == Q * n * D and not int((out["flags"] & 0xC0).any())
    sim, fin = copies.sim, out["env"]
    for f in ("board", "rng", "timer", "eff"):
        assert torch.equal(getattr(fin, f), getattr(sim, f)), f"final {f} differs"
    del out, fin
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    repeats = args.repeats
    for r in range(args.repeats):
        if r >= repeats:
            break
        for v, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1))
        if r == 0:
            repeats = max(5, min(args.repeats, int(BUDGET_MS / max(ms[v][0] for v in variants))))
    assert env.status() == 0 and sim.status() == 0, "device status"
    r = {"shape": name, "envs": n, "seqs": Q, "depth": D, "kind": kind, "plies": Q * n * D,
         "repeats": len(ms["playout"]), "lib_variant": info["variant"], "src": info["src"][:16]}
    for v, xs in ms.items():                                     # per variant: median, min, max in ms
        r[v] = [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]
    print(json.dumps(r), flush=True)
    return [r]


def run_shape(name, args, torch):
    from tile_match_gym_amd import _native
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    R, C, k, cl, co = SHAPES[name]
    info = _native.build_info(args.lib)
    res = []
    for n in args.envs:
        env = TileMatchVecEnv(n, R, C, k, MOVES, cl, co, seed=0, device="cuda:0", groups=1, lib_path=args.lib)
        env.reset()
        for t in range(POLICY_STEPS):
            env.step_effective(t, key=KEY)
        env.join()
        torch.cuda.synchronize()
        assert POLICY_STEPS + max(args.depths) <= MOVES, "the sequences must end before the episode does"
        for Q in args.seqs:
            copies = StepCopies(env, Q, torch)
            for D in args.depths:
                for kind in args.kinds:
                    res += run_case(env, copies, name, Q, D, kind, args, torch, info)
            copies.close()
            del copies
            torch.cuda.empty_cache()
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,c5")
    ap.add_argument("--envs", default="64,4096")
    ap.add_argument("--seqs", default="16,256")
    ap.add_argument("--depths", default="4,16")
    ap.add_argument("--kinds", default="uniform,masked")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libtmg.so (an A/B variant)")
    args = ap.parse_args()
    args.envs = [int(x) for x in args.envs.split(",")]
    args.seqs = [int(x) for x in args.seqs.split(",")]
    args.depths = [int(x) for x in args.depths.split(",")]
    args.kinds = args.kinds.split(",")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("playout_bench needs a HIP device: there is no CPU fallback")
    out = []
    for name in args.shapes.split(","):
        out += run_shape(name, args, torch)
    print(json.dumps({"playout_bench": out}))


if __name__ == "__main__":
    main()
