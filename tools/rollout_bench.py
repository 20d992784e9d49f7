"""Policy-rollout throughput: tmg_rollout against the way the same simulation is
run with the stepping API alone.

For each shape (c2: 65 536 x 10x10 k4 without specials; c3: 262 144 x 10x10 k4
with v/h-laser + bomb; g1: 65 536 x 10x10 k5 without specials), after a reset
and 10 steps of the effective-action policy, and for each (depth, samples), it
times with HIP events, after warm-up:

  (a) rollout       tmg_rollout writing the (S, N, A) return table;
  (b) step_copies   the stepping API only: the (N, A) effective-action mask
                    from the bitmask, repeat_interleave of board / rng / timer /
                    eff to one row per (sample, env, effective action) into a
                    second batch, one step with the rows' actions, then
                    depth - 1 steps of the in-kernel effective-action policy
                    (copies and the host's wait for the row count included;
                    the second batch's buffers are allocated once, outside
                    the timing).

The two are measured in turn within each repeat, so drift of the machine falls
on both alike.  Both simulate E * samples * depth moves, E the number of
effective (env, action) pairs; rates are simulated moves per second.  (b)
draws its continuation actions from another stream than (a) (one key for the
whole second batch), so the returns agree in distribution only; at depth 1 and
one sample they are compared exactly before anything is timed.  Peak extra
device memory is torch's high-water mark over one call of each way, the
second batch of (b) included.  Prints one JSON line per (shape, depth,
samples, variant) and a final JSON line with all of them.

    python tools/rollout_bench.py [--shapes c2,c3,g1] [--depths 4,16] [--samples 1,4] [--repeats 20]
                                  [--warmup 3] [--lib PATH] [--envs N]
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
    # name: (envs, R, C, k, colourless specials, colour specials)
    "c2": (65536, 10, 10, 4, [], []),
    "c3": (262144, 10, 10, 4, [], ["vertical_laser", "horizontal_laser", "bomb"]),
    "g1": (65536, 10, 10, 5, [], []),
}
KEY = 12345
MOVES = 30
POLICY_STEPS = 10


class StepCopies:
    """(b): a second batch of one row per (sample, env, effective action)."""

    def __init__(self, env, samples, words, torch):
        from tile_match_gym_amd.vec_env import TileMatchVecEnv
        self.env, self.samples, self.words, self.torch = env, samples, words, torch
        self.rows = int(env.effective_mask().sum()) * samples
        self.sim = TileMatchVecEnv(self.rows, env.num_rows, env.num_cols, env.num_colours, env.num_moves,
                                   env.colourless_specials, env.colour_specials, seed=0, device=env.device,
                                   autoreset=False, groups=1)

    def __call__(self, depth):
        torch, env, sim, S = self.torch, self.env, self.sim, self.samples
        mask = env.effective_mask()                              # (N, A) bool
        counts = mask.sum(dim=1)
        actions = mask.nonzero()[:, 1].to(torch.int32)
        E = actions.numel()                                      # the host waits for the count here
        assert E * S == self.rows
        for s in range(S):
            lo, hi = s * E, (s + 1) * E
            sim.board[lo:hi] = torch.repeat_interleave(env.board, counts, dim=0)
            sim.rng[lo:hi] = torch.repeat_interleave(self.words[s], counts, dim=0)
            sim.timer[lo:hi] = torch.repeat_interleave(env.timer, counts, dim=0)
            sim.eff[lo:hi] = torch.repeat_interleave(env.eff, counts, dim=0)
        sim._eff_valid = True
        ret = torch.zeros(self.rows, dtype=torch.int32, device=env.device)
        sim.step_raw(actions.repeat(S).contiguous())
        ret += sim.reward
        for d in range(1, depth):
            sim.step_effective(d, key=KEY)
            ret += sim.reward
        return E, mask, ret

    def close(self):
        self.sim.close()


def run_shape(name, args, torch):
    from tile_match_gym_amd import _native
    from tile_match_gym_amd.seeding import batch_rng_words
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    n, R, C, k, cl, co = SHAPES[name]
    n = args.envs or n
    dev = "cuda:0"
    env = TileMatchVecEnv(n, R, C, k, MOVES, cl, co, seed=0, device=dev, groups=1, lib_path=args.lib)
    env.reset()
    for t in range(POLICY_STEPS):
        env.step_effective(t, key=KEY)
    env.join()
    torch.cuda.synchronize()
    info = _native.build_info(args.lib)
    res = []
    for S in args.samples:
        import numpy as np
        words = torch.from_numpy(np.stack([batch_rng_words(range(10 ** 6 * (s + 1), 10 ** 6 * (s + 1) + n))
                                           for s in range(S)]).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        copies = StepCopies(env, S, words, torch)
        if S == 1:                                               # depth 1, one sample: the same moves exactly
            E, mask, ret = copies(1)
            table = env.rollout(1, 1, rng=words, outputs=("ret", "flags"))
            torch.cuda.synchronize()
            assert torch.equal(table["ret"][0][mask], ret), "rollout and step-on-copies disagree at depth 1"
            assert not int((table["flags"] & 0xC0).any())
            del table, mask, ret
        for depth in args.depths:
            variants = {"rollout": lambda: env.rollout(depth, S, rng=words, key=KEY, outputs=("ret",)),
                        "step_copies": lambda: copies(depth)}
            # what both ways played, and their memory high-water marks, before anything is timed
            env._roll_bufs.clear()                               # rollout's tables are allocated by its first call
            torch.cuda.reset_peak_memory_stats()
            E = copies(depth)[0]
            torch.cuda.synchronize()
            mem = {"step_copies": torch.cuda.max_memory_allocated() - base}
            sim_bytes = torch.cuda.memory_allocated() - base      # the second batch stays allocated
            torch.cuda.reset_peak_memory_stats()
            out = env.rollout(depth, S, rng=words, key=KEY, outputs=("ret", "plies"))
            torch.cuda.synchronize()
            mem["rollout"] = torch.cuda.max_memory_allocated() - base - sim_bytes
            moves = int(out["plies"].sum())
            assert moves == E * S * depth, (moves, E, S, depth)
            for _ in range(args.warmup):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            ms = {v: [] for v in variants}
            for _ in range(args.repeats):
                for v, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms[v].append(e0.elapsed_time(e1))
            assert env.status() == 0 and copies.sim.status() == 0, "device status"
            for v, xs in ms.items():
                med = statistics.median(xs)
                r = {"shape": name, "variant": v, "envs": n, "actions": env.num_actions, "depth": depth, "samples": S,
                     "effective_pairs": E, "moves": moves, "repeats": len(xs), "ms_median": round(med, 4),
                     "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4),
                     "moves_per_s_median": round(moves / (med * 1e-3), 1), "peak_extra_bytes": int(mem[v]),
                     "lib_variant": info["variant"], "src": info["src"][:16]}
                print(json.dumps(r), flush=True)
                res.append(r)
        copies.close()
        del copies, words
        env._roll_bufs.clear()
        torch.cuda.empty_cache()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,g1")
    ap.add_argument("--depths", default="4,16")
    ap.add_argument("--samples", default="1,4")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libtmg.so (an A/B variant)")
    ap.add_argument("--envs", type=int, default=0, help="override the shape's env count (rehearsal)")
    args = ap.parse_args()
    args.depths = [int(x) for x in args.depths.split(",")]
    args.samples = [int(x) for x in args.samples.split(",")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench needs a HIP device: there is no CPU fallback")
    out = []
    for name in args.shapes.split(","):
        out += run_shape(name, args, torch)
    print(json.dumps({"rollout_bench": out}))


if __name__ == "__main__":
    main()
