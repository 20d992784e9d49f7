"""One-ply lookahead throughput: tmg_peek against the way the same question is
answered with tmg_step alone.

For each shape (c2: 65 536 x 10x10 k4 without specials; c3: 262 144 x 10x10 k4
with v/h-laser + bomb), after a reset and 10 steps of the effective-action
policy, it times with HIP events, after warm-up:

  (a) peek_reward   tmg_peek writing the (N, A) reward table only;
  (b) peek_best     tmg_peek writing best_action / best_reward only;
  (c) step_copies   the existing API only: the (N, A) effective-action mask
                    from the bitmask, repeat_interleave of board / rng / timer /
                    eff to one row per (env, effective action), and one tmg_step
                    over the copies (copies and the host's wait for the row
                    count included).

The three are measured in turn within each repeat, so drift of the machine
falls on all of them alike.  Rates are simulated effective moves per second.
Prints one JSON line per (shape, variant) and a final JSON line with all of
them; the reward tables of (a) and (c) are compared before anything is timed.

    python tools/peek_bench.py [--shapes c2,c3] [--repeats 20] [--warmup 3] [--lib PATH] [--envs N]
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
    # not in the default set: 5 colours, where tmg_step has no shape-specialised kernel either
    "g1": (65536, 10, 10, 5, [], []),
}
KEY = 12345
MOVES = 30
POLICY_STEPS = 10


def step_copies(env, torch, keep=None):
    """(c): every effective (env, action) stepped on a copy of its env, with the calls a user has today."""
    mask = env.effective_mask()                              # (N, A) bool
    counts = mask.sum(dim=1)
    actions = mask.nonzero()[:, 1].to(torch.int32).contiguous()
    E = actions.numel()                                      # the host waits for the count here
    board = torch.repeat_interleave(env.board, counts, dim=0)
    rng = torch.repeat_interleave(env.rng, counts, dim=0)
    timer = torch.repeat_interleave(env.timer, counts, dim=0)
    eff = torch.repeat_interleave(env.eff, counts, dim=0)
    out = torch.empty((3, E), dtype=torch.int32, device=env.device)
    flags = torch.empty(E, dtype=torch.uint8, device=env.device)
    env.ctx.step(E, board.data_ptr(), rng.data_ptr(), timer.data_ptr(), actions.data_ptr(), out[0].data_ptr(),
                 out[1].data_ptr(), out[2].data_ptr(), flags.data_ptr(), eff.data_ptr(), 1, 0, env._stream())
    if keep is not None:
        keep.update(mask=mask, reward=out[0], flags=flags)
    return E


def run_shape(name, args, torch):
    from tile_match_gym_amd import _native
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    n, R, C, k, cl, co = SHAPES[name]
    n = args.envs or n
    env = TileMatchVecEnv(n, R, C, k, MOVES, cl, co, seed=0, device="cuda:0", groups=1, lib_path=args.lib)
    env.reset()
    for t in range(POLICY_STEPS):
        env.step_effective(t, key=KEY)
    env.join()
    torch.cuda.synchronize()
    variants = {
        "peek_reward": lambda: env.peek(outputs=("reward",)),
        "peek_best": lambda: env.peek(outputs=(), best=True),
        "step_copies": lambda: step_copies(env, torch),
    }
    # the three answers agree before anything is timed
    kept = {}
    E = step_copies(env, torch, kept)
    table = env.peek(outputs=("reward", "flags"), best=True)
    torch.cuda.synchronize()
    assert torch.equal(table["reward"][kept["mask"]], kept["reward"]), "peek and step-on-copies disagree on rewards"
    assert int((table["reward"] != 0).sum()) == int((table["reward"][kept["mask"]] != 0).sum())
    assert torch.equal(table["best_reward"], table["reward"].max(dim=1).values)
    assert not int((kept["flags"] & 0xC0).any()) and not int((table["flags"] & 0xC0).any())
    del kept, table
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
    assert env.status() == 0, "device status"
    info = _native.build_info(args.lib)
    res = []
    for v, xs in ms.items():
        med = statistics.median(xs)
        r = {"shape": name, "variant": v, "envs": n, "actions": env.num_actions, "effective_moves": E,
             "repeats": len(xs), "ms_median": round(med, 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4),
             "moves_per_s_median": round(E / (med * 1e-3), 1), "lib_variant": info["variant"], "src": info["src"][:16]}
        print(json.dumps(r), flush=True)
        res.append(r)
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libtmg.so (an A/B variant)")
    ap.add_argument("--envs", type=int, default=0, help="override the shape's env count (rehearsal)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("peek_bench needs a HIP device: there is no CPU fallback")
    out = []
    for name in args.shapes.split(","):
        out += run_shape(name, args, torch)
    print(json.dumps({"peek_bench": out}))


if __name__ == "__main__":
    main()
