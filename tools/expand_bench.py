"""Expansion throughput: tmg_expand against the way the same children are built
with tmg_step alone.

For each shape (c2: 65 536 x 10x10 k4 without specials; c3: 262 144 x 10x10 k4
with v/h-laser + bomb; g1: 65 536 x 10x10 k5 without specials; c5: 16 384 x
20x20 k6 with all specials — a sixteenth of the bench's c5 batch, whose
children would not fit twice), after a reset and 10 steps of the
effective-action policy, it times with HIP events, after warm-up, two ways of
producing every effective child (board, RNG words, timer, mask, and what the
move reports):

  (e) expand        TileMatchVecEnv.expand(): tmg_expand_count, the host's read
                    of the total, the allocation of the child rows, tmg_expand;
  (c) step_copies   tools/peek_bench.py's mode (c): the (N, A) effective-action
                    mask from the bitmask, repeat_interleave of board / rng /
                    timer / eff to one row per (env, effective action), and one
                    tmg_step over the copies (copies and the host's wait for the
                    row count included).

Both run the same step kernel on the same rows.  The two are measured in turn
within each repeat, so drift of the machine falls on both alike.  Rates are
children per second.  Prints one JSON line per (shape, variant) and a final
JSON line with all of them; the children of the two sides are compared, every
array, before anything is timed.

    python tools/expand_bench.py [--shapes c2,c3,g1,c5] [--repeats 20] [--warmup 3] [--lib PATH] [--envs N]
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

ALL = ["cookie"], ["vertical_laser", "horizontal_laser", "bomb"]
SHAPES = {
    # name: (envs, R, C, k, colourless specials, colour specials)
    "c2": (65536, 10, 10, 4, [], []),
    "c3": (262144, 10, 10, 4, [], ["vertical_laser", "horizontal_laser", "bomb"]),
    "g1": (65536, 10, 10, 5, [], []),
    "c5": (16384, 20, 20, 6, ALL[0], ALL[1]),
}
KEY = 12345
MOVES = 30
POLICY_STEPS = 10


def step_copies(env, torch):
    """(c): every effective (env, action) stepped on a copy of its env, with the calls a user had before tmg_expand."""
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
    return {"board": board, "rng": rng, "timer": timer, "eff": eff, "action": actions, "reward": out[0],
            "n_new": out[1], "n_act": out[2], "flags": flags}


def expand(env):
    exp = env.expand()
    if exp.env is not None:
        exp.env.close()                                      # the children's step plans (events), not their tensors
    return exp


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
    # the two sides agree on every array before anything is timed
    want = step_copies(env, torch)
    exp = env.expand()
    torch.cuda.synchronize()
    E = exp.count
    assert E == want["action"].numel(), "expand and step-on-copies disagree on the child count"
    for f in ("board", "rng", "timer", "eff"):
        assert torch.equal(getattr(exp.env, f), want[f]), f"expand and step-on-copies disagree on {f}"
    for f in ("action", "reward", "n_new", "n_act", "flags"):
        assert torch.equal(getattr(exp, f), want[f]), f"expand and step-on-copies disagree on {f}"
    assert not int((exp.flags & 0xC0).any())
    exp.env.close()
    del want, exp
    variants = {"expand": lambda: expand(env), "step_copies": lambda: step_copies(env, torch)}
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
        r = {"shape": name, "variant": v, "envs": n, "actions": env.num_actions, "children": E,
             "repeats": len(xs), "ms_median": round(med, 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4),
             "children_per_s_median": round(E / (med * 1e-3), 1), "lib_variant": info["variant"], "src": info["src"][:16]}
        print(json.dumps(r), flush=True)
        res.append(r)
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3,g1,c5")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libtmg.so (an A/B variant)")
    ap.add_argument("--envs", type=int, default=0, help="override the shape's env count (rehearsal)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("expand_bench needs a HIP device: there is no CPU fallback")
    out = []
    for name in args.shapes.split(","):
        out += run_shape(name, args, torch)
    print(json.dumps({"expand_bench": out}))


if __name__ == "__main__":
    main()
