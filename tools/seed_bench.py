"""Seeding throughput: tmg_seed on the device against the host loop it replaces.

For each m (4 096, 65 536, 262 144 env streams, and 16 x 1 024, the words of a
16-sample lookahead over 1 024 envs) it times, after warm-up:

  (a) tmg_seed into an (m, 5) device buffer, with HIP events:
        range         TMG_SEED_INT, seeds base + j (nothing uploaded);
        array         TMG_SEED_INT on an (m,) uint64 seed array: the H2D copy
                      of the packed host array and the kernel (the packing on
                      the host is outside the events and reported as pack_ms);
        array_device  the same kernel on seeds already on the device;
        spawn         TMG_SEED_SPAWN, key (j / 1 024, j % 1 024);
      each with the library's default store variant, and at the largest m the
      range form with the direct and the staged store (--stores);
  (b) host          the parent's way: seeding.batch_rng_words (one
                    np.random.PCG64 per seed) and .to(device), wall-clock with
                    a final synchronize (--host-repeats runs; 0 leaves the host
                    out, for sizes it would take too long at: the device rows
                    are then not compared with numpy's either).

With --constructor it also times TileMatchVecEnv(n, 10, 10, 4, 30, specials
of c3) at the c3 batch size, wall-clock from the call to a synchronize after
it (the context, the state tensors and the seeding; the first construction,
which also loads the library's code objects, is reported apart).  Run it on
the parent commit as well for the "before" figure: nothing here needs tmg_seed
unless a seed variant is asked for (--no-seed skips them).

Prints one JSON line per (m, variant) and a final JSON line with all of them.

    python tools/seed_bench.py [--sizes 4096,65536,262144,16384] [--repeats 50] [--warmup 5]
                               [--host-repeats 3] [--constructor] [--no-seed] [--lib PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tile-match-gym_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = "cuda:0"
BASE = 10 ** 6
C3 = (262144, 10, 10, 4, 30, [], ["vertical_laser", "horizontal_laser", "bomb"])


def _events(fn, repeats, warmup, torch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def _row(m, variant, ms, info, **extra):
    med = statistics.median(ms)
    r = {"m": m, "variant": variant, "repeats": len(ms), "ms_median": round(med, 5), "ms_min": round(min(ms), 5),
         "ms_max": round(max(ms), 5), "us_per_stream": round(med * 1e3 / m, 6),
         "streams_per_s_median": round(m / (med * 1e-3), 1), "lib_variant": info["variant"], "src": info["src"][:16]}
    r.update(extra)
    print(json.dumps(r), flush=True)
    return r


def run_size(m, args, ctx, info, torch, stores):
    import numpy as np
    from tile_match_gym_amd import _native
    from tile_match_gym_amd.seeding import batch_rng_words, pack_seeds
    res = []
    host_ms = []
    want = None
    for _ in range(args.host_repeats):                          # (b) the parent's way
        t0 = time.perf_counter()
        w = torch.from_numpy(batch_rng_words(range(BASE, BASE + m)).view(np.int64)).to(DEV)
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        want = w
    if args.no_seed:
        return [_row(m, "host", host_ms, info)]
    buf = torch.empty((m, 5), dtype=torch.int64, device=DEV)
    stream = 0

    def seed(**kw):
        ctx.seed(m, buf.data_ptr(), stream, **kw)

    # what is timed is what numpy gives
    seeds_list = list(range(BASE, BASE + m))
    t0 = time.perf_counter()
    packed = pack_seeds(seeds_list)[1]
    pack_ms = (time.perf_counter() - t0) * 1e3
    on_dev = torch.from_numpy(packed.view(np.int64)).to(DEV)
    for kw in (dict(base=BASE), dict(seeds=on_dev.data_ptr())):
        buf.zero_()
        seed(**kw)
        torch.cuda.synchronize()
        assert want is None or torch.equal(buf, want), "tmg_seed and numpy disagree"

    def upload_and_seed():
        d = torch.from_numpy(packed.view(np.int64)).to(DEV)
        ctx.seed(m, buf.data_ptr(), stream, seeds=d.data_ptr())

    variants = [("range", lambda: seed(base=BASE), {}),
                ("array", upload_and_seed, {"pack_ms": round(pack_ms, 4)}),
                ("array_device", lambda: seed(seeds=on_dev.data_ptr()), {}),
                ("spawn", lambda: seed(mode=_native.SEED_SPAWN, base=BASE, key1=0, period=1024), {})]
    if stores:
        variants += [("range_direct", lambda: seed(mode=_native.SEED_STORE_DIRECT, base=BASE), {}),
                     ("range_staged", lambda: seed(mode=_native.SEED_STORE_STAGED, base=BASE), {})]
    for name, fn, extra in variants:
        ms = _events(fn, args.repeats, args.warmup, torch)
        if host_ms:
            extra = dict(extra, host_over_this=round(statistics.median(host_ms) / statistics.median(ms), 1))
        res.append(_row(m, name, ms, info, **extra))
    if host_ms:
        res.append(_row(m, "host", host_ms, info))
    return res


def constructor(args, info, torch):
    from tile_match_gym_amd.vec_env import TileMatchVecEnv
    n, R, C, k, moves, cl, co = C3
    n = args.envs or n
    ms = []
    for _ in range(args.constructor_repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env = TileMatchVecEnv(n, R, C, k, moves, cl, co, seed=0, device=DEV, lib_path=args.lib)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        env.close()
        del env
    r = {"constructor": "TileMatchVecEnv c3", "envs": n, "first_ms": round(ms[0], 3),
         "ms_median": round(statistics.median(ms[1:]), 3), "ms_min": round(min(ms[1:]), 3),
         "ms_max": round(max(ms[1:]), 3), "repeats": len(ms) - 1, "lib_variant": info["variant"], "src": info["src"][:16]}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536,262144,16384")
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--stores", action="store_true", help="direct / staged store at every m, not only the largest")
    ap.add_argument("--constructor", action="store_true", help="also time TileMatchVecEnv(...) at the c3 shape")
    ap.add_argument("--constructor-repeats", type=int, default=3)
    ap.add_argument("--no-seed", action="store_true", help="host figures only (a library without tmg_seed)")
    ap.add_argument("--envs", type=int, default=0, help="override the constructor's env count (rehearsal)")
    ap.add_argument("--lib", default=None, help="another build of libtmg.so (an A/B variant)")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seed_bench needs a HIP device: there is no CPU fallback")
    from tile_match_gym_amd import _native
    info = _native.build_info(args.lib)
    ctx = _native.Context(0, 10, 10, 4, 0, 30, lib_path=args.lib)
    out = []
    for m in sizes:
        out += run_size(m, args, ctx, info, torch, args.stores or m == max(sizes))
    ctx.close()
    if args.constructor:
        out.append(constructor(args, info, torch))
    print(json.dumps({"seed_bench": out}))


if __name__ == "__main__":
    main()
