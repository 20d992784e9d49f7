"""TileMatchVecEnv — N independent TileMatchEnv boards stepped by one HIP launch.

State lives in PyTorch-ROCm tensors on one device (layout: include/tmg.h);
each reset/step enqueues one kernel on the current torch stream through the
C ABI.  Per env the semantics are the reference's TileMatchEnv
(tile_match_env.py:84-124) with one numpy PCG64 stream per env, so env i
seeded with s follows exactly the trajectory of TileMatchEnv(..., seed=s).

Autoreset (default on): an env whose episode ends is regenerated inside the
same step call, continuing its RNG stream (== the reference's reset() without
a seed, tile_match_env.py:84-87); reward/flags describe the final move,
`info["final_board"]` is not kept (pass autoreset=False to inspect it).

groups > 1: the envs are split into that many contiguous groups, each stepped
on its own HIP stream, so the tail of one group's launch overlaps the next
launch of another (envs are independent; results are identical to
groups=1).  `step_raw` then only enqueues: call `join()` before reading the
state or outputs on the current stream (`step`, `reset` and the other
accessors join themselves).
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import _native
from .seeding import batch_rng_words, pack_seeds, rng_words_from_seed

CHECKPOINT_FORMAT = 1
_STATE_ARRAYS = ("board", "rng", "timer", "eff")


def save_state(path, arrays: dict, config: dict) -> None:
    """Write a batched-env checkpoint: the four state arrays (include/tmg.h
    layout) plus the env config as JSON, in one .npz (no pickled objects)."""
    meta = dict(config, format=CHECKPOINT_FORMAT)
    np.savez(path, config=np.array(json.dumps(meta, sort_keys=True)),
             **{k: np.ascontiguousarray(arrays[k]) for k in _STATE_ARRAYS})


def load_state(path):
    """(arrays, config) of a checkpoint written by save_state (numpy.load with
    allow_pickle=False)."""
    with np.load(path, allow_pickle=False) as z:
        config = json.loads(str(z["config"]))
        if config.get("format") != CHECKPOINT_FORMAT:
            raise ValueError(f"unsupported checkpoint format {config.get('format')!r}")
        arrays = {k: z[k].copy() for k in _STATE_ARRAYS}
    return arrays, config


def _ptr(t: torch.Tensor):
    return t.data_ptr() if t is not None else None


def _raw_stream(device_index: int) -> int:
    """The current HIP stream of the device as a raw handle (the cheap accessor
    when this torch has it)."""
    return torch.cuda.current_stream(device_index).cuda_stream


if hasattr(torch._C, "_cuda_getCurrentRawStream"):
    _raw_stream = torch._C._cuda_getCurrentRawStream        # noqa: F811


class Expansion:
    """What TileMatchVecEnv.expand returns.  count: the number of child rows;
    first_child: (N + 1,) int64, env i's children are rows first_child[i] to
    first_child[i + 1] (first_child[N] is the total, which count is unless
    max_children cut it); per child row: parent (int64, its env), action,
    reward, n_new, n_act (int32) and flags (uint8), what the move reported (as
    a step with autoreset off: FLAG_DONE on a child that used the last move);
    env: a TileMatchVecEnv over the children's boards, RNG words, timers and
    masks (None when count == 0), with the parent's shape, colours, specials and
    num_moves, autoreset mode "none", the mask cache valid and no reset run, so
    env.peek(), env.rollout(), env.step_raw() and env.expand() work on it
    directly.  It shares the parent env's context: close the parent last."""

    __slots__ = ("count", "first_child", "parent", "action", "reward", "n_new", "n_act", "flags", "env")

    def __init__(self, count, first_child, parent, action, reward, n_new, n_act, flags, env):
        self.count, self.first_child, self.parent, self.action = count, first_child, parent, action
        self.reward, self.n_new, self.n_act, self.flags, self.env = reward, n_new, n_act, flags, env


class TileMatchVecEnv:
    def __init__(self, num_envs: int, num_rows: int, num_cols: int, num_colours: int, num_moves: int,
                 colourless_specials=(), colour_specials=(), seed: int = 0, seeds=None, device=None,
                 autoreset: bool = True, groups: int = 1, lib_path: str = None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise _native.TmgError("TileMatchVecEnv runs on a HIP device only (no CPU fallback)")
        self.device = device
        self.num_envs = int(num_envs)
        self.num_rows, self.num_cols, self.num_colours, self.num_moves = num_rows, num_cols, num_colours, num_moves
        self.colourless_specials = list(colourless_specials)
        self.colour_specials = list(colour_specials)
        self.specials_mask = _native.specials_mask(colourless_specials, colour_specials)
        # the one source of truth for the autoreset semantics: "none",
        # "same_step" or "next_step" (set_step_outputs); `autoreset` derives from it
        self._autoreset_mode = "same_step" if autoreset else "none"
        # lib_path: another build of libtmg.so (a diagnostic variant) for this env's context
        self.ctx = _native.Context(device.index if device.index is not None else torch.cuda.current_device(),
                                   num_rows, num_cols, num_colours, self.specials_mask, num_moves, lib_path=lib_path)
        self.num_actions = self.ctx.num_actions
        self.mask_words = self.ctx.mask_words
        N = self.num_envs
        kw = dict(device=device)
        self.board = torch.zeros((N, 2, num_rows, num_cols), dtype=torch.int8, **kw)
        if seeds is None:
            seeds = range(int(seed), int(seed) + N)
        self._dev_index = device.index if device.index is not None else torch.cuda.current_device()
        self.rng = torch.empty((N, 5), dtype=torch.int64, **kw)
        self._seed_rng(seeds)
        self.timer = torch.zeros(N, dtype=torch.int32, **kw)
        self.eff = torch.zeros((N, self.mask_words), dtype=torch.int64, **kw)
        self.reward = torch.zeros(N, dtype=torch.int32, **kw)
        self.n_new = torch.zeros(N, dtype=torch.int32, **kw)
        self.n_act = torch.zeros(N, dtype=torch.int32, **kw)
        self.flags = torch.zeros(N, dtype=torch.uint8, **kw)
        self.actions = None                     # step_effective's sampled actions (N,) int32
        self._peek_bufs = {}                    # peek's output tensors, allocated on first use
        self._roll_bufs = {}                    # rollout's, by sample count
        self.onehot = None                      # fused one-hot planes (attach_onehot)
        self._oh_code = _native.DTYPE_F32
        self._eff_valid = False
        groups = max(1, min(int(groups), N))
        self.groups = groups
        bounds = [g * N // groups for g in range(groups + 1)]
        self._ranges = [(bounds[g], bounds[g + 1]) for g in range(groups) if bounds[g + 1] > bounds[g]]
        self._streams = [torch.cuda.Stream(device) for _ in self._ranges] if groups > 1 else []
        # step plans (tmg_plan_*): one host call per batched step enqueues every
        # group's launches with their fork event; one plan per action source
        # (given actions / the in-kernel effective-action policy), configured
        # with the attached outputs
        bounds = [lo for lo, _ in self._ranges] + [N]
        streams = [st.cuda_stream for st in self._streams] if self._streams else [0]
        self._plans = {pol: _native.Plan(self.ctx, N, _ptr(self.board), _ptr(self.rng), _ptr(self.timer),
                                         _ptr(self.reward), _ptr(self.n_new), _ptr(self.n_act), _ptr(self.flags),
                                         _ptr(self.eff), bounds, streams) for pol in (False, True)}
        self._policy = (12345, 0)                   # (key, first_env) the policy plan is configured with
        self._vout = {}                             # extra outputs (set_step_outputs)
        self._held = []                             # action tensors the queued steps still read
        self._configure()

    # ----------------------------------------------------------------- API
    @property
    def autoreset(self) -> bool:
        """Whether envs whose episode ends are reset (same step or, after
        set_step_outputs("next_step"), the next one).  Settable: True keeps a
        next-step mode and otherwise selects same-step; False selects none (the
        step plans are reconfigured)."""
        return self._autoreset_mode != "none"

    @property
    def autoreset_mode(self) -> str:
        return self._autoreset_mode

    @autoreset.setter
    def autoreset(self, value):
        mode = ("next_step" if self._autoreset_mode == "next_step" else "same_step") if value else "none"
        if mode != self._autoreset_mode:
            self.join()
            self._autoreset_mode = mode
            self._configure()

    def _stream(self):
        return _raw_stream(self._dev_index)

    def _configure(self):
        """(Re)configure both step plans: autoreset mode, fused one-hot planes,
        vector-env outputs, the policy's key and shard offset."""
        for pol, plan in self._plans.items():
            plan.config(self._autoreset_mode, policy=pol, key=self._policy[0], first_env=self._policy[1],
                        onehot=_ptr(self.onehot), onehot_dtype=self._oh_code, **self._vout)

    def set_step_outputs(self, autoreset_mode: str = None, terminated=None, action_mask=None, moves_left=None,
                         final_board=None, board32=None):
        """Outputs every step writes in the kernels' own write-back (tmg_plan_config):
        terminated (N, 4) uint8 (terminated, is_combination_match, shuffled, error),
        action_mask (N, A) uint8/bool (kept up to date: rows are rewritten where the
        mask changes, so initialise it after a reset), moves_left (N,) int64,
        final_board (N, 2, R, C) int8 (same-step autoreset: the last board of each
        env whose episode ended), board32 (N, 2, R, C) int32 (the boards in the
        reference's observation dtype, kept up to date like action_mask).
        autoreset_mode: "none", "same_step", "next_step"."""
        self.join()
        if autoreset_mode is not None:
            if autoreset_mode not in ("none", "same_step", "next_step"):
                raise ValueError("autoreset_mode must be 'none', 'same_step' or 'next_step'")
            self._autoreset_mode = autoreset_mode
        self._vout = {k: _ptr(v) for k, v in (("terminated", terminated), ("action_mask", action_mask),
                                               ("moves_left", moves_left), ("final_board", final_board),
                                               ("board32", board32))}
        self._vout_refs = (terminated, action_mask, moves_left, final_board, board32)
        self._configure()

    def set_seed(self, seeds):
        """Re-seed every env (== tile_match_env.py:79-82 per env): one seed per
        env, as a range, a list / tuple, an integer ndarray or tensor (seeded on
        the device, tmg_seed) or any other iterable of ints (seeded by numpy on
        the host, as are seeds of 2^128 and more).  A negative seed raises
        ValueError."""
        self.join()
        self._seed_rng(seeds)

    def _seed_rng(self, seeds):
        """self.rng <- np.random.default_rng(seed) of every env's seed."""
        N = self.num_envs
        if isinstance(seeds, torch.Tensor):
            seeds = seeds.detach().cpu().numpy()
        how = pack_seeds(seeds)
        if how is None:                            # only numpy can: the host loop
            w = batch_rng_words(seeds)
            if w.shape[0] != N:
                raise ValueError(f"{w.shape[0]} seeds for {N} envs")
            self.rng.copy_(torch.from_numpy(w.view(np.int64)))
        elif how[0] == "range":
            if how[2] != N:
                raise ValueError(f"{how[2]} seeds for {N} envs")
            self.ctx.seed(N, _ptr(self.rng), self._stream(), base=how[1])
        else:
            a = how[1]
            if a.shape[0] != N:
                raise ValueError(f"{a.shape[0]} seeds for {N} envs")
            d = torch.from_numpy(a.view(np.int64)).to(self.device)
            self.ctx.seed(N, _ptr(self.rng), self._stream(), seeds=_ptr(d), seed_words=a.ndim)

    def fresh_rng(self, samples: int, entropy: int, first_env: int = 0) -> torch.Tensor:
        """New PCG64 words for a sampled lookahead, seeded on the device
        (tmg_seed): an (S, N, 5) int64 tensor whose row (s, i) is
        np.random.default_rng(np.random.SeedSequence(entropy, spawn_key=(s,
        first_env + i))), so a shard passing its global offset as first_env gets
        the unsharded batch's streams.  entropy: a non-negative int below
        2^128.  Enqueues on the current stream."""
        samples, first_env = int(samples), int(first_env)
        if samples < 1:
            raise ValueError("samples must be >= 1")
        if first_env < 0:
            raise ValueError("first_env must be >= 0")
        N = self.num_envs
        w = torch.empty((samples, N, 5), dtype=torch.int64, device=self.device)
        self.ctx.seed(samples * N, _ptr(w), self._stream(), mode=_native.SEED_SPAWN, base=entropy, key1=first_env,
                      period=N)
        return w

    def stagger_phases(self, blocks: int = 0, first_env: int = 0, interleave: bool = False, shift: int = 0):
        """Offset the episode phases right after a reset by setting timers.  A
        timer of m is the state after m ineffective moves (board.py:352-353: no
        board or RNG change; tile_match_env.py:100 counts the move).

        blocks = 0: env i gets (first_env + i) mod num_moves, so every step
        finishes ~N/num_moves episodes (pass the shard's global offset as
        first_env to keep the layout shard-invariant).
        blocks = P > 0: each env group's range is split into Pg = ceil(P / groups)
        contiguous sub-blocks; sub-block j of group g starts at phase
        j * M / Pg + g * M / (Pg * groups) (M = num_moves, floors).  Every
        group then finishes a sub-block's episodes every M / Pg steps, and the
        groups take turns, so a window of a multiple of M / Pg steps holds the
        same reset work on every group's stream.
        interleave=True: env i belongs to block i mod P instead, so every group
        stream holds an equal part of every block's resets.
        shift: every phase advanced by `shift` steps (mod num_moves), i.e. the
        whole reset schedule moved `shift` steps earlier; the reset work per
        window of a multiple of the block spacing is unchanged."""
        self.join()
        N, M = self.num_envs, self.num_moves
        if blocks == 1:
            self.timer.zero_()
        elif blocks and blocks > 0 and interleave:
            # interleaved blocks: env i in block i mod P (every env group holds
            # all P blocks), block b starting at b * M // P
            i = torch.arange(N, device=self.device, dtype=torch.int64)
            self.timer.copy_(((i % blocks) * M // blocks % M).to(torch.int32))
        elif blocks and blocks > 0:
            G = len(self._ranges)
            Pg = max(1, -(-int(blocks) // G))
            t = torch.zeros(N, dtype=torch.int64)
            for g, (lo, hi) in enumerate(self._ranges):
                n = hi - lo
                for j in range(Pg):
                    a, b = lo + j * n // Pg, lo + (j + 1) * n // Pg
                    t[a:b] = (j * M // Pg + g * M // (Pg * G) + shift) % M
            self.timer.copy_(t.to(torch.int32).to(self.device))
        else:
            g = torch.arange(first_env, first_env + N, device=self.device, dtype=torch.int64)
            self.timer.copy_((g % M).to(torch.int32))

    def status(self, clear: bool = False) -> int:
        """Sticky _native.STATUS_* bits: OR over every env of every step since
        the last clear (waits for the device)."""
        self.join()
        return self.ctx.status(clear)

    def record(self, event, group: int = 0):
        """Record `event` on the stream group `group` is stepped on (the current
        stream for groups=1): HIP-event timing of that group's launches."""
        event.record(self._streams[group] if self._streams else torch.cuda.current_stream(self.device))

    def join(self):
        """Make the current stream wait for every group's queued steps (no-op for groups=1)."""
        if self._streams:
            self._plans[False].join(self._stream())
        self._held.clear()

    def reset(self, seed=None, env_mask=None):
        self.join()
        if seed is not None:
            self.set_seed(range(int(seed), int(seed) + self.num_envs))
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=self.device).to(torch.uint8).contiguous()
        self.ctx.reset(self.num_envs, _ptr(self.board), _ptr(self.rng), _ptr(self.timer), _ptr(self.eff),
                       _ptr(m), self._stream(), self._oh(0), self._oh_code)
        self._eff_valid = True
        return self._obs(), {"effective_bits": self.eff}

    def step(self, actions):
        a = torch.as_tensor(actions, device=self.device)
        if a.dtype != torch.int32:
            a = a.to(torch.int32)
        a = a.contiguous()
        if a.shape != (self.num_envs,):
            raise ValueError(f"actions must have shape ({self.num_envs},)")
        self.step_raw(a)
        self.join()
        flags = self.flags
        info = {
            "is_combination_match": (flags & _native.FLAG_COMBO) != 0,
            "num_new_specials": self.n_new,
            "num_specials_activated": self.n_act,
            "shuffled": (flags & _native.FLAG_SHUFFLED) != 0,
            "effective_bits": self.eff,
            "error": (flags & _native.FLAG_ERROR) != 0,
            "overflow": (flags & _native.FLAG_OVERFLOW) != 0,
        }
        done = (flags & _native.FLAG_DONE) != 0
        return self._obs(), self.reward, done, torch.zeros_like(done), info

    def step_raw(self, actions_i32: torch.Tensor, fork: bool = True):
        """Enqueue one batched step (no output post-processing): the bench path.
        actions_i32: contiguous int32 (N,) on the device.  With groups > 1 call
        join() before reading results.  One host call (tmg_plan_step) enqueues
        every group's launches; the actions tensor is held until join().
        fork=False: nothing queued on the current stream since the previous
        step is read by this one (e.g. actions staged beforehand), so the group
        streams need not wait for it (saves the fork event per step)."""
        self._plans[False].step(actions_i32.data_ptr(), 0, int(self._eff_valid), self._stream(), int(fork))
        self._eff_valid = True
        if self._streams:
            self._held.append(actions_i32)
            if len(self._held) > 256:
                self.join()

    def step_effective(self, t: int, key: int = 12345, first_env: int = 0, fork: bool = True):
        """Enqueue one step of the examples' policy (src/examples/q_learning.py:19-25):
        every env takes an action drawn uniformly from its effective actions
        (tmg_sample_effective's draw, counter-based in (key, first_env + env, t),
        so a shard passing its global offset as first_env picks the same actions
        as the unsharded batch), sampled by the step kernel itself from the mask
        it reads anyway.  The sampled actions stay in self.actions."""
        # a mask from tmg_effective (hand-edited boards) may sit beside a line
        # on the board, so that step runs untrusted (tmg.h, trust_eff)
        trust = int(self._eff_valid)
        if not self._eff_valid:
            self.compute_effective()
        if self.actions is None:
            self.actions = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        if self._policy != (int(key), int(first_env)):
            self.join()
            self._policy = (int(key), int(first_env))
            self._configure()
        self._plans[True].step(self.actions.data_ptr(), int(t), trust, self._stream(), int(fork))
        self._eff_valid = True

    _PEEK_OUTPUTS = {"reward": torch.int32, "n_new": torch.int32, "n_act": torch.int32, "flags": torch.uint8}

    def peek(self, rng=None, outputs=("reward",), best: bool = False, seed=None, first_env: int = 0) -> dict:
        """What a step with each action would report, for all A actions of every
        env at once, without changing any state (tmg_peek): Board.move on a copy
        of each board.  outputs: any of "reward", "n_new", "n_act" ((N, A)
        int32) and "flags" ((N, A) uint8: FLAG_COMBO | FLAG_SHUFFLED |
        FLAG_ERROR); best=True adds "best_action" / "best_reward" ((N,) int32:
        the lowest action of maximal reward).  Ineffective actions give zeros.
        rng=None simulates with the envs' own RNG streams, i.e. exactly what the
        next step will return; an (N, 5) int64 device tensor of other PCG64
        words gives a sampled lookahead that does not see the env's real
        refills; seed=E (instead of rng) draws such words on the device,
        fresh_rng(1, E, first_env)[0].  Joins, then enqueues on the current
        stream; the returned tensors are reused by the next call."""
        self.join()
        for name in outputs:
            if name not in self._PEEK_OUTPUTS:
                raise ValueError(f"unknown peek output {name!r}")
        if rng is not None and seed is not None:
            raise ValueError("pass rng or seed, not both")
        if seed is not None:
            rng = self.fresh_rng(1, seed, first_env)[0]
        elif rng is None:
            rng = self.rng
        elif rng.shape != (self.num_envs, 5) or rng.dtype != torch.int64 or rng.device != self.board.device \
                or not rng.is_contiguous():
            raise ValueError(f"rng must be a contiguous ({self.num_envs}, 5) int64 tensor on {self.board.device}")
        bufs = self._peek_bufs
        names = list(outputs) + (["best_action", "best_reward"] if best else [])
        for name in names:
            if name not in bufs:
                shape = (self.num_envs, self.num_actions) if name in self._PEEK_OUTPUTS else (self.num_envs,)
                bufs[name] = torch.zeros(shape, dtype=self._PEEK_OUTPUTS.get(name, torch.int32), device=self.device)
        p = {name: _ptr(bufs[name]) if name in names else None
             for name in ("reward", "n_new", "n_act", "flags", "best_action", "best_reward")}
        self.ctx.peek(self.num_envs, _ptr(self.board), _ptr(rng), _ptr(self.eff), int(self._eff_valid), p["reward"],
                      p["n_new"], p["n_act"], p["flags"], p["best_action"], p["best_reward"], self._stream())
        return {name: bufs[name] for name in names}

    def step_greedy(self, rng=None, fork: bool = True):
        """Enqueue one step of the greedy policy: every env takes its lowest
        action of maximal one-ply reward (peek(best=True) into self.actions; an
        env with no effective action takes action 0).  rng as for peek: None
        is the oracle-greedy policy, other words the fair sampled one.  Returns
        the peeked best reward (N,) int32."""
        out = self.peek(rng=rng, outputs=(), best=True)
        if self.actions is None:
            self.actions = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.actions.copy_(out["best_action"])
        self.step_raw(self.actions, fork=fork)
        return out["best_reward"]

    _ROLL_OUTPUTS = {"ret": torch.int32, "plies": torch.int32, "flags": torch.uint8, "total": torch.int32}

    def rollout(self, depth: int, samples: int = 1, rng=None, key: int = 12345, first_env: int = 0, t: int = 0,
                horizon: bool = True, outputs=("ret",), best: bool = False, seed=None) -> dict:
        """Policy rollouts of every action of every env, without changing any
        state (tmg_rollout): rollout (s, i, a) plays action a on a copy of
        board i with the RNG words rng[s, i], then continues with the examples'
        policy (uniform over the effective actions: step_effective's draw with
        key (key + s * A + a) mod 2^64, global env first_env + i and step
        counter t + d at ply d) for min(depth, moves left) plies in all
        (horizon=False: depth plies whatever the timer says).  outputs: any of
        "ret" (the summed rewards), "plies" ((S, N, A) int32), "flags" ((S, N,
        A) uint8: the OR of the plies' FLAG_COMBO | FLAG_SHUFFLED | FLAG_ERROR)
        and "total" ((N, A) int32: ret summed over the samples); best=True adds
        "best_action" / "best_total" ((N,) int32: the lowest action of maximal
        total).  Ineffective actions and finished envs give zeros.  rng=None
        (samples == 1 only) simulates with the envs' own RNG streams, i.e. with
        the refills the env will really draw; otherwise a contiguous (S, N, 5)
        int64 device tensor of PCG64 words ((N, 5) for S = 1), or seed=E for
        fresh words drawn on the device, fresh_rng(samples, E, first_env): an
        honest sampled lookahead with a new E per decision.  Joins, then
        enqueues on the current stream; the returned tensors are reused by the
        next call of the same samples."""
        self.join()
        depth, samples = int(depth), int(samples)
        if depth < 1:
            raise ValueError("rollout depth must be >= 1")
        if samples < 1:
            raise ValueError("rollout samples must be >= 1")
        for name in outputs:
            if name not in self._ROLL_OUTPUTS:
                raise ValueError(f"unknown rollout output {name!r}")
        N, A = self.num_envs, self.num_actions
        if rng is not None and seed is not None:
            raise ValueError("pass rng or seed, not both")
        if seed is not None:
            rng = self.fresh_rng(samples, seed, first_env)
        elif rng is None:
            if samples != 1:
                raise ValueError("rng=None (the envs' own streams) needs samples == 1: pass (S, N, 5) words")
            rng = self.rng
        else:
            ok = (N, 5) if samples == 1 else None
            if (tuple(rng.shape) != (samples, N, 5) and tuple(rng.shape) != ok) or rng.dtype != torch.int64 \
                    or rng.device != self.board.device or not rng.is_contiguous():
                raise ValueError(f"rng must be a contiguous ({samples}, {N}, 5) int64 tensor on {self.board.device}")
        names = list(outputs) + (["best_action", "best_total"] if best else [])
        # the sums over the samples are taken from ret
        need = set(names) | ({"ret"} if best or "total" in names else set())
        bufs = self._roll_bufs.setdefault(samples, {})
        for name in need:
            if name not in bufs:
                shape = (samples, N, A) if name in ("ret", "plies", "flags") else (N, A) if name == "total" else (N,)
                bufs[name] = torch.zeros(shape, dtype=self._ROLL_OUTPUTS.get(name, torch.int32), device=self.device)
        p = {name: _ptr(bufs[name]) if name in need else None
             for name in ("ret", "plies", "flags", "total", "best_action", "best_total")}
        self.ctx.rollout(N, _ptr(self.board), _ptr(rng), _ptr(self.timer) if horizon else None, _ptr(self.eff),
                         int(self._eff_valid), depth, samples, key, first_env, t, p["ret"], p["plies"], p["flags"],
                         p["total"], p["best_action"], p["best_total"], self._stream())
        return {name: bufs[name] for name in names}

    def step_rollout_greedy(self, depth: int, samples: int = 1, rng=None, key: int = 12345, first_env: int = 0,
                            t: int = 0, horizon: bool = True, fork: bool = True, seed=None):
        """Enqueue one step of the rollout-greedy policy: every env takes its
        lowest action of maximal summed rollout return (rollout(best=True) into
        self.actions; an env with no effective action takes action 0).
        Arguments as for rollout.  Returns that best total (N,) int32."""
        out = self.rollout(depth, samples, rng=rng, key=key, first_env=first_env, t=t, horizon=horizon, outputs=(),
                           best=True, seed=seed)
        if self.actions is None:
            self.actions = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.actions.copy_(out["best_action"])
        self.step_raw(self.actions, fork=fork)
        return out["best_total"]

    _PLAY_OUTPUTS = {"ret": torch.int32, "n_new": torch.int32, "n_act": torch.int32, "plies": torch.int32,
                     "flags": torch.uint8, "ply_reward": torch.int32}

    def playout(self, actions, rng=None, seed=None, outputs=("ret",), best: bool = False, final: bool = False,
                horizon: bool = True, first_env: int = 0) -> dict:
        """Play given action sequences on copies of every env, without changing
        any state (tmg_playout): row (q, i) is exactly what successive
        step_raw calls (autoreset off) with actions[q, i, 0], [q, i, 1], ...
        leave and report on a copy of env i.  actions: a (Q, N, D) int32 device
        tensor ((N, D): Q = 1).  An ineffective action is a move like any other
        (reward 0, nothing changes but the timer); a negative action ends its
        sequence quietly (padding); an action >= A sets FLAG_ERROR, stops the
        sequence before that ply and raises STATUS_CALLER.  A sequence plays at
        most min(D, moves left) plies (horizon=False: D plies whatever the timer
        says; not with final=True) and carries FLAG_DONE when it ends the
        episode.  outputs: any of "ret", "n_new", "n_act" (the sums over the
        plies), "plies" ((Q, N) int32), "flags" ((Q, N) uint8: the OR of the
        plies' flags, plus FLAG_DONE) and "ply_reward" ((Q, N, D) int32);
        best=True adds "best_seq" / "best_ret" ((N,) int32: the lowest q of
        maximal ret).  rng=None plays with the envs' own RNG words (shared by
        all sequences of an env), i.e. with the refills the env will really
        draw; an (N, 5) int64 device tensor of other PCG64 words is shared the
        same way, a (Q, N, 5) tensor gives each sequence its own; seed=E draws
        fresh_rng(Q, E, first_env).  final=True adds "env": a TileMatchVecEnv
        over the Q * N final states (row q * N + i; autoreset mode "none", mask
        cache valid, this env's context: close this env last), to peek, roll
        out, step, expand or play out again.  Joins, then enqueues on the
        current stream; the output tensors are fresh ones."""
        self.join()
        N, dev = self.num_envs, self.board.device
        if actions.dim() == 2:
            actions = actions.unsqueeze(0)
        if actions.dim() != 3 or actions.shape[1] != N or actions.dtype != torch.int32 or actions.device != dev \
                or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous (Q, {N}, D) int32 tensor on {dev}")
        Q, D = int(actions.shape[0]), int(actions.shape[2])
        if Q < 1 or D < 1:
            raise ValueError("playout needs >= 1 sequence of >= 1 action")
        for name in outputs:
            if name not in self._PLAY_OUTPUTS:
                raise ValueError(f"unknown playout output {name!r}")
        if final and not horizon:
            raise ValueError("final=True needs the horizon (the final timers follow the envs')")
        if rng is not None and seed is not None:
            raise ValueError("pass rng or seed, not both")
        if seed is not None:
            rng = self.fresh_rng(Q, seed, first_env)
        elif rng is None:
            rng = self.rng
        elif tuple(rng.shape) not in ((N, 5), (Q, N, 5)) or rng.dtype != torch.int64 or rng.device != dev \
                or not rng.is_contiguous():
            raise ValueError(f"rng must be a contiguous ({N}, 5) or ({Q}, {N}, 5) int64 tensor on {dev}")
        per_seq = rng.dim() == 3
        kw = dict(device=dev)
        names = list(outputs) + (["best_seq", "best_ret"] if best else [])
        need = set(names) | ({"ret"} if best else set())
        bufs = {}
        for name in need:
            shape = (Q, N, D) if name == "ply_reward" else (N,) if name.startswith("best_") else (Q, N)
            bufs[name] = torch.empty(shape, dtype=self._PLAY_OUTPUTS.get(name, torch.int32), **kw)
        fb = fr = ft = fe = None
        if final:
            fb = torch.empty((Q * N, 2, self.num_rows, self.num_cols), dtype=torch.int8, **kw)
            fr = torch.empty((Q * N, 5), dtype=torch.int64, **kw)
            ft = torch.empty(Q * N, dtype=torch.int32, **kw)
            fe = torch.empty((Q * N, self.mask_words), dtype=torch.int64, **kw)
        p = {name: _ptr(bufs.get(name)) for name in ("ret", "n_new", "n_act", "plies", "flags", "ply_reward",
                                                      "best_seq", "best_ret")}
        self.ctx.playout(N, _ptr(self.board), _ptr(rng), per_seq, _ptr(self.timer) if horizon else None,
                         _ptr(self.eff), int(self._eff_valid), Q, D, _ptr(actions), p["ret"], p["n_new"], p["n_act"],
                         p["plies"], p["flags"], p["ply_reward"], _ptr(fb), _ptr(fr), _ptr(ft), _ptr(fe),
                         p["best_seq"], p["best_ret"], self._stream())
        out = {name: bufs[name] for name in names}
        if final:
            out["env"] = self._child_env(fb, fr, ft, fe)
        return out

    _TRACE_FIELDS = ("frames", "kind", "frame_elim", "n_frames", "reward", "n_new", "n_act", "flags", "out_rng")

    def trace(self, actions, stages=("clear", "fall", "refill"), max_frames: int = 16, stop: bool = False, rng=None,
              seed=None, frames: bool = True, first_env: int = 0) -> dict:
        """One move's cascade stage by stage, on copies of every env, without
        changing any state (tmg_trace): row (q, i) traces Board.move(actions[q,
        i]) on a copy of env i.  actions: an (N,) or (Q, N) int32 device tensor.
        stages: the kinds to record, of "swap", "combo", "clear", "fall",
        "refill", "shuffle" (a move runs swap; combo, fall, refill when it is a
        combination; clear, fall, refill per cascade iteration; shuffle when the
        ensure-playable loop shuffled).  Returns "frames" ((Q, N, max_frames, 2,
        R, C) int8: the board after each recorded stage; None with
        frames=False), "kind" ((Q, N, max_frames) uint8, 0 past the last
        frame), "frame_elim" ((Q, N, max_frames) int32: the cells a combo or
        clear stage emptied), "n_frames", "reward", "n_new", "n_act" ((Q, N)
        int32), "flags" ((Q, N) uint8) and "out_rng" ((Q, N, 5) int64).
        stop=False: the move runs to its end, the sums and flags are peek's,
        n_frames counts every stage of the selected kinds (more than
        max_frames: the trace was cut) and out_rng holds the words after the
        move.  stop=True: a row ends right after its max_frames-th frame, with
        FLAG_STOPPED and the sums, flags and words of the stages run so far.
        Frame boards past min(n_frames, max_frames) are not written.  An
        ineffective or negative action gives zeros; an action >= A sets
        FLAG_ERROR and raises STATUS_CALLER.  rng and seed as for peek.  Joins,
        then enqueues on the current stream; the output tensors are fresh
        ones (frames costs Q * N * max_frames * 2RC bytes)."""
        self.join()
        N, dev = self.num_envs, self.board.device
        if actions.dim() == 1:
            actions = actions.unsqueeze(0)
        if actions.dim() != 2 or actions.shape[1] != N or actions.dtype != torch.int32 or actions.device != dev \
                or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous ({N},) or (Q, {N}) int32 tensor on {dev}")
        Q, F = int(actions.shape[0]), int(max_frames)
        if Q < 1 or F < 1:
            raise ValueError("trace needs >= 1 action row and max_frames >= 1")
        codes = {name: code for code, name in _native.STAGE_NAMES.items()}
        mask = 0
        for name in stages:
            if name not in codes:
                raise ValueError(f"unknown trace stage {name!r}")
            mask |= 1 << codes[name]
        if not mask:
            raise ValueError("trace needs at least one stage")
        if rng is not None and seed is not None:
            raise ValueError("pass rng or seed, not both")
        if seed is not None:
            rng = self.fresh_rng(1, seed, first_env)[0]
        elif rng is None:
            rng = self.rng
        elif rng.shape != (N, 5) or rng.dtype != torch.int64 or rng.device != dev or not rng.is_contiguous():
            raise ValueError(f"rng must be a contiguous ({N}, 5) int64 tensor on {dev}")
        kw = dict(device=dev)
        out = {"frames": torch.empty((Q, N, F, 2, self.num_rows, self.num_cols), dtype=torch.int8, **kw) if frames
               else None,
               "kind": torch.empty((Q, N, F), dtype=torch.uint8, **kw),
               "frame_elim": torch.empty((Q, N, F), dtype=torch.int32, **kw),
               "flags": torch.empty((Q, N), dtype=torch.uint8, **kw),
               "out_rng": torch.empty((Q, N, 5), dtype=torch.int64, **kw)}
        for name in ("n_frames", "reward", "n_new", "n_act"):
            out[name] = torch.empty((Q, N), dtype=torch.int32, **kw)
        self.ctx.trace(N, _ptr(self.board), _ptr(rng), _ptr(self.eff), int(self._eff_valid), Q, _ptr(actions), mask, F,
                       bool(stop), *(_ptr(out[name]) for name in self._TRACE_FIELDS), self._stream())
        return out

    def afterstates(self, actions=None):
        """The afterstate of every traced action: the board at the end of the
        move's deterministic prefix (the swap, the first resolve, the first
        gravity), holes at the top and no draw made yet, which is what
        afterstate value functions and chance-node search work on.  actions: as
        for trace; None is every action, Q = A.  Returns (boards (Q, N, 2, R, C)
        int8, reward (Q, N) int32: the deterministic part of the move's reward,
        effective (Q, N) bool).  The board of an ineffective action is the
        env's own.  Costs Q * N * 2RC bytes: N * A * 2RC for every action."""
        N, A = self.num_envs, self.num_actions
        if actions is None:
            actions = torch.arange(A, dtype=torch.int32, device=self.board.device).unsqueeze(1).expand(A, N).contiguous()
        out = self.trace(actions, stages=("fall",), max_frames=1, stop=True)
        effective = out["n_frames"] > 0
        boards = torch.where(effective[:, :, None, None, None], out["frames"][:, :, 0], self.board.unsqueeze(0))
        return boards, out["reward"], effective

    def step_best_sequence(self, actions, rng=None, seed=None, horizon: bool = True, first_env: int = 0,
                           fork: bool = True):
        """Enqueue one step of the shooting planner: every env plays the first
        action of its best sequence, actions[best_seq[i], i, 0] (playout(best=
        True) into self.actions).  Every sequence must start with an action:
        a first action below 0 (padding only) would leave nothing to play and
        raises ValueError, checked on the host before anything is enqueued (one
        wait for the actions tensor).  Arguments as for playout.  Returns that
        best return (N,) int32."""
        if actions.dim() == 2:
            actions = actions.unsqueeze(0)
        if actions.dim() == 3 and actions.shape[2] > 0 and bool((actions[:, :, 0] < 0).any()):
            raise ValueError("step_best_sequence needs every sequence to start with an action (>= 0)")
        out = self.playout(actions, rng=rng, seed=seed, outputs=(), best=True, horizon=horizon, first_env=first_env)
        idx = out["best_seq"].to(torch.int64)
        first = actions[:, :, 0].gather(0, idx.unsqueeze(0))[0]
        if self.actions is None:
            self.actions = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.actions.copy_(first)
        self.step_raw(self.actions, fork=fork)
        return out["best_ret"]

    def expand(self, select=None, rng=None, max_children: int = None) -> "Expansion":
        """The successor states of every effective action of every env, without
        changing any state (tmg_expand_count + tmg_expand): one child per (env,
        effective action), env-major and by ascending action, each exactly what
        a step of that action (autoreset off) leaves and reports on a copy of
        the env.  The children are an env of their own, Expansion.env, to peek,
        roll out, step or expand again.
        select: an (N, A) bool tensor; only the effective actions it names are
        expanded (packed to mask words on the device).  rng as for peek: None
        gives the children the envs would really reach, an (N, 5) int64 device
        tensor of other PCG64 words sampled ones.  max_children: at most that
        many rows, the first ones.  A finished env (autoreset off) has no child.
        Joins, counts the children on the device, then reads the total: the one
        host wait of the call, needed to allocate exactly that many rows."""
        self.join()
        N, A, W = self.num_envs, self.num_actions, self.mask_words
        dev = self.board.device
        if rng is None:
            rng = self.rng
        elif rng.shape != (N, 5) or rng.dtype != torch.int64 or rng.device != dev or not rng.is_contiguous():
            raise ValueError(f"rng must be a contiguous ({N}, 5) int64 tensor on {dev}")
        sel = None
        if select is not None:
            select = torch.as_tensor(select, device=dev)
            if select.shape != (N, A) or select.dtype != torch.bool:
                raise ValueError(f"select must be a ({N}, {A}) bool tensor")
            bits = torch.zeros((N, W * 64), dtype=torch.int64, device=dev)
            bits[:, :A] = select
            sel = (bits.view(N, W, 64) << torch.arange(64, device=dev, dtype=torch.int64)).sum(dim=-1).contiguous()
        if max_children is not None and int(max_children) < 0:
            raise ValueError("max_children must be >= 0")
        # a mask from tmg_effective (hand-edited boards) may sit beside a line
        # on the board, so those moves run untrusted (tmg.h, trust_eff)
        trust = int(self._eff_valid)
        if not self._eff_valid:
            self.compute_effective()
        first = torch.empty(N + 1, dtype=torch.int64, device=dev)
        self.ctx.expand_count(N, _ptr(self.timer), _ptr(self.eff), _ptr(sel), _ptr(first), self._stream())
        total = int(first[N].item())                    # the host wait
        m = total if max_children is None else min(total, int(max_children))
        return self.expand_rows(first, m, rng, sel, trust)

    def expand_rows(self, first, m: int, rng, sel=None, trust: int = 1) -> "Expansion":
        """The second half of expand(): tmg_expand into m freshly allocated
        child rows placed by first, the (N + 1,) int64 device tensor
        tmg_expand_count wrote for this env's timers and masks (and sel, the
        (N, W) int64 select words, or None).  rng: the (N, 5) int64 words the
        moves draw from; trust: tmg_expand's trust_eff."""
        if m < 0:
            raise ValueError("m must be >= 0")
        if first.shape != (self.num_envs + 1,) or first.dtype != torch.int64 or first.device != self.board.device \
                or not first.is_contiguous():
            raise ValueError(f"first_child must be a contiguous ({self.num_envs + 1},) int64 tensor on the env's device")
        m = int(m)
        kw = dict(device=self.board.device)
        board = torch.empty((m, 2, self.num_rows, self.num_cols), dtype=torch.int8, **kw)
        crng = torch.empty((m, 5), dtype=torch.int64, **kw)
        timer = torch.empty(m, dtype=torch.int32, **kw)
        eff = torch.empty((m, self.mask_words), dtype=torch.int64, **kw)
        parent = torch.empty(m, dtype=torch.int64, **kw)
        action, reward, n_new, n_act = (torch.empty(m, dtype=torch.int32, **kw) for _ in range(4))
        flags = torch.empty(m, dtype=torch.uint8, **kw)
        env = None
        if m:
            self.ctx.expand(self.num_envs, _ptr(self.board), _ptr(rng), _ptr(self.timer), _ptr(self.eff), _ptr(sel),
                            trust, _ptr(first), m, _ptr(board), _ptr(crng), _ptr(timer), _ptr(eff), _ptr(parent),
                            _ptr(action), _ptr(reward), _ptr(n_new), _ptr(n_act), _ptr(flags), self._stream())
            env = self._child_env(board, crng, timer, eff)
        return Expansion(m, first, parent, action, reward, n_new, n_act, flags, env)

    def _child_env(self, board, rng, timer, eff) -> "TileMatchVecEnv":
        """An env over child tensors: this env's shape, colours, specials,
        num_moves and context, autoreset mode "none", the mask cache valid, no
        reset run, one env group."""
        env = object.__new__(TileMatchVecEnv)
        N = board.shape[0]
        env.device = self.device
        env.num_envs = N
        env.num_rows, env.num_cols, env.num_colours, env.num_moves = \
            self.num_rows, self.num_cols, self.num_colours, self.num_moves
        env.colourless_specials, env.colour_specials = list(self.colourless_specials), list(self.colour_specials)
        env.specials_mask = self.specials_mask
        env._autoreset_mode = "none"
        env.ctx = self.ctx                          # shared: the context holds no per-batch state
        env._owns_ctx = False
        env.num_actions, env.mask_words = self.num_actions, self.mask_words
        env._dev_index = self._dev_index
        env.board, env.rng, env.timer, env.eff = board, rng, timer, eff
        kw = dict(device=self.device)
        env.reward, env.n_new, env.n_act = (torch.zeros(N, dtype=torch.int32, **kw) for _ in range(3))
        env.flags = torch.zeros(N, dtype=torch.uint8, **kw)
        env.actions = None
        env._peek_bufs, env._roll_bufs = {}, {}
        env.onehot = None
        env._oh_code = _native.DTYPE_F32
        env._eff_valid = True
        env.groups = 1
        env._ranges = [(0, N)]
        env._streams = []
        env._plans = {pol: _native.Plan(env.ctx, N, _ptr(env.board), _ptr(env.rng), _ptr(env.timer), _ptr(env.reward),
                                        _ptr(env.n_new), _ptr(env.n_act), _ptr(env.flags), _ptr(env.eff), [0, N], [0])
                      for pol in (False, True)}
        env._policy = (12345, 0)
        env._vout = {}
        env._held = []
        env._configure()
        return env

    def capture_steps(self, actions=None, ts=None, policy: bool = False, key: int = 12345, first_env: int = 0):
        """Capture len(ts) batched steps into a HIP graph (tmg_plan_capture):
        run_graph() then enqueues all of them with one host call, the env
        groups still overlapping across the steps.  actions: a list of (N,)
        int32 device tensors, one per step (kept alive by the graph), or
        policy=True for the in-kernel effective-action policy (step counters
        ts).  Nothing runs at capture time; the graph assumes the state it is
        replayed on has this library's own masks (run it right after steps,
        resets or other graphs of this env)."""
        ts = list(range(len(actions))) if ts is None else [int(t) for t in ts]
        self.join()
        if policy:
            if self.actions is None:
                self.actions = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            if self._policy != (int(key), int(first_env)):
                self._policy = (int(key), int(first_env))
                self._configure()
            ptrs = [self.actions.data_ptr()] * len(ts)
        else:
            if len(actions) != len(ts):
                raise ValueError("one action tensor per step")
            ptrs = [a.data_ptr() for a in actions]
        side = torch.cuda.Stream(self.device)          # the NULL stream cannot be captured
        side.wait_stream(torch.cuda.current_stream(self.device))
        g = self._plans[bool(policy)].capture(ptrs, ts, int(self._eff_valid), side.cuda_stream)
        g.refs = (actions, side)
        return g

    def run_graph(self, graph):
        """Enqueue a captured run of steps (capture_steps) on the current stream."""
        graph.launch(self._stream())
        self._eff_valid = True

    def invalidate_effective_cache(self):
        """Call after editing self.board by hand."""
        self._eff_valid = False

    def compute_effective(self):
        self.join()
        self.ctx.effective(self.num_envs, _ptr(self.board), _ptr(self.eff), self._stream())
        return self.eff

    def effective_mask(self) -> torch.Tensor:
        """(N, A) bool mask of effective actions, unpacked from the bitmask."""
        self.join()
        bits = torch.arange(64, device=self.device, dtype=torch.int64)
        m = ((self.eff.unsqueeze(-1) >> bits) & 1).reshape(self.num_envs, -1)[:, :self.num_actions]
        return m.bool()

    # ------------------------------------------------------ fused one-hot
    def attach_onehot(self, dtype=torch.float32) -> torch.Tensor:
        """Keep OneHotWrapper planes (wrappers.py:56-69) of every board in a
        (N, channels, R, C) tensor that the step / reset kernels update in
        their own write-back (tmg_step_onehot): only boards a step changes are
        rewritten.  Encodes the current boards once (tmg_onehot); returns the
        tensor (also self.onehot).  Call refresh_onehot() after editing boards
        by hand with a trusted mask."""
        codes = {torch.float32: _native.DTYPE_F32, torch.uint8: _native.DTYPE_U8, torch.int32: _native.DTYPE_I32}
        if dtype not in codes:
            raise ValueError(f"dtype must be one of {list(codes)}")
        self.join()
        ch = self.ctx.onehot_channels()
        self.onehot = torch.zeros((self.num_envs, ch, self.num_rows, self.num_cols), dtype=dtype, device=self.device)
        self._oh_code = codes[dtype]
        self.refresh_onehot()
        self._configure()
        return self.onehot

    def refresh_onehot(self):
        self.join()
        self.ctx.onehot(self.num_envs, self.board.data_ptr(), self.onehot.data_ptr(), self._oh_code, self._stream())

    def _oh(self, lo):
        if self.onehot is None:
            return None
        return self.onehot.data_ptr() + lo * self.onehot[0].numel() * self.onehot.element_size()

    def _obs(self):
        return {"board": self.board, "num_moves_left": self.num_moves - self.timer}

    def rng_words(self) -> np.ndarray:
        self.join()
        return self.rng.cpu().numpy().view(np.uint64)

    # ------------------------------------------------------- checkpoint/restore
    def config(self) -> dict:
        return {"num_rows": self.num_rows, "num_cols": self.num_cols, "num_colours": self.num_colours,
                "num_moves": self.num_moves, "colourless_specials": self.colourless_specials,
                "colour_specials": self.colour_specials, "num_envs": self.num_envs, "autoreset": self.autoreset,
                "autoreset_mode": self._autoreset_mode}

    def state_dict(self) -> dict:
        """Host copy of the whole batched state: boards, the exact PCG64 stream
        position of every env (incl. numpy's buffered half-word), timers and the
        effective-action masks; restoring it continues every trajectory
        bit-exactly."""
        self.join()
        torch.cuda.synchronize(self.device)
        return {"board": self.board.cpu().numpy(), "rng": self.rng_words().copy(),
                "timer": self.timer.cpu().numpy(), "eff": self.eff.cpu().numpy().view(np.uint64).copy(),
                "eff_valid": self._eff_valid, "config": self.config()}

    def load_state_dict(self, sd: dict) -> None:
        cfg = sd["config"]
        mine = self.config()
        def norm(v):
            return list(v) if isinstance(v, (list, tuple)) else v

        for k in ("num_rows", "num_cols", "num_colours", "num_moves", "colourless_specials", "colour_specials",
                  "num_envs"):
            if norm(cfg[k]) != norm(mine[k]):
                raise ValueError(f"checkpoint {k}={cfg[k]!r} does not match this env ({mine[k]!r})")
        self.board.copy_(torch.from_numpy(np.ascontiguousarray(sd["board"], dtype=np.int8)))
        self.rng.copy_(torch.from_numpy(np.ascontiguousarray(sd["rng"], dtype=np.uint64).view(np.int64)))
        self.timer.copy_(torch.from_numpy(np.ascontiguousarray(sd["timer"], dtype=np.int32)))
        self.eff.copy_(torch.from_numpy(np.ascontiguousarray(sd["eff"], dtype=np.uint64).view(np.int64)))
        self._eff_valid = bool(sd.get("eff_valid", True))

    def save(self, path) -> None:
        sd = self.state_dict()
        cfg = dict(sd["config"], eff_valid=sd["eff_valid"])
        save_state(path, sd, cfg)

    @classmethod
    def load(cls, path, device=None) -> "TileMatchVecEnv":
        arrays, cfg = load_state(path)
        env = cls(cfg["num_envs"], cfg["num_rows"], cfg["num_cols"], cfg["num_colours"], cfg["num_moves"],
                  cfg["colourless_specials"], cfg["colour_specials"], seeds=range(cfg["num_envs"]), device=device,
                  autoreset=cfg["autoreset"])
        # next-step mode: the pending resets are implicit in timer == num_moves,
        # so the mode must come back with the state (older checkpoints: the bool)
        mode = cfg.get("autoreset_mode")
        if mode is not None and mode != env._autoreset_mode:
            env._autoreset_mode = mode
            env._configure()
        env.load_state_dict(dict(arrays, config=cfg, eff_valid=cfg.get("eff_valid", True)))
        return env

    def close(self):
        self.join()
        for plan in self._plans.values():
            plan.close()
        if getattr(self, "_owns_ctx", True):           # an Expansion's env shares its parent's context
            self.ctx.close()
