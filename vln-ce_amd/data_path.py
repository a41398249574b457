"""Cached-feature DAgger data path on the device.

Upstream, `collate_fn` (dagger_trainer.py:39-114) pads every trajectory of a batch to the
longest one on the host (observations with 1.0, actions / weights with 0), interleaves them
time-major (row t*B + b), and the train loop then copies the padded tensors to the GPU casting
every sensor to fp32 (:559-583); the inflection weights come from
IWTrajectoryDataset.__next__ (:196-208) and the length-bucketed ordering from _load_next
(:174-184).  Here the host only concatenates the RAGGED rows (pinned, in the storage dtype --
fp16 if the LMDB cache was written with IL.DAGGER.lmdb_fp16) and ships them once; padding,
interleave, widening, inflection weights and masks are one kernel pass per sensor on the GPU.
The returned 5-tuple is what `_update_agent` takes, already on the device.
"""
import random

import torch

from . import ops


_STAGE = {}         # slot -> pinned uint8 buffer
_STAGE_EVENTS = {}  # slot -> event recorded after the last H2D copy out of that buffer


def _staging(slot, dtype, shape):
    n = 1
    for s in shape:
        n *= s
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    ev = _STAGE_EVENTS.get(slot)
    if ev is not None:
        ev.synchronize()
    buf = _STAGE.get(slot)
    if buf is None or buf.numel() < nbytes:
        buf = _STAGE[slot] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
    return buf[:nbytes].view(dtype).view(shape)


def inflection_weights_host(oracle_actions, coef):
    """reference values on the host (used by tests and by callers that stay on the CPU path)."""
    infl = torch.ones_like(oracle_actions, dtype=torch.bool)
    infl[1:] = oracle_actions[1:] != oracle_actions[:-1]
    return torch.where(infl, torch.tensor(float(coef)), torch.tensor(1.0))


def bucketed_order(lengths, batch_size, rng=random):
    """order in which IWTrajectoryDataset._load_next hands out a preload chunk: sort by
    (length, random tie-break), shuffle blocks of `batch_size`, consumed from the END (.pop())."""
    n = len(lengths)
    prio = list(range(n))
    rng.shuffle(prio)
    order = sorted(range(n), key=lambda k: (lengths[k], prio[k]))
    blocks = [order[i:i + batch_size] for i in range(0, n, batch_size)]
    rng.shuffle(blocks)
    flat = [k for blk in blocks for k in blk]
    return flat[::-1]


def collate_trajectories(batch, device, inflection_coef=1.0, pin=True):
    """batch: list of (obs dict of [T_b, ...] tensors / arrays, prev_actions [T_b],
    oracle_actions [T_b]) as stored in the LMDB feature cache.  Returns
    (observations {sensor: [Tmax*B, ...] fp32}, prev_actions [Tmax*B, 1] int64,
     not_done_masks [Tmax*B, 1] uint8, corrected_actions [Tmax, B] int64, weights [Tmax, B] fp32)
    on `device`."""
    lib = ops.L()
    B = len(batch)
    lens = [int(torch.as_tensor(tr[1]).shape[0]) for tr in batch]
    Tmax = max(lens)
    off = torch.zeros(B + 1, dtype=torch.int32)
    off[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)

    use_pinned = pin and str(device) != "cpu" and torch.cuda.is_available()

    def ship(parts, slot):
        parts = [torch.as_tensor(p) for p in parts]
        if not use_pinned:
            return torch.cat(parts, dim=0).contiguous().to(device)
        # rows go straight into a persistent pinned staging buffer (one per slot, grown on
        # demand), then one asynchronous H2D copy; the buffer is reused by the next batch only
        # after that copy has completed
        shape = (sum(p.shape[0] for p in parts),) + tuple(parts[0].shape[1:])
        stage = _staging(slot, parts[0].dtype, shape)
        row = 0
        for p in parts:
            stage[row:row + p.shape[0]].copy_(p)
            row += p.shape[0]
        out = stage.to(device, non_blocking=True)
        _STAGE_EVENTS[slot] = torch.cuda.Event()
        _STAGE_EVENTS[slot].record()
        return out

    off_d = off.to(device, non_blocking=True)
    observations = {}
    for sensor in batch[0][0]:
        rows = ship([tr[0][sensor] for tr in batch], "obs/" + sensor)
        if rows.dtype not in (torch.float32, torch.float16, torch.int64):
            rows = rows.to(torch.int64 if not rows.is_floating_point() else torch.float32)
        tail = tuple(rows.shape[1:])
        D = 1
        for s in tail:
            D *= s
        dst = torch.empty((Tmax * B,) + tail, device=device, dtype=torch.float32)
        lib.ragged_pad_rows(rows, off_d, B, Tmax, D, 1.0, dst)  # observations pad = 1.0 (:77)
        observations[sensor] = dst
    prev = ship([torch.as_tensor(tr[1]).to(torch.int64) for tr in batch], "prev")
    prev_out = torch.empty((Tmax * B, 1), device=device, dtype=torch.int64)
    lib.ragged_pad_rows_i64(prev, off_d, B, Tmax, 1, 0, prev_out)
    oracle = ship([torch.as_tensor(tr[2]).to(torch.int64) for tr in batch], "oracle")
    corrected = torch.empty((Tmax, B), device=device, dtype=torch.int64)
    weights = torch.empty((Tmax, B), device=device, dtype=torch.float32)
    masks = torch.empty((Tmax * B, 1), device=device, dtype=torch.uint8)
    lib.dagger_targets(oracle, off_d, B, Tmax, inflection_coef, corrected, weights, masks)
    return observations, prev_out, masks, corrected, weights


# ---- the write half: rollout collection (dagger_trainer.py:248-467) ------------------------------
def _on_gpu(device):
    return torch.device(device).type == "cuda"


# arena keys of the two action columns (tuples: no observation key can collide with them)
_PREV, _ORACLE = ("prev_actions",), ("oracle_actions",)


class TrajectoryRecorder:
    """Device-side episode buffers for `DaggerTrainer._update_dataset`.

    The reference keeps `episodes[i]`, a host list of (observation row, prev_action,
    expert_action) per environment: the cached trunk outputs reach it through `o.cpu()` forward
    hooks (:294-314), the actions through `.item()` per environment (:429-435), and a finished
    episode is re-stacked by `batch_obs(..., cpu)` and narrowed with `astype(np.float16)`
    (:341-356).  Here every recorded sensor has an arena [num_envs, capacity, D] on the device in
    its storage dtype (float16 for every observation sensor when `fp16` -- IL.DAGGER.lmdb_fp16 --
    else float32, which is what batch_obs's cast to float leaves; int64 for the two action
    columns); `append` is ONE launch per step, `pop` one D2H per sensor and one synchronisation
    per call.  The per-environment lengths are host integers: nothing is read back to learn them.

    Environments are addressed by their ACTIVE position, the `i` of the reference's loops;
    `pause` removes positions exactly as `_pause_envs` does, and the rows of later calls map to
    the surviving environments.

    exclude: observation keys that are never stored (the expert-action sensor: `del
    traj_obs[expert_uuid]`, :346).  A hooked feature `<sensor>_features` replaces the observation
    `<sensor>` (:421-427); popped dicts list the remaining observations in their own order, then
    the hooked features in the order their hooks were made.
    """

    def __init__(self, num_envs, device, fp16, capacity=128, exclude=()):
        self.num_envs, self.device = int(num_envs), torch.device(device)
        self.fp16, self.capacity = bool(fp16), int(capacity)
        assert self.num_envs > 0 and self.capacity > 0
        self.exclude = set(exclude)
        self._active = list(range(self.num_envs))   # active position -> arena slot
        self._len = [0] * self.num_envs             # per slot
        # name -> (last module output, (the stream it was made on, an event there if that is a side
        # stream)); None: consumed
        self._hooked = {}
        self._names = None                          # recorded sensors, fixed by the first append
        self._shapes = {}
        self._arenas = {}
        self._stage = None                          # pinned D2H staging of pop()

    # -- hooks
    def feature_hook(self, name):
        """forward hook for a trunk whose output is cached under `name`: keeps a reference to the
        output where it is (no copy, no synchronisation); the next append() records it"""
        self._hooked.setdefault(name, None)
        events = {}   # side stream -> the one event this hook re-records there

        def hook(module, inputs, output):
            # the trunk may be running ahead on a side stream (policy.encode_ahead): remember where,
            # so that append() orders its launch behind it whatever the caller did in between
            # (on the default stream, where append() is expected too, there is nothing to record)
            mark = None
            if output.is_cuda and not torch.cuda.is_current_stream_capturing():
                stream = torch.cuda.current_stream(output.device)
                mark = (stream, None)
                if stream != torch.cuda.default_stream(output.device):
                    if stream not in events:
                        events[stream] = torch.cuda.Event()
                    mark = (stream, events[stream])
                    mark[1].record(stream)
            self._hooked[name] = (output.detach(), mark)

        return hook

    # -- recording
    def _sources(self, observations):
        replaced = {n[:-len("_features")] for n in self._hooked if n.endswith("_features")}
        src = {k: v for k, v in observations.items()
               if k not in self.exclude and k not in replaced and k not in self._hooked}
        for name, out in self._hooked.items():
            if out is None:
                raise RuntimeError(f"TrajectoryRecorder: the hook of {name!r} has not fired since "
                                   "the last append()")
            tensor, mark = out
            if mark is not None:
                cur = torch.cuda.current_stream(tensor.device)
                if cur != mark[0]:
                    if mark[1] is not None:
                        cur.wait_event(mark[1])
                    else:
                        cur.wait_stream(mark[0])
                    tensor.record_stream(cur)
            src[name] = tensor
        return src

    def _alloc(self, capacity):
        odt = torch.float16 if self.fp16 else torch.float32
        out = {}
        for name in self._names:
            D = 1
            for s in self._shapes[name]:
                D *= s
            dt = torch.int64 if name in (_PREV, _ORACLE) else odt
            out[name] = torch.empty((self.num_envs, capacity, D), dtype=dt, device=self.device)
        return out

    def _grow(self, need):
        cap = self.capacity
        while cap < need:
            cap *= 2
        new = self._alloc(cap)
        used = max(self._len)
        if used:
            for name, arena in self._arenas.items():
                new[name][:, :used].copy_(arena[:, :used])
        self._arenas, self.capacity = new, cap

    def append(self, observations, prev_actions, oracle_actions):
        """one step of every active environment: row i of every tensor belongs to active
        position i.  prev_actions / oracle_actions: [n] or [n, 1]."""
        n = len(self._active)
        if n == 0:
            return
        src = self._sources(observations)
        # (batch_obs leaves the expert sensor as float: the launch truncates it to int64, which is
        # what np.array([... .item()], dtype=np.int64) makes of it, :355)
        oracle = oracle_actions.reshape(-1)
        if oracle.dtype not in (torch.int64, torch.float32, torch.uint8):
            oracle = oracle.long()
        src[_PREV] = prev_actions.reshape(-1)
        src[_ORACLE] = oracle
        if self._names is None:
            self._names = list(src)
            self._shapes = {k: tuple(v.shape[1:]) for k, v in src.items()}
            self._arenas = self._alloc(self.capacity)
        if list(src) != self._names:
            raise RuntimeError(f"TrajectoryRecorder: sensors {[k for k in src if isinstance(k, str)]} "
                               "differ from the first append()'s")
        for k, v in src.items():
            if v.size(0) != n or tuple(v.shape[1:]) != self._shapes[k]:
                raise RuntimeError(f"TrajectoryRecorder: {k!r} has shape {tuple(v.shape)}, expected "
                                   f"{(n,) + self._shapes[k]}")
        steps = [self._len[s] for s in self._active]
        if max(steps) >= self.capacity:
            self._grow(max(steps) + 1)
        ops.L().traj_append([src[k] for k in self._names], [self._arenas[k] for k in self._names],
                            self._active, steps)
        for s in self._active:
            self._len[s] += 1
        for name in self._hooked:
            self._hooked[name] = None

    # -- episode ends
    def pop(self, env_indices):
        """[[obs dict of numpy arrays [T, ...], prev_actions int64 [T], oracle_actions int64 [T]]]
        for the given active positions, in the given order -- the reference's `transposed_ep`
        (:352-356).  The arrays own their memory; the environments' lengths reset to 0."""
        import numpy as np

        slots = [self._active[i] for i in env_indices]
        if not slots:
            return []
        if self._names is None:
            raise RuntimeError("TrajectoryRecorder.pop() before the first append()")
        jobs, nbytes = [], 0
        for slot in slots:
            T = self._len[slot]
            for name in self._names:
                arena = self._arenas[name]
                jobs.append((slot, name, T, nbytes))
                nbytes += -(-T * arena.size(2) * arena.element_size() // 16) * 16
        pinned = _on_gpu(self.device)
        if pinned and (self._stage is None or self._stage.numel() < nbytes):
            self._stage = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        parts = {}
        for slot, name, T, off in jobs:
            arena = self._arenas[name]
            rows = arena[slot, :T]   # contiguous slab
            if pinned:
                host = self._stage[off:off + rows.numel() * rows.element_size()].view(arena.dtype)
                host = host.view(rows.shape)
                host.copy_(rows, non_blocking=True)
            else:
                host = rows
            parts[(slot, name)] = host
        if pinned:
            torch.cuda.current_stream(self.device).synchronize()
        out = []
        for slot in slots:
            T = self._len[slot]
            arrays = {name: np.array(parts[(slot, name)].numpy().reshape((T,) + self._shapes[name]))
                      for name in self._names}
            prev, oracle = arrays.pop(_PREV), arrays.pop(_ORACLE)
            out.append([arrays, prev, oracle])
        for slot in slots:
            self._len[slot] = 0
        return out

    def discard(self, env_indices):
        """forget what the given active positions have recorded (`dones[i]` with `skips[i]`, and
        the reset at :385-386): no copy"""
        for i in env_indices:
            self._len[self._active[i]] = 0

    def pause(self, env_indices):
        """remove active positions as `_pause_envs` does (their rows stop arriving)"""
        for i in sorted(set(env_indices), reverse=True):
            self._len[self._active.pop(i)] = 0

    def lengths(self):
        """recorded steps per active position"""
        return [self._len[s] for s in self._active]


def dagger_step(actions, expert_actions, beta, prev_actions):
    """dagger_trainer.py:414-444 behind act(): the beta mix (same torch.rand_like draw as the
    reference, so the RNG stream is its), the skip rule for expert action -1 and
    prev_actions.copy_ in one launch, then ONE device-to-host copy.  Returns (the mixed actions on
    the device, shaped like `actions`; [int] for envs.step; [bool] skips).  prev_actions is
    updated in place."""
    n = actions.numel()
    uniform = torch.rand_like(actions, dtype=torch.float)
    expert = expert_actions.reshape(-1)
    if expert.dtype not in (torch.float32, torch.int64):
        expert = expert.long()
    stepped = torch.empty((2, n), dtype=torch.int64, device=actions.device)
    prev = prev_actions.view(-1)   # (a view: the kernel writes prev_actions itself)
    ops.L().dagger_mix_actions(actions.reshape(-1).contiguous(), expert.contiguous(),
                               uniform.reshape(-1), beta, prev, stepped)
    host = stepped.cpu()
    return stepped[0].view(actions.shape), host[0].tolist(), [bool(v) for v in host[1].tolist()]
