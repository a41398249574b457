"""vlnce_amd.ActionDictRolloutStorage (side A: one launch per insert / after_update / minibatch /
get_advantages) against a plain-torch restatement of the reference storage's per-call arithmetic
(side B: copy_ per field, a Python loop over the environments with stack / view per minibatch, a
mean() / std() chain), on one MI355X, same device, same arenas' shapes.

Full Waypoint size: num_steps 16, 8 environments, num_mini_batch 4 -- 32 rows x 13 frames, the
416-frame batch of `bench.py --policy waypoint` -- 224 px RGB, 256 px depth, the reference's six
sensors.  The sides alternate call by call and swap who goes first; medians of --reps calls.  Per
insert, per minibatch (a whole generator pass / num_mini_batch), per after_update and per
get_advantages:
  host      time inside the call, device idle before, not waited for after
  events    hipEvent before the call -> hipEvent after it (what the stream was busy or waiting)
  ops, sum  from one extra call under torch.profiler: device operations (kernels and copies) and
            the sum of their durations
For rollout_copy_kernel and rollout_gather_kernel: bytes moved (read + written) / kernel time, next
to the rate of one device-to-device Tensor.copy_ of the same byte count in the same run.

    python scripts/rollout_storage_ab.py [--reps 40] [--warmup 5] [--out profiles/rollout_storage_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vlnce_amd.rollout_storage import ActionDictRolloutStorage  # noqa: E402

DEV = "cuda:0"
T, N, MINI, L, H = 16, 8, 4, 2, 512
SENSORS = {"rgb": (12, 224, 224, 3), "depth": (12, 256, 256, 1), "rgb_history": (224, 224, 3),
           "depth_history": (256, 256, 1), "angle_features": (12, 4), "instruction": (200,)}
LINES = []


def say(msg=""):
    print(msg, flush=True)
    LINES.append(msg)


class TorchStorage(ActionDictRolloutStorage):
    """side B: the same arenas, moved the way the reference moves them -- one copy_ per field, and a
    minibatch assembled environment by environment"""

    def insert(self, observations, recurrent_hidden_states, action, action_log_probs, value_preds,
               rewards, masks):
        s = self.step
        for k, v in observations.items():
            self.observations[k][s + 1].copy_(v)
        self.recurrent_hidden_states[s + 1].copy_(recurrent_hidden_states)
        for k, v in action.items():
            self.actions[k][s].copy_(v)
            self.prev_actions[k][s + 1].copy_(v)
        self.action_log_probs[s].copy_(action_log_probs)
        self.value_preds[s].copy_(value_preds)
        self.rewards[s].copy_(rewards)
        self.masks[s + 1].copy_(masks)
        self.step = s + 1

    def after_update(self):
        s = self.step
        for a in list(self.observations.values()) + [self.recurrent_hidden_states, self.masks] \
                + list(self.prev_actions.values()):
            a[0].copy_(a[s])
        self.step = 0

    def get_advantages(self, use_normalized_advantage=False):
        adv = self.returns[:-1] - self.value_preds[:-1]
        return (adv - adv.mean()) / (adv.std() + 1e-5) if use_normalized_advantage else adv

    def recurrent_generator(self, advantages, num_mini_batch):
        n_envs = self.rewards.size(1)
        per = n_envs // num_mini_batch
        perm = torch.randperm(n_envs)
        Ts = self.step
        arenas = [*self.observations.values(), *self.actions.values(), *self.prev_actions.values(),
                  self.value_preds, self.returns, self.masks, self.action_log_probs, advantages]
        for start in range(0, n_envs, per):
            cols = [[] for _ in arenas]
            hidden = []
            for offset in range(per):
                ind = perm[start + offset]
                for col, a in zip(cols, arenas):
                    col.append(a[:Ts, ind])
                hidden.append(self.recurrent_hidden_states[0, ind])
            flat = [torch.stack(col, 1) for col in cols]
            flat = [x.view(Ts * per, *x.shape[2:]) for x in flat]
            it = iter(flat)
            obs = {k: next(it) for k in self.observations}
            actions = {k: next(it) for k in self.actions}
            prev = {k: next(it) for k in self.actions}
            yield (obs, torch.stack(hidden, 0), actions, prev, *it)


def step_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return dict(
        observations={k: torch.randn(N, *s, generator=g).to(DEV) for k, s in SENSORS.items()},
        recurrent_hidden_states=torch.randn(N, L, H, generator=g).to(DEV),
        action={"pano": torch.randint(0, 12, (N, 1), generator=g).to(DEV),
                "offset": torch.rand(N, 1, generator=g).to(DEV),
                "distance": torch.rand(N, 1, generator=g).to(DEV)},
        action_log_probs=-torch.rand(N, 1, generator=g).to(DEV),
        value_preds=torch.randn(N, 1, generator=g).to(DEV), rewards=torch.randn(N, 1, generator=g).to(DEV),
        masks=(torch.rand(N, 1, generator=g) > 0.1).float().to(DEV))


def measure(fn):
    """(host seconds, event seconds) of one call on an idle device"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    fn()
    host = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return host, a.elapsed_time(b) * 1e-3


def device_ops(fn):
    prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU,
                                              torch.profiler.ProfilerActivity.CUDA])
    torch.cuda.synchronize()
    prof.start()
    fn()
    torch.cuda.synchronize()
    prof.stop()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and not e.name.startswith("Memset")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    space = types.SimpleNamespace(spaces={k: types.SimpleNamespace(shape=s) for k, s in SENSORS.items()})
    sides = {"A vlnce_amd": ActionDictRolloutStorage(T, N, space, H, L, device=DEV),
             "B torch": TorchStorage(T, N, space, H, L, device=DEV)}
    inputs = [step_inputs(s) for s in range(2)]
    for st in sides.values():   # a full rollout in both, so that every row read holds data
        for s in range(T):
            st.insert(**inputs[s % 2])
        st.compute_returns(torch.zeros(N, 1, device=DEV), True, 0.99, 0.95)
    row_bytes = sum(a[0, 0].numel() * a.element_size() for st in [sides["A vlnce_amd"]]
                    for a, _ in st._batched)

    def op(name, st, rep):
        if name == "insert":
            st.step = rep % T
            return lambda: st.insert(**inputs[rep % 2])
        if name == "after_update":
            st.step = T
            return lambda: st.after_update()
        if name == "get_advantages":
            st.step = T
            return lambda: st.get_advantages(True)
        st.step = T
        adv = st.get_advantages(False)
        return lambda: [None for _ in st.recurrent_generator(adv, MINI)]

    say(f"# scripts/rollout_storage_ab.py: num_steps {T}, {N} environments, num_mini_batch {MINI}, "
        f"{torch.cuda.get_device_name(0)}; medians of {args.reps} calls, sides alternating")
    say(f"# one environment-step of every field: {row_bytes / 1e6:.2f} MB; arenas "
        f"{sum(a.numel() * a.element_size() for a, _ in sides['A vlnce_amd']._batched) / 1e9:.2f} GB per side")
    say(f"{'call':16s}{'side':14s}{'host us':>10s}{'events us':>11s}{'ops':>6s}{'sum of ops us':>15s}")
    for name, per in (("insert", 1), ("minibatch", MINI), ("after_update", 1), ("get_advantages", 1)):
        times = {side: [] for side in sides}
        for rep in range(-args.warmup, args.reps):
            order = list(sides) if rep % 2 == 0 else list(sides)[::-1]
            for side in order:
                host, ev = measure(op(name, sides[side], rep))
                if rep >= 0:
                    times[side].append((host, ev))
        for side, st in sides.items():
            events = device_ops(op(name, st, 0))
            total = sum(e.time_range.elapsed_us() for e in events)
            host =statistics.median(h for h, _ in times[side]) / per
            ev = statistics.median(e for _, e in times[side]) / per
            say(f"{name:16s}{side:14s}{host * 1e6:10.1f}{ev * 1e6:11.1f}{len(events) / per:6.1f}"
                f"{total / per:15.1f}")
    say()
    moved = {"insert": 2 * N * row_bytes, "minibatch": 2 * T * (N // MINI) * row_bytes}
    say("# bytes moved (read + written) / kernel time, and one device-to-device Tensor.copy_ of the same bytes")
    st = sides["A vlnce_amd"]
    for name, nbytes in moved.items():
        # the kernel and the copy_ alternate, so that neither finds its bytes in the 256 MB cache
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)
        dst = torch.empty_like(src)
        copies, kernels = [], []
        for rep in range(args.reps):
            events = device_ops(op(name, st, rep))
            kernels += [e.time_range.elapsed_us() for e in events if "rollout_" in e.name]
            events = device_ops(lambda: dst.copy_(src))
            copies.append(sum(e.time_range.elapsed_us() for e in events))
        c, k = statistics.median(copies), statistics.median(kernels)
        say(f"{name:12s} {nbytes / 1e6:8.1f} MB  kernel {k:8.1f} us {nbytes / k / 1e6:6.2f} TB/s   "
            f"copy_ {c:8.1f} us {nbytes / c / 1e6:6.2f} TB/s   ratio {c / k:.2f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
