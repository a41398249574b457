"""update_agent(fused_loss=True) -- the imitation-learning objective as one launch with its
gradient (vlnce_il_loss), the progress monitor's term as one more (vlnce_pair_mse), one read-back
-- against the default chain of torch ops, A/B in one process on one MI355X.

Two batches, one CMA policy and one Adam optimizer each, the two sides alternating step by step
(and alternating who goes first):
  1. the headline batch of bench.py: N = 64 environments, T = 1, 256x256 RGB-D, 80 tokens,
     progress monitor off;
  2. the cached-feature DAgger batch of scripts/bench_data_path.py: 5 episodes x 100 steps,
     PROGRESS_MONITOR.use = True (the [500, 500] loss matrix on the default side).
Per side: the median host wall time of a step (device idle before, synchronised after), and the
number of kernels the device ran between build_distribution() returning and backward() returning
-- the loss, its backward and the backward of the whole policy; the difference between the sides
is the loss chain -- counted in one extra step per side with torch.profiler, the window opened
and closed on a synchronised device.  Where the profiler reports no device activity the count is
the number of aten operators and library entry points issued from Python in that window instead.

    python scripts/il_loss_ab.py [--steps 40] [--warmup 6] [--out profiles/il_loss_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import vlnce_amd  # noqa: E402
from vlnce_amd import _lib, data_path, ops  # noqa: E402
from vlnce_amd.il_harness import update_agent  # noqa: E402

SIDES = ("default", "fused")
LINES = []


def say(msg=""):
    print(msg, flush=True)
    LINES.append(msg)


def headline_batch(dev, N=64, hw=256, L=80, seed=1):
    """bench.py's synth_batch"""
    g = torch.Generator().manual_seed(seed)
    obs = {"rgb": torch.randint(0, 256, (N, hw, hw, 3), generator=g).float(),
           "depth": torch.rand(N, hw, hw, 1, generator=g),
           "instruction": torch.zeros(N, 200, dtype=torch.long)}
    obs["instruction"][:, :L] = torch.randint(1, 2504, (N, L), generator=g)
    prev = torch.randint(0, 4, (N, 1), generator=g)
    masks = (torch.rand(N, 1, generator=g) > 0.1).to(torch.uint8)
    targets = torch.randint(0, 4, (1, N), generator=g)
    weights = torch.rand(1, N, generator=g) + 0.5
    return ({k: v.to(dev) for k, v in obs.items()}, prev.to(dev), masks.to(dev), targets.to(dev),
            weights.to(dev))


def cached_batch(dev, episodes=5, steps=100):
    """the batch of scripts/bench_data_path.py, with the progress targets of a real episode"""
    rng = np.random.RandomState(0)
    lens = [max(1, int(steps * f)) for f in np.linspace(1.0, 0.55, episodes)]
    trajs = []
    for T in lens:
        obs = {"rgb_features": rng.rand(T, 2048, 4, 4).astype(np.float16),
               "depth_features": rng.rand(T, 128, 4, 4).astype(np.float16),
               "instruction": np.tile(np.concatenate([rng.randint(1, 2504, size=80),
                                                      np.zeros(120, np.int64)])[None], (T, 1)),
               "progress": np.linspace(0.0, 1.0, T, dtype=np.float32)[:, None]}
        oracle = rng.randint(0, 4, size=T).astype(np.int64)
        trajs.append((obs, np.concatenate([[0], oracle[:-1]]).astype(np.int64), oracle))
    return data_path.collate_trajectories(trajs, dev, inflection_coef=3.2), lens


class IssueCount(TorchDispatchMode):
    """aten operators dispatched while the mode is on (the autograd engine carries it to its
    worker threads)"""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


class Window:
    """opens when policy.build_distribution returns, closes in update_agent's grad_hook, which
    runs right after loss.backward() returned"""

    def __init__(self, policy, lib):
        self.policy, self.lib = policy, lib
        self.kernels = self.issued = None

    def run(self, step):
        inner = self.policy.build_distribution
        prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU,
                                                  torch.profiler.ProfilerActivity.CUDA])
        mode = IssueCount()
        lib_calls = [0]
        entry_points = [n[len("vlnce_"):] for n in _lib.exported_symbols()
                        if callable(getattr(type(self.lib), n[len("vlnce_"):], None))]

        def counted(f):
            def g(*a, **k):
                lib_calls[0] += 1
                return f(*a, **k)
            return g

        def opening(*a, **k):
            dist = inner(*a, **k)
            torch.cuda.synchronize()
            for n in entry_points:
                setattr(self.lib, n, counted(getattr(self.lib, n)))
            prof.start()
            mode.__enter__()
            return dist

        def closing():
            mode.__exit__(None, None, None)
            torch.cuda.synchronize()
            prof.stop()
            for n in entry_points:
                delattr(self.lib, n)

        self.policy.build_distribution = opening
        try:
            step(grad_hook=closing)
        finally:
            del self.policy.build_distribution
        kernels = [e for e in prof.events()
                   if e.device_type == torch.autograd.DeviceType.CUDA
                   and not e.name.startswith(("Memcpy", "Memset"))]
        self.kernels = len(kernels) if kernels else None
        self.issued = (mode.n, lib_calls[0])
        return self


def ab(name, policy, batch, hidden, a, lib, describe):
    opt = torch.optim.Adam(policy.parameters(), lr=2.5e-4)
    obs, prev, masks, tgt, w = batch
    wall = {s: [] for s in SIDES}
    last = {}

    def step(side, record=True, grad_hook=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = update_agent(policy, opt, obs, prev, masks, tgt, w, hidden, grad_hook=grad_hook,
                           fused_loss=(side == "fused"))
        torch.cuda.synchronize()
        if record:
            wall[side].append((time.perf_counter() - t0) * 1e3)
        last[side] = out

    for _ in range(a.warmup):
        for s in SIDES:
            step(s, record=False)
    for i in range(a.steps):
        for s in (SIDES if i % 2 == 0 else SIDES[::-1]):
            step(s)
    say(f"{name}: {describe}; {a.steps} steps per side after {a.warmup} warm-up steps per side, "
        "sides alternating")
    med = {}
    for s in SIDES:
        v = sorted(wall[s])
        med[s] = statistics.median(v)
        say(f"  fused_loss={str(s == 'fused'):5s}: host wall median {med[s]:7.3f} ms (min {v[0]:.3f}, "
            f"max {v[-1]:.3f}); last (loss, action_loss, aux_loss) = "
            f"({last[s][0]:.6f}, {last[s][1]:.6f}, {last[s][2]:.6f})")
    say(f"  default - fused (host wall medians): {med['default'] - med['fused']:+.3f} ms; "
        f"default / fused: {med['default'] / med['fused']:.4f}")
    for s in SIDES:   # one more step per side, not timed: what runs in the window
        win = Window(policy, lib).run(lambda grad_hook, s=s: step(s, False, grad_hook))
        count = (f"{win.kernels} kernels" if win.kernels is not None
                 else "no device activity from the profiler")
        say(f"  fused_loss={str(s == 'fused'):5s}: build_distribution returned -> backward() returned: "
            f"{count} ({win.issued[0]} aten operators + {win.issued[1]} library calls issued from "
            "Python)")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed steps per side")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "il_loss_ab.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = ops.L()
    vlnce_amd.AuxLosses.activate()
    say(f"scripts/il_loss_ab.py --steps {a.steps} --warmup {a.warmup}; {torch.cuda.get_device_name(0)}, "
        f"torch {torch.__version__}, libvlnce_hip ABI {lib.ABI}")
    try:
        run(a, dev, lib)
    finally:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


def run(a, dev, lib):
    torch.manual_seed(0)
    policy = vlnce_amd.build_model(vlnce_amd.make_config("CMAPolicy"),
                                   *vlnce_amd.make_spaces(256, 256)).to(dev)
    ab("headline batch", policy, headline_batch(dev), 512, a, lib,
       "CMA, N = 64, T = 1, 256x256 RGB-D, 80 tokens, progress monitor off")
    del policy

    torch.manual_seed(0)
    cfg = vlnce_amd.make_config("CMAPolicy", **{"PROGRESS_MONITOR.use": True})
    policy = vlnce_amd.build_model(cfg, *vlnce_amd.make_spaces(256, 256)).to(dev)
    batch, lens = cached_batch(dev)
    ab("cached-feature batch", policy, batch, policy.net.model_config.STATE_ENCODER.hidden_size, a,
       lib, f"CMA on cached trunk features, {len(lens)} episodes of lengths {lens} (T = {max(lens)}, "
       f"{max(lens) * len(lens)} rows), progress monitor on")
    vlnce_amd.AuxLosses.deactivate()


if __name__ == "__main__":
    main()
