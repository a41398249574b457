"""WaypointPolicy.fused_distributions -- evaluate_actions' log-probability and entropies as one
launch forward and one backward (vlnce_waypoint_eval / _bwd), no host synchronisation -- against the
default chain of torch distribution ops, A/B in one process on one MI355X.

The `waypoint_update_n32_256` geometry (bench.py --policy waypoint): one WDDPPO minibatch update at
num_envs = 32, 12 panorama frames + the history frame of 256x256 RGB-D per environment (416 frames),
200-token instructions, encoders in eval mode.  One policy (the same initial weights) and one Adam
optimizer per side, one resident batch, the two sides alternating step by step (and alternating who
goes first).  Per side: the median host wall time of a step (device idle before, the six statistics
read back and the device synchronised after), and -- in one extra step per side -- what happens
between the net's tail returning its head outputs and backward() returning: the kernels the device
ran (torch.profiler; the window opened and closed on a synchronised device), the aten operators and
library entry points issued from Python, and the host synchronisations
(torch.cuda.set_sync_debug_mode("warn") reports each one).

    python scripts/waypoint_dist_ab.py [--steps 40] [--warmup 6] [--out profiles/waypoint_dist_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import vlnce_amd  # noqa: E402
from vlnce_amd import _lib, ops  # noqa: E402
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update  # noqa: E402

SIDES = ("default", "fused")
LINES = []


def say(msg=""):
    print(msg, flush=True)
    LINES.append(msg)


def pano_sample(policy, dev, n=32, hw=256, tokens=200, seed=1):
    """bench.py's synth_pano_batch and the 9-tuple it makes of it: the action components are the
    policy's own deterministic act(), inside the truncated-normal supports"""
    g = torch.Generator().manual_seed(seed)
    obs = {"rgb": torch.randint(0, 256, (n, 12, hw, hw, 3), generator=g).float(),
           "depth": torch.rand(n, 12, hw, hw, 1, generator=g),
           "rgb_history": torch.randint(0, 256, (n, hw, hw, 3), generator=g).float(),
           "depth_history": torch.rand(n, hw, hw, 1, generator=g),
           "angle_features": torch.randn(n, 12, 4, generator=g),
           "instruction": torch.zeros(n, 200, dtype=torch.long)}
    obs["instruction"][:, :tokens] = torch.randint(1, 2504, (n, tokens), generator=g)
    prev = {"pano": torch.randint(0, 12, (n, 1), generator=g),
            "offset": (torch.rand(n, 1, generator=g) - 0.5) * 0.4,
            "distance": 0.25 + torch.rand(n, 1, generator=g) * 2.0}
    pano_action = torch.randint(0, 12, (n, 1), generator=g)
    value_preds = torch.randn(n, 1, generator=g) * 0.5
    adv = torch.randn(n, 1, generator=g)
    obs = {k: v.to(dev) for k, v in obs.items()}
    prev = {k: v.to(dev) for k, v in prev.items()}
    masks = torch.ones(n, 1, dtype=torch.uint8, device=dev)
    hid = policy.net.model_config.STATE_ENCODER.hidden_size
    h0 = torch.zeros(n, policy.net.num_recurrent_layers, hid, device=dev)
    with torch.no_grad():
        out = policy.act(obs, h0, {k: v.clone() for k, v in prev.items()}, masks, deterministic=True)
    actions = {k: v.clone() for k, v in out[2].items()}
    actions["pano"] = pano_action.to(dev)
    value_preds = value_preds.to(dev)
    return (obs, h0, actions, prev, value_preds, value_preds + 0.3, masks,
            torch.full((n, 1), -2.0, device=dev), adv.to(dev))


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
    """opens when the net's tail returns the head outputs, closes in the update's grad_hook, which
    runs right after loss.backward() returned"""

    def __init__(self, policy, lib):
        self.policy, self.lib = policy, lib
        self.kernels = self.issued = self.syncs = None

    def run(self, step):
        net = self.policy.net
        inner = net._tail
        prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU,
                                                  torch.profiler.ProfilerActivity.CUDA])
        mode = IssueCount()
        lib_calls = [0]
        caught = warnings.catch_warnings(record=True)
        seen = []
        entry_points = [n[len("vlnce_"):] for n in _lib.exported_symbols()
                        if callable(getattr(type(self.lib), n[len("vlnce_"):], None))]

        def counted(f):
            def g(*a, **k):
                lib_calls[0] += 1
                return f(*a, **k)
            return g

        def opening(*a, **k):
            heads = inner(*a, **k)
            torch.cuda.synchronize()
            for n in entry_points:
                setattr(self.lib, n, counted(getattr(self.lib, n)))
            prof.start()
            seen.append(caught.__enter__())
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            mode.__enter__()
            return heads

        def closing():
            mode.__exit__(None, None, None)
            torch.cuda.set_sync_debug_mode("default")
            caught.__exit__(None, None, None)
            torch.cuda.synchronize()
            prof.stop()
            for n in entry_points:
                delattr(self.lib, n)

        object.__setattr__(net, "_tail", opening)
        try:
            step(grad_hook=closing)
        finally:
            object.__setattr__(net, "_tail", inner)
        kernels = [e for e in prof.events()
                   if e.device_type == torch.autograd.DeviceType.CUDA
                   and not e.name.startswith(("Memcpy", "Memset"))]
        self.kernels = len(kernels) if kernels else None
        self.issued = (mode.n, lib_calls[0])
        self.syncs = sum("synchroniz" in str(w.message) for w in seen[0])
        return self


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed steps per side")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--num-envs", type=int, default=32)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waypoint_dist_ab.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = ops.L()
    say(f"scripts/waypoint_dist_ab.py --steps {a.steps} --warmup {a.warmup}; "
        f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, libvlnce_hip ABI {lib.ABI}")
    try:
        run(a, dev, lib)
    finally:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


def run(a, dev, lib):
    policies, opts = {}, {}
    for s in SIDES:
        torch.manual_seed(0)
        p = vlnce_amd.build_model(vlnce_amd.make_config("WaypointPolicy"),
                                  *vlnce_amd.make_spaces(a.hw, a.hw, pano=True)).to(dev)
        p.train()
        p.net.rgb_encoder.eval()
        p.net.depth_encoder.eval()
        p.fused_distributions = s == "fused"
        policies[s] = p
        opts[s] = torch.optim.Adam([q for q in p.parameters() if q.requires_grad], lr=2.5e-4)
    sample = pano_sample(policies["default"], dev, a.num_envs, a.hw)
    wall = {s: [] for s in SIDES}
    issue = {s: [] for s in SIDES}
    last = {}

    def step(side, record=True, grad_hook=None):
        s = list(sample)
        s[3] = {k: v.clone() for k, v in s[3].items()}   # the policy mutates prev_actions
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = wddppo_minibatch_update(policies[side], opts[side], tuple(s), PPOConfig(),
                                        grad_hook=grad_hook)
        t1 = time.perf_counter()   # everything is issued; the device may still be running
        out = torch.stack(stats).tolist()
        torch.cuda.synchronize()
        if record:
            wall[side].append((time.perf_counter() - t0) * 1e3)
            issue[side].append((t1 - t0) * 1e3)
        last[side] = out

    for _ in range(a.warmup):
        for s in SIDES:
            step(s, record=False)
    for i in range(a.steps):
        for s in (SIDES if i % 2 == 0 else SIDES[::-1]):
            step(s)
    say(f"waypoint_update_n32_256 geometry: WaypointPolicy WDDPPO minibatch update, num_envs = "
        f"{a.num_envs}, {13 * a.num_envs} frames of {a.hw}x{a.hw} RGB-D, 200 tokens, encoders in eval "
        f"mode; {a.steps} steps per side after {a.warmup} warm-up steps per side, sides alternating")
    med = {}
    for s in SIDES:
        v = sorted(wall[s])
        med[s] = statistics.median(v)
        say(f"  fused_distributions={str(s == 'fused'):5s}: host wall median {med[s]:7.3f} ms (min "
            f"{v[0]:.3f}, max {v[-1]:.3f}), of which the update call returned after "
            f"{statistics.median(issue[s]):.3f} ms; last (value_loss, action_loss, entropy_loss) = "
            f"({last[s][0]:.6f}, {last[s][1]:.6f}, {last[s][2]:.6f})")
    say(f"  default - fused (host wall medians): {med['default'] - med['fused']:+.3f} ms; "
        f"default / fused: {med['default'] / med['fused']:.4f}")
    for s in SIDES:   # one more step per side, not timed: what runs in the window
        win = Window(policies[s], lib).run(lambda grad_hook, s=s: step(s, False, grad_hook))
        count = (f"{win.kernels} kernels" if win.kernels is not None
                 else "no device activity from the profiler")
        say(f"  fused_distributions={str(s == 'fused'):5s}: tail returned -> backward() returned: "
            f"{count}, {win.syncs} host synchronisations ({win.issued[0]} aten operators + "
            f"{win.issued[1]} library calls issued from Python)")
    policies["fused"].check_eval_flags()
    # control: the same two policy objects with the switch the other way round, so that a difference
    # between the objects (allocation order, captured graphs) is told apart from one between the paths
    for s in SIDES:
        policies[s].fused_distributions = s != "fused"
        wall[s].clear()
        issue[s].clear()
    for _ in range(a.warmup):
        for s in SIDES:
            step(s, record=False)
    for i in range(a.steps // 2):
        for s in (SIDES if i % 2 == 0 else SIDES[::-1]):
            step(s)
    say(f"control, the switch swapped between the two policy objects ({a.steps // 2} steps per side):")
    for s in SIDES:
        say(f"  the policy that ran {s:7s} above, now fused_distributions="
            f"{str(policies[s].fused_distributions):5s}: host wall median "
            f"{statistics.median(wall[s]):7.3f} ms, update call returned after "
            f"{statistics.median(issue[s]):.3f} ms")


if __name__ == "__main__":
    main()
