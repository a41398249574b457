"""vlnce_amd.optim.Adam -- clip_grad_norm_ + Adam over the whole parameter list in two launches
(vlnce_grad_sumsq, vlnce_adam_step) -- against torch's default Adam and torch's fused=True Adam
(each with torch.nn.utils.clip_grad_norm_ in front where the trainer clips), A/B/C in one process
on one MI355X.

Three workloads, per side one policy (the same initial weights) and one optimizer, the sides
alternating step by step and rotating who goes first:
  1. the headline CMA update of bench.py (N = 64, T = 1, 256x256 RGB-D, 80 tokens), no clipping;
  2. the Waypoint DD-PPO minibatch update (num_envs 32, 12 x 256x256 RGB-D) with max_grad_norm 0.2;
  3. the CMA update with TRAINABLE visual encoders, no clipping.
Per side: the median host time inside optimizer.step() (+ clip_grad_norm_), the median host wall
time of a step (device idle before, synchronised after), and from one extra step under
torch.profiler, the window opened on a synchronised device when backward() has returned and closed
when the update call has returned: the number of kernels and the device time in it (sum of the
kernels, and first start -> last end).  For workload 3 also the achieved bytes/s of
adam_step_kernel (28 bytes per parameter: p, m, v read and written, g read) and, from three extra
steps with max_grad_norm set, of grad_sumsq_kernel (4 bytes per parameter).

    python scripts/fused_adam_ab.py [--steps 40] [--warmup 6] [--out profiles/fused_adam_ab.txt]
                                    [--workloads cma,waypoint,trainable]
VLNCE_AB_NAMES=1 also prints every device event of the profiled windows (start, duration, name).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

import vlnce_amd  # noqa: E402
from il_loss_ab import headline_batch  # noqa: E402
from vlnce_amd import ops  # noqa: E402
from vlnce_amd.il_harness import update_agent  # noqa: E402
from vlnce_amd.optim import Adam  # noqa: E402
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update  # noqa: E402
from waypoint_dist_ab import pano_sample  # noqa: E402

SIDES = ("torch", "torch fused", "vlnce_amd")
LINES = []


def say(msg=""):
    print(msg, flush=True)
    LINES.append(msg)


def make_optimizer(side, params, clip, **kw):
    if side == "torch":
        return torch.optim.Adam(params, **kw)
    if side == "torch fused":
        return torch.optim.Adam(params, fused=True, **kw)
    return Adam(params, max_grad_norm=clip, **kw)


class Timed:
    """host time spent inside optimizer.step() and clip_grad_norm_ of one update call"""

    def __init__(self, opt):
        self.ms = 0.0
        inner = opt.step

        def step(*a, **k):
            t0 = time.perf_counter()
            out = inner(*a, **k)
            self.ms += (time.perf_counter() - t0) * 1e3
            return out

        opt.step = step
        self.clip = torch.nn.utils.clip_grad_norm_

    def clipping(self, *a, **k):
        t0 = time.perf_counter()
        out = self.clip(*a, **k)
        self.ms += (time.perf_counter() - t0) * 1e3
        return out


def profile_window(update):
    """update(grad_hook) runs one update call; the window opens in grad_hook (backward() has
    returned) and closes when the call has returned.  -> the device's kernel events"""
    prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU,
                                              torch.profiler.ProfilerActivity.CUDA])

    def opening():
        torch.cuda.synchronize()
        prof.start()

    update(opening)
    torch.cuda.synchronize()
    prof.stop()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and not e.name.startswith(("Memcpy", "Memset", "Optimizer."))]   # (the last: torch's
    # record_function span around step(), mirrored onto the device timeline, not a kernel)


def describe(events):
    if not events:
        return "no device activity from the profiler", {}
    total = sum(e.time_range.elapsed_us() for e in events)
    span = max(e.time_range.end for e in events) - min(e.time_range.start for e in events)
    ours = {}
    if os.environ.get("VLNCE_AB_NAMES"):
        for e in events:
            print(f"    {e.time_range.start:.1f} +{e.time_range.elapsed_us():.1f} us  {e.name[:100]}")
    for e in events:
        for key in ("adam_step_kernel", "grad_sumsq_kernel"):
            if key in e.name:
                ours[key] = ours.get(key, 0.0) + e.time_range.elapsed_us()
    return f"{len(events)} kernels, {total / 1e3:.3f} ms of kernels, {span / 1e3:.3f} ms first start -> last end", ours


def ab(name, what, policies, update, clip, a, **kw):
    """update(policy, optimizer, grad_hook) -> one update call"""
    opts, timers = {}, {}
    for s in SIDES:
        params = [p for p in policies[s].parameters() if p.requires_grad]
        opts[s] = make_optimizer(s, params, clip, **kw)
        timers[s] = Timed(opts[s])
    n_params = sum(p.numel() for p in policies[SIDES[0]].parameters() if p.requires_grad)
    n_tensors = sum(1 for p in policies[SIDES[0]].parameters() if p.requires_grad)
    wall = {s: [] for s in SIDES}
    host = {s: [] for s in SIDES}

    def step(side, record=True, grad_hook=None):
        timer = timers[side]
        timer.ms = 0.0
        torch.nn.utils.clip_grad_norm_ = timer.clipping
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            update(policies[side], opts[side], grad_hook)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        finally:
            torch.nn.utils.clip_grad_norm_ = timer.clip
        if record:
            wall[side].append((t1 - t0) * 1e3)
            host[side].append(timer.ms)

    for _ in range(a.warmup):
        for s in SIDES:
            step(s, record=False)
    for i in range(a.steps):
        k = i % len(SIDES)
        for s in SIDES[k:] + SIDES[:k]:
            step(s)
    say(f"{name}: {what}; {n_params} trainable parameters in {n_tensors} tensors, "
        f"{'max_grad_norm ' + str(clip) if clip is not None else 'no clipping'}; {a.steps} steps per side "
        f"after {a.warmup} warm-up steps per side, sides alternating")
    med = {}
    for s in SIDES:
        w, h = sorted(wall[s]), sorted(host[s])
        med[s] = statistics.median(w)
        say(f"  {s:12s}: host inside step(){' + clip_grad_norm_' if clip is not None else ''} median "
            f"{statistics.median(h):6.3f} ms (min {h[0]:.3f}); wall per step median {med[s]:7.3f} ms "
            f"(min {w[0]:.3f}, max {w[-1]:.3f})")
    for s in SIDES[:2]:
        say(f"  {s} - vlnce_amd (wall medians): {med[s] - med['vlnce_amd']:+.3f} ms")
    ours = {}
    for s in SIDES:   # one more step per side, not timed: what the device runs after backward()
        text, mine = describe(profile_window(lambda hook, s=s: step(s, False, hook)))
        say(f"  {s:12s}: backward() returned -> update returned: {text}")
        ours = mine or ours
    return opts, n_params, ours


def bandwidth(n_params, ours):
    for key, per in (("adam_step_kernel", 28), ("grad_sumsq_kernel", 4)):
        if key in ours:
            us = ours[key]
            say(f"  {key}: {us:.1f} us for {per} x {n_params} bytes = "
                f"{per * n_params / us / 1e6:.3f} TB/s")


def cma_policies(dev, **overrides):
    out = {}
    for s in SIDES:
        torch.manual_seed(0)
        out[s] = vlnce_amd.build_model(vlnce_amd.make_config("CMAPolicy", **overrides),
                                       *vlnce_amd.make_spaces(256, 256)).to(dev)
    return out


def run(a, dev):
    obs, prev, masks, tgt, w = headline_batch(dev)

    def cma_update(policy, opt, grad_hook):
        update_agent(policy, opt, obs, prev, masks, tgt, w, 512, grad_hook=grad_hook)

    if "cma" in a.workloads:
        ab("headline CMA update", "CMA, N = 64, T = 1, 256x256 RGB-D, 80 tokens", cma_policies(dev),
           cma_update, None, a, lr=2.5e-4)

    if "waypoint" in a.workloads:
        policies = {}
        for s in SIDES:
            torch.manual_seed(0)
            p = vlnce_amd.build_model(vlnce_amd.make_config("WaypointPolicy"),
                                      *vlnce_amd.make_spaces(256, 256, pano=True)).to(dev)
            p.train()
            p.net.rgb_encoder.eval()
            p.net.depth_encoder.eval()
            policies[s] = p
        sample = pano_sample(policies[SIDES[0]], dev, 32, 256)
        cfg = PPOConfig()

        def wp_update(policy, opt, grad_hook):
            s = list(sample)
            s[3] = {k: v.clone() for k, v in s[3].items()}   # the policy mutates prev_actions
            wddppo_minibatch_update(policy, opt, tuple(s), cfg, grad_hook=grad_hook)

        ab("Waypoint DD-PPO minibatch update", "num_envs 32, 12 x 256x256 RGB-D + history, 200 tokens",
           policies, wp_update, cfg.max_grad_norm, a, lr=2.5e-4, eps=1e-5)
        del policies, sample

    if "trainable" in a.workloads:
        policies = cma_policies(dev, **{"RGB_ENCODER.trainable": True, "DEPTH_ENCODER.trainable": True})
        opts, n_params, ours = ab("trainable-encoder CMA update",
                                  "CMA with trainable visual encoders, N = 64, T = 1, 256x256 RGB-D",
                                  policies, cma_update, None, a, lr=2.5e-4)
        bandwidth(n_params, ours)
        policy = policies["vlnce_amd"]
        clipped = Adam([p for p in policy.parameters() if p.requires_grad], lr=2.5e-4, max_grad_norm=1e3)
        clipped.load_state_dict(opts["vlnce_amd"].state_dict())
        for _ in range(2):
            cma_update(policy, clipped, None)
        _, ours = describe(profile_window(lambda hook: cma_update(policy, clipped, hook)))
        say("  the same step with max_grad_norm set (the norm pass added):")
        bandwidth(n_params, ours)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed steps per side")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--workloads", default="cma,waypoint,trainable")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_adam_ab.txt"))
    a = ap.parse_args()
    a.workloads = a.workloads.split(",")
    dev = torch.device("cuda:0")
    lib = ops.L()
    say(f"scripts/fused_adam_ab.py --steps {a.steps} --warmup {a.warmup}; {torch.cuda.get_device_name(0)}, "
        f"torch {torch.__version__}, libvlnce_hip ABI {lib.ABI}, chunk {lib.adam_chunk()}, "
        f"{lib.adam_max_tensors()} tensors per launch")
    try:
        run(a, dev)
    finally:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
