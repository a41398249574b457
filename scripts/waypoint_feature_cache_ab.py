"""The Waypoint DD-PPO loop with and without the trunk-feature cache, on one MI355X:
  off  ActionDictRolloutStorage as it was: every stored frame goes through its trunk in act() and
       again in every epoch's evaluate_actions, the history frame every step
  on   ActionDictRolloutStorage(trunk_features=...): act_for_rollout stores the panorama's trunk outputs
       and picks the history features from them, bootstrap_value stores the last row's, wddppo_update
       gathers no frame and runs no trunk
Full Waypoint sensor sizes and the geometry of scripts/rollout_storage_ab.py (num_steps 16, 8
environments, num_mini_batch 4, ppo_epoch 2, 224 px RGB, 256 px depth).  One policy, one optimizer and
one storage per side, built under the same seeds; the sides alternate and swap who goes first; medians
of --reps after --warmup rounds that warm every shape.  A host clock around work that ends in a
synchronise:
  step       one rollout step through act_for_rollout (the insert is outside the clock)
  minibatch  one minibatch of the update: its gather, forward, backward, clip + Adam
  update     a whole PPO update: bootstrap_value, compute_returns, 2 x 4 minibatches, after_update
Beside them: trunk forward calls and frames per PPO update and per rollout (counted at the encoders),
the trunks' device operations per PPO update (one extra update per side under torch.profiler), and the
bytes of the added arenas.

--errors writes, for the six PPO statistics and the post-update parameters, the largest difference
between an update from the cache and an update from the frames (same rollout, same state, same
permutations), and beside it the difference between two updates from the frames: the yardstick.

    python scripts/waypoint_feature_cache_ab.py [--reps 40] [--warmup 3] \\
        [--out profiles/waypoint_feature_cache_ab.txt] [--errors profiles/waypoint_feature_cache_errors.txt]
"""
import argparse
import os
import statistics
import sys
import time
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import vlnce_amd  # noqa: E402
from rollout_storage_ab import MINI, N, SENSORS, T, device_ops  # noqa: E402
from vlnce_amd import ppo_harness  # noqa: E402
from vlnce_amd.optim import Adam  # noqa: E402
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update, wddppo_update  # noqa: E402

DEV = "cuda:0"
EPOCHS = 2
CFG = PPOConfig()
LINES = []
TRUNK_KERNELS = ("conv_", "stem7", "maxpool", "scale_shift", "gn_", "frames_", "avgpool")


def say(msg="", lines=LINES):
    print(msg, flush=True)
    lines.append(msg)


class Side:
    """one policy, one optimizer, one storage; the simulator's frames are shared"""

    def __init__(self, cache):
        torch.manual_seed(0)
        cfg = vlnce_amd.make_config("WaypointPolicy")
        obs_space, act_space = vlnce_amd.make_spaces(256, 256, pano=True)
        obs_space.spaces["rgb"] = vlnce_amd.make_spaces(224, 224, pano=True)[0].spaces["rgb"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # (random trunk weights: timing only)
            self.policy = vlnce_amd.WaypointPolicy.from_config(cfg, obs_space, act_space)
        self.policy.to(DEV)
        self.policy.train()          # agent.train(); visual encoders .eval() (ddppo_waypoint_trainer.py:526-530)
        self.policy.net.rgb_encoder.eval()
        self.policy.net.depth_encoder.eval()
        self.policy.fused_act = True
        self.opt = Adam([p for p in self.policy.parameters() if p.requires_grad], lr=2.5e-4, eps=1e-5,
                        max_grad_norm=CFG.max_grad_norm)
        net = self.policy.net
        space = types.SimpleNamespace(spaces={k: types.SimpleNamespace(shape=s) for k, s in SENSORS.items()})
        self.st = vlnce_amd.ActionDictRolloutStorage(
            T, N, space, net._hidden_size, net.num_recurrent_layers, device=DEV,
            trunk_features=net.trunk_feature_shapes() if cache else None)
        self.cache = cache
        self.calls = self.frames = 0
        for enc, key in ((net.rgb_encoder, "rgb"), (net.depth_encoder, "depth")):
            self._count(enc, key)

    def _count(self, enc, key):
        inner = type(enc).trunk_features

        def counted(observations):
            x = observations[key]
            parts = x if isinstance(x, (tuple, list)) else (x,)
            self.calls += 1
            self.frames += sum(p.numel() // (p.shape[-1] * p.shape[-2] * p.shape[-3]) for p in parts[:2])
            return inner(enc, observations)

        enc.trunk_features = counted

    def counts(self):
        out, self.calls, self.frames = (self.calls, self.frames), 0, 0
        return out


def simulator(seed):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.zeros(N, 200)
    tokens[:, :60] = torch.randint(1, 2000, (N, 60), generator=g).float()
    return {"rgb": torch.randint(0, 256, (N,) + SENSORS["rgb"], generator=g).float().to(DEV),
            "depth": torch.rand((N,) + SENSORS["depth"], generator=g).to(DEV),
            "angle_features": torch.randn((N,) + SENSORS["angle_features"], generator=g).to(DEV),
            "instruction": tokens.to(DEV)}


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def rollout_step(side, frames, rewards, masks):
    """one step as ddppo_waypoint_trainer.py:160-240 drives it; returns the clocked action half"""
    dt, (outputs, history, _) = clocked(lambda: ppo_harness.act_for_rollout(side.policy, side.st))
    values, _, elements, _, _, log_prob, hidden, _ = outputs
    batch = dict(frames)
    for k, v in history.items():
        batch[k + "_history" if k in ("rgb", "depth") else k] = v
    side.st.insert(batch, hidden, elements, log_prob, values, rewards, masks)
    return dt


def ppo_update(side, seed, use_trunk_cache=None):
    torch.manual_seed(seed)      # the minibatch permutations
    st = side.st
    st.compute_returns(ppo_harness.bootstrap_value(side.policy, st), True, 0.99, 0.95)
    stats = wddppo_update(side.policy, side.opt, st, CFG, ppo_epoch=EPOCHS, num_mini_batch=MINI,
                          use_trunk_cache=side.cache if use_trunk_cache is None else use_trunk_cache)
    st.after_update()
    return stats


def minibatches(side, seed):
    """the update's minibatches one by one, each clocked with its share of the gather"""
    torch.manual_seed(seed)
    st, times = side.st, []
    st.compute_returns(ppo_harness.bootstrap_value(side.policy, st), True, 0.99, 0.95)
    adv = st.get_advantages(False)
    for _ in range(EPOCHS):
        gen = st.recurrent_generator(adv, MINI, frames=not side.cache)
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sample = next(gen, None)
            if sample is None:
                break
            if side.cache:
                sample[0]["trunk_feature_key"] = st.trunk_key
            wddppo_minibatch_update(side.policy, side.opt, sample, CFG)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    st.after_update()
    return times


def collect(side, sims, g):
    times = []
    for t in range(T):
        rewards = (torch.randn(N, 1, generator=g) * 0.5).to(DEV)
        masks = (torch.rand(N, 1, generator=g) > 0.05).float().to(DEV)
        times.append(rollout_step(side, sims[(t + 1) % len(sims)], rewards, masks))
    return times


def timing(args):
    sides = {"off": Side(False), "on": Side(True)}
    sims = [simulator(s) for s in range(3)]
    gens = {k: torch.Generator().manual_seed(5) for k in sides}
    for side in sides.values():
        for k, v in sims[0].items():
            side.st.observations[k][0].copy_(v)
    step_t = {k: [] for k in sides}
    mini_t = {k: [] for k in sides}
    upd_t = {k: [] for k in sides}
    counts = {}
    # even rounds clock the update as a whole, odd rounds minibatch by minibatch until there are enough
    rounds = max(args.warmup, 2) + args.reps + -(-args.reps // (EPOCHS * MINI)) + 2
    for rnd in range(rounds):
        order = list(sides) if rnd % 2 == 0 else list(sides)[::-1]
        for k in order:
            side = sides[k]
            torch.manual_seed(100 + rnd)     # the actions' noise
            side.counts()
            ts = collect(side, sims, gens[k])
            rollout_counts = side.counts()
            if rnd % 2 == 0 or len(mini_t[k]) >= args.reps:
                dt, _ = clocked(lambda: ppo_update(side, 1000 + rnd))
                if rnd >= args.warmup:
                    upd_t[k].append(dt)
                    counts[k] = (rollout_counts, side.counts())
            else:
                tm = minibatches(side, 1000 + rnd)
                if rnd >= args.warmup:
                    mini_t[k] += tm
            if rnd >= args.warmup:
                step_t[k] += ts
        if all(len(upd_t[k]) >= args.reps and len(mini_t[k]) >= args.reps for k in sides):
            break
    name = torch.cuda.get_device_name(0)
    say(f"# scripts/waypoint_feature_cache_ab.py: {name}; num_steps {T}, {N} environments, num_mini_batch "
        f"{MINI}, ppo_epoch {EPOCHS}, 224 px RGB / 256 px depth; medians of {args.reps}, sides alternating")
    say(f"{'':22s}{'cache off':>12s}{'cache on':>12s}{'off / on':>10s}")
    for label, d in (("ms per rollout step", step_t), ("ms per minibatch", mini_t),
                     ("ms per PPO update", upd_t)):
        med = {k: statistics.median(d[k][-args.reps:]) * 1e3 for k in sides}
        say(f"{label:22s}{med['off']:12.3f}{med['on']:12.3f}{med['off'] / med['on']:10.2f}"
            f"   (n = {min(len(d['off']), args.reps)})")
    for label, i in (("per rollout of 16 steps", 0), ("per PPO update", 1)):
        say(f"trunk forward calls / frames {label}: off {counts['off'][i][0]} / {counts['off'][i][1]}, "
            f"on {counts['on'][i][0]} / {counts['on'][i][1]}")
    # kernel counts: one extra update per side under the profiler, outside every clock
    for k, side in sides.items():
        collect(side, sims, gens[k])
        ops = device_ops(lambda: ppo_update(side, 7))
        trunk = [e for e in ops if any(t in e.name for t in TRUNK_KERNELS)]
        say(f"device operations per PPO update, cache {k}: {len(ops)}, of them trunk kernels "
            f"({', '.join(TRUNK_KERNELS)}): {len(trunk)}")
    st = sides["on"].st
    added = sum(v.numel() * v.element_size() for k, v in st.observations.items()
                if k.endswith("_features") and k != "angle_features")
    frames = sum(st.observations[k].numel() * st.observations[k].element_size()
                 for k in ("rgb", "depth", "rgb_history", "depth_history"))
    say(f"added arenas: {added / 1e6:.1f} MB beside {frames / 1e9:.2f} GB of frame arenas")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


def errors(args):
    """cache against frames on ONE rollout from the same state, and frames against frames"""
    lines = []
    sims = [simulator(s) for s in range(3)]
    collector = Side(True)
    for k, v in sims[0].items():
        collector.st.observations[k][0].copy_(v)
    torch.manual_seed(3)
    collect(collector, sims, torch.Generator().manual_seed(5))
    results = {}
    for name, use in (("cache", True), ("frames 1", False), ("frames 2", False)):
        side = collector if name == "cache" else Side(True)
        side.st = collector.st
        torch.manual_seed(11)
        st = side.st
        if name == "cache":
            st.compute_returns(ppo_harness.bootstrap_value(side.policy, st), True, 0.99, 0.95)
        stats = wddppo_update(side.policy, side.opt, st, CFG, ppo_epoch=EPOCHS, num_mini_batch=MINI,
                              use_trunk_cache=use)
        params = torch.cat([p.detach().reshape(-1) for p in side.policy.parameters()]).double().cpu()
        results[name] = (torch.tensor(stats, dtype=torch.float64), params)
    say(f"# scripts/waypoint_feature_cache_ab.py --errors: {torch.cuda.get_device_name(0)}; one rollout of "
        f"{T} steps x {N} environments, one wddppo_update ({EPOCHS} x {MINI} minibatches, clip + Adam) from "
        "the same state and the same permutations", lines)
    names = ("value_loss", "action_loss", "entropy_loss", "pano_entropy", "offset_entropy", "distance_entropy")
    say(f"{'':20s}{'|cache - frames|':>20s}{'|frames - frames|':>20s}{'value (frames)':>18s}", lines)
    sc, sf, sg = results["cache"][0], results["frames 1"][0], results["frames 2"][0]
    for i, n in enumerate(names):
        say(f"{n:20s}{abs(sc[i] - sf[i]):20.3e}{abs(sf[i] - sg[i]):20.3e}{sf[i]:18.6f}", lines)
    pc, pf, pg = results["cache"][1], results["frames 1"][1], results["frames 2"][1]
    say(f"{'parameters (max)':20s}{(pc - pf).abs().max():20.3e}{(pf - pg).abs().max():20.3e}"
        f"{pf.abs().max():18.6f}", lines)
    say(f"parameters that differ: cache vs frames {int((pc != pf).sum())}, frames vs frames "
        f"{int((pf != pg).sum())}, of {pf.numel()}", lines)
    with open(args.errors, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--errors", default=None)
    ap.add_argument("--no-timing", action="store_true")
    args = ap.parse_args()
    if args.errors:
        errors(args)
        torch.cuda.empty_cache()
    if not args.no_timing:
        timing(args)


if __name__ == "__main__":
    main()
