"""The action half of the Waypoint DD-PPO trainer's rollout step, two ways on one MI355X:
  A  ppo_harness.act_for_rollout with policy.fused_act = True: the net, ONE vlnce_waypoint_act launch,
     one [B, 8] read-back, ONE vlnce_waypoint_history_pick launch
  B  the default path: WaypointPolicy.act over torch's distribution objects, then the reference's loop
     over the environments (ddppo_waypoint_trainer.py:190-220; act_for_rollout with the switch off)
at num_envs 8 and 32, full Waypoint sensor sizes (scripts/rollout_storage_ab.py: 224 px RGB, 256 px
depth, 12 panorama frames), sampled actions, the same policy and the same storage for both sides.

The sides alternate call by call and swap who goes first; medians of --reps calls.  Per step:
  host    wall time from entering the call, device idle before, to having the simulator's actions and
          the logging predictions on the host (the call's return)
  idle    the same, to the device being idle again (the history frames are in place)
  tail    `host` minus the wall time of the net and the critic alone on an idle device, waited for:
          what the distributions, the read-backs and the per-environment loop add to the step
  ops     device operations (kernels and copies) of one extra call under torch.profiler
  syncs   host synchronisations of one extra call, counted by torch.cuda.set_sync_debug_mode("warn")

    python scripts/waypoint_act_ab.py [--reps 40] [--warmup 5] [--envs 8 32] [--out profiles/waypoint_act_ab.txt]
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
from rollout_storage_ab import SENSORS, device_ops  # noqa: E402
from vlnce_amd import ppo_harness  # noqa: E402

DEV = "cuda:0"
LINES = []


def say(msg=""):
    print(msg, flush=True)
    LINES.append(msg)


def build_policy():
    cfg = vlnce_amd.make_config("WaypointPolicy")
    obs_space, act_space = vlnce_amd.make_spaces(256, 256, pano=True)
    obs_space.spaces["rgb"] = vlnce_amd.make_spaces(224, 224, pano=True)[0].spaces["rgb"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (random trunk weights: timing only)
        policy = vlnce_amd.WaypointPolicy.from_config(cfg, obs_space, act_space)
    policy.to(DEV)
    policy.train()          # agent.train(); visual encoders .eval() (ddppo_waypoint_trainer.py:526-530)
    policy.net.rgb_encoder.eval()
    policy.net.depth_encoder.eval()
    return policy, cfg.MODEL.STATE_ENCODER.hidden_size


def build_storage(policy, hidden, n):
    space = types.SimpleNamespace(spaces={k: types.SimpleNamespace(shape=s) for k, s in SENSORS.items()})
    st = vlnce_amd.ActionDictRolloutStorage(2, n, space, hidden, policy.net.num_recurrent_layers, device=DEV)
    g = torch.Generator().manual_seed(n)
    st.step = 1
    obs = st.observations
    obs["rgb"][1].copy_(torch.randint(0, 256, obs["rgb"][1].shape, generator=g).float())
    obs["depth"][1].copy_(torch.rand(obs["depth"][1].shape, generator=g))
    obs["angle_features"][1].copy_(torch.randn(obs["angle_features"][1].shape, generator=g))
    tokens = torch.zeros(n, 200)
    tokens[:, :60] = torch.randint(1, 2000, (n, 60), generator=g).float()
    obs["instruction"][1].copy_(tokens)
    st.masks[1].fill_(1)
    return st


def count_syncs(fn, where=None):
    """host synchronisations of fn(); where: a list that receives the file:line of each"""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    hits = [w for w in seen if "called a synchronizing" in str(w.message)]   # (not the mode's own notice)
    if where is not None:
        where += [f"{os.path.relpath(w.filename, ROOT)}:{w.lineno}" for w in hits]
    return len(hits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--envs", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=None)
    ap.add_argument("--where", action="store_true", help="print where each side synchronises")
    args = ap.parse_args()
    policy, hidden = build_policy()
    say(f"# scripts/waypoint_act_ab.py: {torch.cuda.get_device_name(0)}; sampled actions; medians of "
        f"{args.reps} steps, sides alternating")
    say(f"{'num_envs':>8s}  {'side':26s}{'host ms':>10s}{'idle ms':>10s}{'tail ms':>10s}{'ops':>7s}{'syncs':>7s}")
    for n in args.envs:
        st = build_storage(policy, hidden, n)

        def step(fused):
            policy.fused_act = fused
            return ppo_harness.act_for_rollout(policy, st)

        def net_only():
            observation = {k: v[1] for k, v in st.observations.items()}
            prev = {k: v[1] for k, v in st.prev_actions.items()}
            with torch.no_grad():
                out = policy.net(observation, st.recurrent_hidden_states[1], prev, st.masks[1],
                                 raw_pano_logits=True)
                policy.critic(out[5])

        sides = {"A fused_act": True, "B default + reference loop": False}
        times = {side: [] for side in sides}
        net = []
        for rep in range(-args.warmup, args.reps):
            torch.manual_seed(1000 + rep)
            order = list(sides) if rep % 2 == 0 else list(sides)[::-1]
            for side in order + ["net"]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if side == "net":
                    net_only()
                else:
                    step(sides[side])
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if rep >= 0:
                    (net if side == "net" else times[side]).append((t1 - t0, t2 - t0))
        net_ms = statistics.median(t for _, t in net) * 1e3
        for side, fused in sides.items():
            host = statistics.median(h for h, _ in times[side]) * 1e3
            idle = statistics.median(i for _, i in times[side]) * 1e3
            ops = len(device_ops(lambda: step(fused)))
            where = []
            syncs = count_syncs(lambda: step(fused), where)
            say(f"{n:8d}  {side:26s}{host:10.3f}{idle:10.3f}{host - net_ms:10.3f}{ops:7d}{syncs:7d}")
            if args.where:
                print("\n".join(f"          {w}" for w in where), flush=True)
        say(f"{n:8d}  {'(net + critic alone)':26s}{'':10s}{net_ms:10.3f}{'':10s}{len(device_ops(net_only)):7d}"
            f"{count_syncs(net_only):7d}")
        del st
        torch.cuda.empty_cache()
    policy.fused_act = False
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
