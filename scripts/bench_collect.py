"""DAgger rollout collection (`DaggerTrainer._update_dataset`, dagger_trainer.py:248-467) on one
MI355X: the loop body without a simulator, CMA policy, 256x256 RGB-D.

  way A  the reference's: `o.cpu()` feature hooks (:294-314), torch.where mixing (:414-442),
         per-environment `.item()` read-backs (:429-444), and at an episode's end the host
         re-stack (`batch_obs(..., cpu)`) + `astype(np.float16)` (:341-356)
  way B  data_path.TrajectoryRecorder (feature_hook / append / pop) + data_path.dagger_step
  bare   act() alone, no hook registered

One process; the three arms alternate, every arm is warmed up first, `--reps` windows of
`--steps` steps each, every window ending in a device synchronise.  Reports per arm the
milliseconds per step (median, min, max over the windows), A's and B's cost on top of the bare
act(), the time to hand back `num_envs` episodes of `--steps` steps, and the append launch timed
with device events over back-to-back launches with its algorithmic bytes (the kernel time proper
comes from `rocprofv3 --kernel-trace --stats -- python scripts/bench_collect.py --append-only`).

    python scripts/bench_collect.py [--num-envs 64] [--steps 60] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import vlnce_amd
from vlnce_amd import data_path

DEV = "cuda:0"
EXPERT = "shortest_path_sensor"


def make_batch(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.zeros(n, 200, dtype=torch.long)
    tokens[:, :80] = torch.randint(1, 2504, (n, 80), generator=g)
    host = {"rgb": torch.randint(0, 256, (n, hw, hw, 3), generator=g).float(),
            "depth": torch.rand(n, hw, hw, 1, generator=g),
            "instruction": tokens,
            EXPERT: torch.randint(0, 4, (n, 1), generator=g).float()}
    return host, {k: v.to(DEV) for k, v in host.items()}


def append_bytes(n):
    """what one append launch of the cached CMA sensors must move: fp32 features + int64 tokens +
    two int64 action columns in, fp16 rows + the action columns out"""
    feats = 2048 * 16 + 128 * 16
    return n * (feats * 4 + 200 * 8 + 16), n * (feats * 2 + 200 * 2 + 16)


def append_only(n, iters):
    """the append launch alone on synthetic trunk outputs (the thing to put under rocprofv3)"""
    rec = data_path.TrajectoryRecorder(n, DEV, True, capacity=4)
    rgb = torch.randn(n, 4, 4, 2048, device=DEV).permute(0, 3, 1, 2)     # the trunks' NHWC view
    depth = torch.randn(n, 4, 4, 128, device=DEV).permute(0, 3, 1, 2)
    hooks = rec.feature_hook("rgb_features"), rec.feature_hook("depth_features")
    obs = {"instruction": torch.randint(0, 2504, (n, 200), device=DEV)}
    prev = torch.zeros(n, 1, dtype=torch.long, device=DEV)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(3):
        ev0.record()
        for _ in range(iters):
            hooks[0](None, None, rgb)
            hooks[1](None, None, depth)
            rec.append(obs, prev, prev)
            rec.discard(range(n))
        ev1.record()
        torch.cuda.synchronize()
        ms.append(ev0.elapsed_time(ev1) / iters)
    rd, wr = append_bytes(n)
    return {"launches": iters, "ms_per_launch_back_to_back": round(min(ms), 4),
            "bytes_read": rd, "bytes_written": wr,
            "GB_per_s_back_to_back": round((rd + wr) / (min(ms) * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--steps", type=int, default=60)     # steps per window = episode length popped
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--append-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_collect.py measures on a GPU; there is none"
    n, hw = a.num_envs, a.hw
    if a.append_only:
        print(json.dumps({"append": append_only(n, 200)}))
        return

    torch.manual_seed(0)
    policy = vlnce_amd.build_model(vlnce_amd.make_config("CMAPolicy"),
                                   *vlnce_amd.make_spaces(hw, hw)).to(DEV)
    cnn, venc = policy.net.rgb_encoder.cnn, policy.net.depth_encoder.visual_encoder
    batches = [make_batch(n, hw, 10 + k) for k in range(4)]
    states = torch.zeros(n, policy.net.num_recurrent_layers, 512, device=DEV)
    masks = torch.ones(n, 1, dtype=torch.uint8, device=DEV)
    prev_actions = torch.zeros(n, 1, dtype=torch.long, device=DEV)

    def act(batch):
        return policy.act(batch, states, prev_actions, masks, deterministic=False)[0]

    # ---- bare
    def window_bare(steps):
        for k in range(steps):
            act(batches[k % 4][1])
        torch.cuda.synchronize()
        return None

    # ---- way A: the reference's lines
    def hook_builder(tgt_tensor):
        def hook(m, i, o):
            tgt_tensor.set_(o.cpu())

        return hook

    def window_a(steps):
        rgb_features, depth_features = torch.zeros((1,)), torch.zeros((1,))
        hooks = [cnn.register_forward_hook(hook_builder(rgb_features)),
                 venc.register_forward_hook(hook_builder(depth_features))]
        episodes = [[] for _ in range(n)]
        for k in range(steps):
            host, batch = batches[k % 4]
            observations = [{"instruction": host["instruction"][i].numpy(),
                             EXPERT: host[EXPERT][i].numpy()} for i in range(n)]   # the simulator's
            actions = act(batch)
            actions = torch.where(torch.rand_like(actions, dtype=torch.float) < a.beta,
                                  batch[EXPERT].long(), actions)
            for i in range(n):
                observations[i]["rgb_features"] = rgb_features[i]
                observations[i]["depth_features"] = depth_features[i]
                episodes[i].append((observations[i], prev_actions[i].item(),
                                    batch[EXPERT][i].item()))
            skips = batch[EXPERT].long() == -1
            actions = torch.where(skips, torch.zeros_like(actions), actions)
            skips = skips.squeeze(-1).to(device="cpu", non_blocking=True)
            prev_actions.copy_(actions)
            _ = [x[0].item() for x in actions]
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        return episodes

    def pop_a(episodes):
        out = []
        for ep in episodes:
            traj_obs = {}
            for sensor in ep[0][0]:                       # batch_obs(..., cpu): stack, cast to float
                traj_obs[sensor] = torch.stack([torch.as_tensor(step[0][sensor]) for step in ep],
                                               dim=0).to(dtype=torch.float)
            del traj_obs[EXPERT]
            for k, v in traj_obs.items():
                traj_obs[k] = v.numpy().astype(np.float16)
            out.append([traj_obs, np.array([step[1] for step in ep], dtype=np.int64),
                        np.array([step[2] for step in ep], dtype=np.int64)])
        return out

    # ---- way B: the recorder
    rec = data_path.TrajectoryRecorder(n, DEV, True, exclude=(EXPERT,))
    rec_hooks = rec.feature_hook("rgb_features"), rec.feature_hook("depth_features")

    def window_b(steps):
        hooks = [cnn.register_forward_hook(rec_hooks[0]), venc.register_forward_hook(rec_hooks[1])]
        for k in range(steps):
            _, batch = batches[k % 4]
            actions = act(batch)
            rec.append(batch, prev_actions, batch[EXPERT])
            data_path.dagger_step(actions, batch[EXPERT], a.beta, prev_actions)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        return rec

    def pop_b(r):
        return r.pop(range(n))

    arms = {"bare": (window_bare, None), "A": (window_a, pop_a), "B": (window_b, pop_b)}
    step_ms = {k: [] for k in arms}
    pop_ms = {"A": [], "B": []}
    last, before = {}, {}
    with torch.no_grad():
        for name, (window, pop) in arms.items():          # warm-up: graphs, allocator, arenas
            got = window(8)
            if pop is not None:
                pop(got)
        for rep in range(a.reps):
            for name, (window, pop) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = window(a.steps)
                step_ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
                if pop is not None:
                    t0 = time.perf_counter()
                    before[name], last[name] = last.get(name), pop(got)
                    pop_ms[name].append((time.perf_counter() - t0) * 1e3)

    # The same batches go through every window, so the popped observations can be compared across
    # windows: B against A, and -- the control for how far two runs of the trunks agree with each
    # other -- B against B's previous window.  (Bit-equality of what the two hooks see in ONE
    # act() is tests/test_traj_recorder_gpu.py's; the mixed actions differ by design: each arm
    # draws its own uniforms.)
    def max_diff(xs, ys):
        return {k: float(max(np.abs(x[0][k].astype(np.float64) - y[0][k].astype(np.float64)).max()
                             for x, y in zip(xs, ys))) for k in xs[0][0]}

    def stat(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                "max": round(max(v), 3)}

    bare = statistics.median(step_ms["bare"])
    res = {
        "workload": f"DAgger collection loop body, CMAPolicy, num_envs {n}, {hw}x{hw}, "
                    f"{a.reps} windows of {a.steps} steps per arm, alternating",
        "step_ms": {k: stat(v) for k, v in step_ms.items()},
        "collection_ms_per_step_on_top_of_act": {
            "A_reference_way": round(statistics.median(step_ms["A"]) - bare, 3),
            "B_recorder": round(statistics.median(step_ms["B"]) - bare, 3)},
        f"pop_{n}_episodes_of_{a.steps}_steps_ms": {k: stat(v) for k, v in pop_ms.items()},
        "popped_observations_max_abs_diff": {"B_vs_A": max_diff(last["B"], last["A"]),
                                             "B_vs_previous_B": max_diff(last["B"], before["B"])},
        "append": append_only(n, 200),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
