"""The LSTM state-encoder rollout as one launch per direction against the step launches, A/B in
one process on one MI355X.

  1. the cached-feature DAgger update of the CMA policy (5 episodes x 100 steps, H = 512, the
     batch of scripts/bench_data_path.py) with STATE_ENCODER.rnn_type = LSTM: the one-launch arm
     and the step arm alternate step by step (the step arm = `lstm_rollout_supported` patched to
     False on the library object; one policy per arm, because the tail of a policy is replayed
     from a HIP graph that keeps the path it was captured with); median of GPU-event time and of
     host wall time per arm, with the tail graphs on (the default) and off (VLNCE_HIP_GRAPHS=0);
  2. the two rollout launches alone (HIP events, back to back) at T = 100, N in {1, 5, 16},
     H = 512, beside the GRU rollout at the same shapes.

    python scripts/lstm_rollout_ab.py [--steps 40] [--warmup 6] [--reps 30]
    python scripts/lstm_rollout_ab.py --kernels-only    # part 2 alone (e.g. once per VLNCE_HIP_LIB)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vlnce_amd  # noqa: E402
from vlnce_amd import data_path, ops  # noqa: E402
from vlnce_amd.il_harness import update_agent  # noqa: E402


def cached_batch(episodes, steps, dev):
    """the batch of scripts/bench_data_path.py: ragged fp16 feature rows, collated on the device"""
    rng = np.random.RandomState(0)
    lens = [max(1, int(steps * f)) for f in np.linspace(1.0, 0.55, episodes)]
    trajs = []
    for T in lens:
        obs = {"rgb_features": rng.rand(T, 2048, 4, 4).astype(np.float16),
               "depth_features": rng.rand(T, 128, 4, 4).astype(np.float16),
               "instruction": np.tile(np.concatenate([rng.randint(1, 2504, size=80),
                                                      np.zeros(120, np.int64)])[None], (T, 1))}
        oracle = rng.randint(0, 4, size=T).astype(np.int64)
        trajs.append((obs, np.concatenate([[0], oracle[:-1]]).astype(np.int64), oracle))
    return data_path.collate_trajectories(trajs, dev, inflection_coef=3.2), lens


class Arm:
    """one policy + optimizer per arm: the tail of a policy (state encoders included) is replayed
    from a HIP graph captured on its second call, so an arm keeps the path it was captured with"""

    def __init__(self, name, dev, lib):
        self.name, self.lib = name, lib
        torch.manual_seed(0)
        cfg = vlnce_amd.make_config("CMAPolicy", **{"STATE_ENCODER.rnn_type": "LSTM"})
        self.policy = vlnce_amd.build_model(cfg, *vlnce_amd.make_spaces(256, 256)).to(dev)
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=2.5e-4)
        self.hidden = self.policy.net.model_config.STATE_ENCODER.hidden_size
        self.calls = {"lstm_rollout_fwd": 0, "rnn_step_fwd": 0}  # issued from Python (eager / capture)
        self.gpu, self.wall, self.loss = [], [], None

    def step(self, batch, record=True):
        lib = self.lib
        obs_b, prev_b, masks_b, corr_b, w_b = batch
        inner = {n: getattr(lib, n) for n in self.calls}

        def counting(n):
            def f(*x):
                self.calls[n] += 1
                return inner[n](*x)
            return f

        for n in self.calls:
            setattr(lib, n, counting(n))
        if self.name == "step":
            lib.lstm_rollout_supported = lambda N, H: False
        try:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            self.loss, _, _ = update_agent(self.policy, self.opt, obs_b, prev_b, masks_b, corr_b, w_b,
                                           self.hidden)
            e1.record()
            torch.cuda.synchronize()
            if record:
                self.gpu.append(e0.elapsed_time(e1))
                self.wall.append((time.perf_counter() - t0) * 1e3)
        finally:
            for n in self.calls:
                delattr(lib, n)
            if self.name == "step":
                del lib.lstm_rollout_supported


def update_ab(a, dev, lib, graphs):
    os.environ["VLNCE_HIP_GRAPHS"] = "1" if graphs else "0"  # read by the tail on every call
    batch, lens = cached_batch(a.episodes, a.rollout_steps, dev)
    arms = [Arm("one_launch", dev, lib), Arm("step", dev, lib)]
    T, N, H = max(lens), a.episodes, arms[0].hidden
    assert lib.lstm_rollout_supported(N, H), (N, H)
    for _ in range(a.warmup):
        for arm in arms:
            arm.step(batch, record=False)
    for i in range(a.steps):
        for arm in (arms if i % 2 == 0 else arms[::-1]):  # alternate, and alternate who goes first
            arm.step(batch)
    print(f"cached-feature DAgger update, CMA, STATE_ENCODER.rnn_type = LSTM: {N} episodes, lengths {lens}, "
          f"T = {T}, H = {H}; tail graphs {'on (default)' if graphs else 'off (VLNCE_HIP_GRAPHS=0)'}; "
          f"{a.steps} steps per arm after {a.warmup} warm-up steps per arm, arms alternating")
    for arm in arms:
        g, w = sorted(arm.gpu), sorted(arm.wall)
        print(f"  {arm.name:10s}: GPU events median {statistics.median(g):7.3f} ms (min {g[0]:.3f}, max {g[-1]:.3f}); "
              f"host wall median {statistics.median(w):7.3f} ms (min {w[0]:.3f}, max {w[-1]:.3f}); "
              f"issued from Python over the run: lstm_rollout_fwd {arm.calls['lstm_rollout_fwd']}, "
              f"rnn_step_fwd {arm.calls['rnn_step_fwd']}; last loss {arm.loss:.6f}")
    one, stp = arms
    assert one.calls["rnn_step_fwd"] == 0 and one.calls["lstm_rollout_fwd"] > 0, one.calls
    assert stp.calls["lstm_rollout_fwd"] == 0 and stp.calls["rnn_step_fwd"] > 0, stp.calls
    r = statistics.median(stp.wall) / statistics.median(one.wall)
    print(f"  step / one_launch (host wall medians): {r:.3f}")


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def kernels(a, dev, lib):
    print(f"rollout launches alone, H = 512, T = 100 (HIP events over {a.reps} back-to-back calls, "
          "each call = the workspace zeroing + the persistent kernel):")
    T, H = 100, 512
    for N in (1, 5, 16):
        row = []
        for kind, G in (("LSTM", 4), ("GRU", 3)):
            GH = G * H
            torch.manual_seed(0)
            gi = torch.randn(T, N, GH, device=dev) * 0.7
            h0, c0 = torch.randn(N, H, device=dev) * 0.4, torch.randn(N, H, device=dev) * 0.4
            w = torch.randn(GH, H, device=dev) * H ** -0.5
            b = torch.randn(GH, device=dev) * 0.1
            mask = (torch.rand(T, N, device=dev) > 0.1).to(torch.uint8)
            hp, out, aux = (torch.empty(T, N, H, device=dev) for _ in range(3))
            gates = torch.empty(T, N, GH, device=dev)
            wt = w.t().contiguous()
            dout = torch.randn(T, N, H, device=dev)
            dgi, dgh = torch.empty(T, N, GH, device=dev), torch.empty(T, N, GH, device=dev)
            dh0, dc0 = torch.empty(N, H, device=dev), torch.empty(N, H, device=dev)
            if kind == "LSTM":
                ws = torch.empty(lib.lstm_rollout_workspace_bytes(N, H), dtype=torch.uint8, device=dev)
                f = timed(lambda: lib.lstm_rollout_fwd(gi, h0, c0, mask, w, b, hp, out, gates, aux, ws,
                                                       T, N, H), a.reps)
                bw = timed(lambda: lib.lstm_rollout_bwd(dout, None, None, gates, aux, hp, c0, mask, wt,
                                                        dgi, dh0, dc0, ws, T, N, H), a.reps)
            else:
                ws = torch.empty(lib.gru_rollout_workspace_bytes(N, H), dtype=torch.uint8, device=dev)
                f = timed(lambda: lib.gru_rollout_fwd(gi, h0, mask, w, b, hp, out, gates, aux, ws,
                                                      T, N, H), a.reps)
                bw = timed(lambda: lib.gru_rollout_bwd(dout, None, gates, aux, hp, mask, wt, dgi, dgh,
                                                       dh0, ws, T, N, H), a.reps)
            row.append(f"{kind} fwd {f:7.1f} us ({f / T:5.2f}/step) bwd {bw:7.1f} us ({bw / T:5.2f}/step)")
        print(f"  N = {N:2d}: " + " | ".join(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=5)        # IL.batch_size
    ap.add_argument("--rollout-steps", type=int, default=100)
    ap.add_argument("--steps", type=int, default=40, help="timed update steps per arm (>= 30)")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--kernels-only", action="store_true", help="only the two rollout launches alone")
    a = ap.parse_args()
    assert a.steps >= 30, "the medians are of at least 30 steps per arm"
    dev = torch.device("cuda:0")
    lib = ops.L()
    if not a.kernels_only:
        update_ab(a, dev, lib, graphs=True)
        update_ab(a, dev, lib, graphs=False)
    kernels(a, dev, lib)


if __name__ == "__main__":
    main()
