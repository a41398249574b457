"""TEST INFRASTRUCTURE ONLY.  hostsim.HostSim plus the two entry points of csrc/traj.hip
(DAgger rollout collection), written in numpy: the contract of HipLib.traj_append /
HipLib.dagger_mix_actions on CPU tensors, so data_path.TrajectoryRecorder and
data_path.dagger_step can be exercised without a GPU."""
import numpy as np
import torch

import hostsim

_NP = {torch.float16: np.float16, torch.float32: np.float32, torch.int64: np.int64}


class HostSimTraj(hostsim.HostSim):
    name = "hostsim_traj"

    def traj_append(self, sources, arenas, slots, steps):
        """row r of sources[k] -> arenas[k][slots[r], steps[r]], flattened in the row's own
        element order; every source goes through float32 on its way to float16 (batch_obs casts
        to float, astype(np.float16) then narrows)"""
        assert len(sources) == len(arenas) and len(slots) == len(steps) > 0
        for src, dst in zip(sources, arenas):
            assert src.dtype in (torch.float32, torch.int64, torch.uint8), src.dtype
            assert dst.dim() == 3 and dst.is_contiguous() and src.size(0) == len(slots)
            rows = src.detach().numpy().reshape(len(slots), -1)
            assert rows.shape[1] == dst.size(2)
            with np.errstate(over="ignore", invalid="ignore"):
                if dst.dtype == torch.float16:
                    rows = rows.astype(np.float32)
                rows = rows.astype(_NP[dst.dtype])
            out = dst.numpy()   # shares the arena's memory
            for r, (slot, step) in enumerate(zip(slots, steps)):
                assert 0 <= slot < dst.size(0) and 0 <= step < dst.size(1)
                out[slot, step] = rows[r]

    def dagger_mix_actions(self, actions, expert, uniform, beta, prev_actions, stepped):
        e = expert.numpy().astype(np.int64)
        a = np.where(uniform.numpy() < np.float32(beta), e, actions.numpy())
        skip = e == -1
        a = np.where(skip, 0, a)
        prev_actions.numpy()[...] = a
        stepped.numpy()[0] = a
        stepped.numpy()[1] = skip
