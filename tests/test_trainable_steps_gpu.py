"""GPU tier: trainable visual trunks beyond the first optimizer step.

Every derived weight image (the `prepare_trainable` bank, `_WeightCache.conv` / `stem_s2d` /
`stem7`, `ops.split_weights` / `ops.pack_weights`, folded eval BatchNorm vectors) and every
captured-graph key is built on `tensor._version`; `vlnce_amd.optim.Adam` writes the parameters
through raw pointers and has to bump the versions itself.  (a)-(c) hold the step to that on the
device; (d) follows three SGD steps against the fp64 CPU oracle (one backward pass is all
tests/test_trainable_encoders.py checks).  64 x 64 frames, 3 rows, the RGB BatchNorm in eval mode
unless a test says otherwise."""
import pytest
import torch
import torch.nn as nn

import vlnce_amd
from oracle import policy_cpu as oc
from oracle import thirdparty as tp
from test_fused_adam_gpu import compare_end_to_end
from test_trainable_encoders import make_inputs
from vlnce_amd import ops
from vlnce_amd.il_harness import update_agent
from vlnce_amd.optim import Adam

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HW, N = 64, 3
TRAINABLE = {"RGB_ENCODER.trainable": True, "DEPTH_ENCODER.trainable": True}
R18 = {"RGB_ENCODER.cnn_type": "TorchVisionResNet18", "DEPTH_ENCODER.backbone": "resnet18"}
R50 = {}   # the defaults: TorchVisionResNet50 + the ResNet-50 depth backbone


def set_train(policy, bn="eval"):
    policy.train()
    if bn == "eval":
        policy.net.rgb_encoder.cnn.eval()


def build(family, sd=None, bn="eval"):
    """the HIP CMAPolicy with both trunks trainable on the device; sd=None: the synthetic weights"""
    policy = vlnce_amd.build_model(vlnce_amd.make_config("CMAPolicy", **TRAINABLE, **family),
                                   *vlnce_amd.make_spaces(HW, HW))
    policy.load_state_dict(tp.synth_state_dict(policy) if sd is None else sd)
    policy.to(DEV)
    set_train(policy, bn)
    return policy


def batch(device=DEV, dtype=torch.float32):
    obs, prev, masks, h0, wts = make_inputs(N, HW)
    obs = {k: (v.to(device, dtype) if v.is_floating_point() else v.to(device)) for k, v in obs.items()}
    return obs, prev.to(device), masks.to(device), h0.to(device, dtype), wts.to(device, dtype)


def logits_of(policy, inputs):
    obs, prev, masks, h0, _ = inputs
    return policy.build_distribution(obs, h0, prev, masks).logits


def one_step(policy, opt, inputs):
    opt.zero_grad()
    loss = (logits_of(policy, inputs) * inputs[4]).sum()
    loss.backward()
    opt.step()
    return loss


def trainable(policy):
    return [p for p in policy.parameters() if p.requires_grad]


def trunks(policy):
    """(name, trunk module with the _WeightCache, its stem convolution)"""
    cnn = policy.net.rgb_encoder.cnn
    enc = policy.net.depth_encoder.visual_encoder
    return [("rgb", cnn, cnn[0]), ("depth", enc, enc.backbone.conv1[0])]


# ---- (a) exact weight images after a device step
def same(a, b):
    return a is not None and b is not None and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("family,bn", [(R50, "eval"), (R18, "train")],
                         ids=["resnet50-eval", "resnet18-train"])
def test_weight_images_after_a_device_step(family, bn):
    """no tolerance: after Adam.step() every image is, bit for bit, the one a cold tensor of the
    stepped weight gives (vlnce_conv2d_prepare_weights writes what the per-tensor entry points
    write: test_prepare_weights_matches_the_per_tensor_entry_points)"""
    policy, inputs = build(family, bn=bn), batch()
    opt = Adam(trainable(policy), lr=1e-2)
    for _, trunk, stem in trunks(policy):   # the stems' images are warm whatever the forward uses
        trunk._cache.conv(stem), trunk._cache.stem_s2d(stem)
        if stem.in_channels == 3:
            trunk._cache.stem7(stem)
    loss = one_step(policy, opt, inputs)    # its forward prepared the step-0 images of both trunks
    assert torch.isfinite(loss)
    fmt = ops.plane_format()
    gfmt = ops.GRAD_PLANES if fmt == ops.PLANES_F16X3 else ops.PLANES_BF16X6
    n_bank = 0
    for tname, trunk, stem in trunks(policy):
        trunk._cache.prepare_trainable(trunk)
        for name, conv in trunk.named_modules():
            if not isinstance(conv, nn.Conv2d):
                continue
            where = (tname, name, tuple(conv.weight.shape))
            w = conv.weight.detach().permute(0, 2, 3, 1).contiguous()
            image = trunk._cache.conv(conv)
            assert same(image, w), where
            if conv.in_channels % 32 or conv.out_channels % 32:
                assert conv is stem, where
                continue
            n_bank += 1
            assert same(ops.split_weights(image), ops.split_weights(w)), where
            assert same(ops.pack_weights(image), ops.pack_weights(w)), where
            wt, cold_t = image._vlnce_dgrad, w.flip(1, 2).permute(3, 1, 2, 0).contiguous()
            assert same(wt, cold_t), where
            assert same(ops.split_weights(wt, gfmt), ops.split_weights(cold_t, gfmt)), where
            assert same(ops.pack_weights(wt, gfmt), ops.pack_weights(cold_t, gfmt)), where
        w = stem.weight.detach().permute(0, 2, 3, 1).contiguous()
        assert same(trunk._cache.stem_s2d(stem), ops.stem_weight_s2d(w)), (tname, "stem_s2d")
        if stem.in_channels == 3:
            frag, sfmt = trunk._cache.stem7(stem)
            assert sfmt == fmt and same(frag, ops.stem7_pack_weights(w, fmt)), (tname, "stem7")
    # every convolution behind the stems: 52 + 53 in the ResNet-50 pair, 19 + 20 in the ResNet-18 pair
    assert n_bank == (105 if family is R50 else 39)


# ---- (b) forward after a step equals a cold policy's
# Gaps are max|a - b| / max|b| per tensor.  Measured on MI355X, cold policy against a second cold
# policy on the same weights after each of the three steps: trunk features of both encoders 0.0
# every time (so they are compared with torch.equal), logits 0.0, 0.0, 4.2e-8; ten times that is
# below the floor of 1e-6, which is the logits' tolerance.  The stepped policy against the cold one
# measured 0.0 for the features and at most 8.4e-8 for the logits.
# Conditioning: at lr 1e-2 the same comparison on an optimizer that leaves the versions alone
# (stale images, a replayed step-0 graph) measured, after the first step, gaps of 1.0 (RGB
# features), 0.87 (depth features) and 0.21 (logits).
FORWARD_TOL = 1e-6
FORWARD_LR = 1e-2


def eval_outputs(policy, inputs, calls=1):
    """trunk features of both encoders and the logits, under no_grad in eval mode; with calls=2
    the second pass replays the trunks' captured graphs"""
    obs = inputs[0]
    policy.eval()
    with torch.no_grad():
        for _ in range(calls):
            out = dict(rgb=policy.net.rgb_encoder.trunk_features(obs).clone(),
                       depth=policy.net.depth_encoder.trunk_features(obs).clone(),
                       logits=logits_of(policy, inputs).clone())
    set_train(policy)
    return out


def gaps(a, b):
    return {k: ((a[k] - b[k]).abs().max() / b[k].abs().max()).item() for k in b}


def test_forward_after_each_step_equals_a_cold_policy():
    policy, inputs = build(R18), batch()
    opt = Adam(trainable(policy), lr=FORWARD_LR)
    eval_outputs(policy, inputs, calls=2)   # the trunk graphs exist for the step-0 versions
    for k in range(3):
        assert torch.isfinite(one_step(policy, opt, inputs))
        warm = eval_outputs(policy, inputs, calls=2)
        sd = policy.state_dict()
        cold = eval_outputs(build(R18, sd), inputs)
        gap = gaps(warm, cold)
        print(f"step {k + 1}: stepped against cold {gap}")
        assert all(v.isfinite().all() for v in cold.values())
        assert torch.equal(warm["rgb"], cold["rgb"]), (k, gap)
        assert torch.equal(warm["depth"], cold["depth"]), (k, gap)
        assert gap["logits"] <= FORWARD_TOL, (k, gap)
    # reference against reference, where the tolerance comes from
    spread = gaps(eval_outputs(build(R18, sd), inputs), cold)
    print(f"cold against cold {spread}")
    assert spread["rgb"] == 0.0 and spread["depth"] == 0.0 and spread["logits"] <= FORWARD_TOL, spread


# ---- (c) device Adam against torch Adam on trainable trunks
# compare_end_to_end's rtol = atol = 1e-4 holds as it stands.  Measured on MI355X over the 73 M
# parameter and moment elements: device Adam against torch Adam max|d| 8.7e-6, torch Adam against a
# second torch Adam run of the same policy 4.4e-6 (the backward's atomics), none outside the bound;
# device Adam with the versions left alone against torch Adam 1.4e-2, 4.1 M elements outside.
def test_update_agent_three_steps_against_torch_adam_with_trainable_trunks():
    obs, prev, masks, _, _ = batch()
    g = torch.Generator().manual_seed(5)
    targets = torch.randint(0, 4, (1, N), generator=g).to(DEV)
    weights = torch.ones(1, N, device=DEV)
    policy, ref = build(R18), build(R18)
    hs = policy.net.model_config.STATE_ENCODER.hidden_size
    opt = Adam(trainable(policy), lr=2.5e-4)
    ropt = torch.optim.Adam(trainable(ref), lr=2.5e-4, foreach=True)
    for _ in range(3):
        update_agent(policy, opt, obs, prev, masks, targets, weights, hs)
        update_agent(ref, ropt, obs, prev, masks, targets, weights, hs)
    in_trunk = {id(p) for _, trunk, _ in trunks(policy) for p in trunk.parameters()}
    assert sum(p in opt.state and id(p) in in_trunk for p in policy.parameters()) >= 123
    compare_end_to_end(policy, opt, ref, ropt)


# ---- (d) a training trajectory against a high-precision oracle
# lr 1e-2, measured on the CPU oracle: the median tensor's fp64 movement |p3 - p0| / |p0| is 5.3e-4,
# and the frozen-weights control 3 * lr * g1 violates the criterion for 41 of the 41 conv tensors
# (at lr 1e-4: 7.3e-6 and 29 of 41; at 1e-3: 6.5e-5 and 41 of 41).
SGD_LR = 1e-2


def oracle_trajectory(dtype, sd):
    ref = oc.CMAPolicy.from_config(tp.make_config("CMAPolicy", **TRAINABLE, **R18),
                                   *tp.make_spaces(HW, HW)).to(dtype)
    ref.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()})
    ref.net.rgb_encoder.cnn.eval()
    return sgd_trajectory(ref, batch("cpu", dtype))


def sgd_trajectory(policy, inputs):
    """three SGD steps; per parameter name: (movement p3 - p0 as fp64 on the CPU or None where no
    gradient ever arrived, p0, first gradient)"""
    named = dict(policy.named_parameters())
    p0 = {n: p.detach().clone() for n, p in named.items()}
    opt = torch.optim.SGD(trainable(policy), lr=SGD_LR)
    g1 = None
    for _ in range(3):
        one_step(policy, opt, inputs)
        if g1 is None:
            g1 = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in named.items()}
    out = {}
    for n, p in named.items():
        moved = None if g1[n] is None else (p.detach() - p0[n]).cpu().double()
        if moved is None:
            assert torch.equal(p.detach(), p0[n]), n
        out[n] = (moved, p0[n].cpu().double(), None if g1[n] is None else g1[n].cpu().double())
    return out


def test_three_sgd_steps_against_the_fp64_oracle():
    """per parameter, the movement p3 - p0 in relative L2 against the fp64 oracle's: no worse than
    3 x the fp32 oracle's own error + 5e-3 (the criterion and the denominator floor of
    test_trainable_encoders.run_pair, there for one gradient)"""
    sd = tp.synth_state_dict(vlnce_amd.build_model(
        vlnce_amd.make_config("CMAPolicy", **TRAINABLE, **R18), *vlnce_amd.make_spaces(HW, HW)))
    t64, t32 = oracle_trajectory(torch.float64, sd), oracle_trajectory(torch.float32, sd)
    moved = {n: m for n, (m, _, _) in t64.items() if m is not None}
    rms = sorted(m.norm().item() / m.numel() ** 0.5 for m in moved.values())
    scale = rms[len(rms) // 2]

    def errors(name, delta):
        t = moved[name]
        den = max(t.norm().item(), 1e-3 * scale * t.numel() ** 0.5)
        return (delta - t).norm().item() / den, (t32[name][0] - t).norm().item() / den

    # the conditions on the inputs, on the oracle alone, before anything runs on the device
    rel = sorted((m.norm() / t64[n][1].norm()).item() for n, m in moved.items())
    median = rel[len(rel) // 2]
    convs = [n for n, m in moved.items() if m.dim() == 4]
    caught = 0
    for n in convs:
        e_control, e_ref = errors(n, -3 * SGD_LR * t32[n][2])
        caught += e_control > 3 * e_ref + 5e-3
    print(f"median movement {median:.3e}; the frozen-weights control violates {caught} of {len(convs)}")
    assert 1e-4 <= median <= 1e-2
    assert 2 * caught > len(convs) >= 41

    hip = build(R18, sd)
    got = sgd_trajectory(hip, batch())
    bad, rows = [], []
    for n, (m, _, _) in t64.items():
        if m is None:
            assert got[n][0] is None, n
            continue
        assert got[n][0] is not None, n
        e_hip, e_ref = errors(n, got[n][0])
        rows.append((e_hip, e_ref, n))
        if e_hip > 3 * e_ref + 5e-3:
            bad.append((n, e_hip, e_ref))
    n_checked = len(rows)
    print("largest (e_hip, e_ref, name):", sorted(rows)[-3:])
    assert not bad, bad[:8]
    assert n_checked >= 161
