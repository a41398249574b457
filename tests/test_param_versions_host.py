"""CPU tier: a parameter written through its pointer must have its `_version` bumped, because every
derived weight image (`_WeightCache.conv` / `stem_s2d` / `stem7` / `bn_eval`, the
`prepare_trainable` bank, `ops.split_weights` / `ops.pack_weights`) and every captured-graph key
(`HipResNetTrunk._graph_key`, `HipResNetEncoder._graph_key`, `ActGraph._key`) is built on versions.

`vlnce_amd.optim.Adam` runs here through `AdamSim` (tests/test_fused_adam_host.py), which writes
the parameters through their storage and moves no version, as `vlnce_adam_step` does.  Everything
is deterministic CPU arithmetic: the comparisons are `torch.equal`."""
import pytest
import torch
import torch.nn as nn

import vlnce_amd
from oracle import thirdparty as tp
from test_fused_adam_host import AdamSim
from test_trainable_encoders import make_inputs
from vlnce_amd import _lib, ops
from vlnce_amd.optim import Adam
from vlnce_amd.streams import ActGraph

HW, N, LR = 64, 2, 1e-2
OVER = {"RGB_ENCODER.trainable": True, "DEPTH_ENCODER.trainable": True}


@pytest.fixture
def sim(monkeypatch):
    s = AdamSim()
    monkeypatch.setattr(_lib, "_LIB", s)
    return s


def build(sd=None):
    """CMAPolicy with both trunks trainable and the RGB BatchNorm in eval mode (the shape of
    test_trainable_encoders_host_logic[eval]); sd=None: the synthetic weights"""
    hip = vlnce_amd.build_model(vlnce_amd.make_config("CMAPolicy", **OVER),
                                *vlnce_amd.make_spaces(HW, HW))
    hip.load_state_dict(tp.synth_state_dict(hip) if sd is None else sd)
    hip.net.rgb_encoder.cnn.eval()
    return hip


def logits_of(policy, inputs):
    obs, prev, masks, h0, _ = inputs
    return policy.build_distribution(obs, h0, prev, masks).logits


def one_step(policy, opt, inputs):
    opt.zero_grad()
    logits = logits_of(policy, inputs)
    loss = (logits * inputs[4]).sum()
    loss.backward()
    opt.step()
    return loss.item()


def trunks(policy):
    """(trunk module that owns a _WeightCache and a _graph_key, its stem convolution)"""
    cnn = policy.net.rgb_encoder.cnn
    enc = policy.net.depth_encoder.visual_encoder
    return [(cnn, cnn[0]), (enc, enc.backbone.conv1[0])]


def trunk_parameter_ids(policy):
    return {id(p) for trunk, _ in trunks(policy) for p in trunk.parameters()}


def graph_keys(policy):
    cnn, enc = (t for t, _ in trunks(policy))
    return cnn._graph_key("sig"), enc._graph_key("sig")


def test_trunk_training_beyond_step_one(sim):
    """after each of three steps the stepped policy (warm caches) computes what a freshly built
    policy loaded from its state_dict (cold caches) computes: on the recorded (training) path and
    under no_grad"""
    inputs = make_inputs(N, HW)
    policy = build()
    opt = Adam([p for p in policy.parameters() if p.requires_grad], lr=LR)
    losses = []
    for k in range(3):
        losses.append(one_step(policy, opt, inputs))
        cold = build(policy.state_dict())
        warm_logits, cold_logits = logits_of(policy, inputs), logits_of(cold, inputs)
        assert torch.equal(warm_logits, cold_logits), (k, (warm_logits - cold_logits).abs().max())
        with torch.no_grad():
            warm_logits, cold_logits = logits_of(policy, inputs), logits_of(cold, inputs)
        assert torch.equal(warm_logits, cold_logits), (k, "no_grad")
    print("losses", losses)
    assert losses[0] != losses[1] != losses[2]   # the steps moved the policy


def test_a_stepped_parameter_gets_a_new_version(sim):
    inputs = make_inputs(N, HW)
    policy = build()
    params = [p for p in policy.parameters() if p.requires_grad]
    opt = Adam(params, lr=LR)
    opt.zero_grad()
    (logits_of(policy, inputs) * inputs[4]).sum().backward()
    before = [p._version for p in params]
    with_grad = [p.grad is not None for p in params]
    assert sum(with_grad) >= 161
    opt.step()
    for p, v, had in zip(params, before, with_grad):
        assert (p._version > v) if had else (p._version == v)


def test_a_parameter_without_gradient_keeps_its_version(sim):
    """the case of test_a_tensor_without_gradient_is_left_alone, with and without state"""
    torch.manual_seed(0)
    ps = [nn.Parameter(torch.randn(4099)), nn.Parameter(torch.randn(7)), nn.Parameter(torch.randn(300))]
    opt = Adam(ps, lr=LR, max_grad_norm=0.2)
    for step in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        ps[1].grad = None
        before = [p._version for p in ps]
        kept = ps[1].detach().clone()
        opt.step()
        assert ps[0]._version > before[0] and ps[2]._version > before[2]
        assert ps[1]._version == before[1] and torch.equal(ps[1], kept)
    # with state (it stepped once) and no gradient now: in the launch's table, still not written
    ps[1].grad = torch.randn_like(ps[1])
    opt.step()
    ps[1].grad = None
    before, kept = ps[1]._version, ps[1].detach().clone()
    opt.step()
    assert ps[1]._version == before and torch.equal(ps[1], kept)


def test_weight_images_follow_a_step(sim):
    """every image the trunks keep per parameter version is the stepped weight's after a step"""
    inputs = make_inputs(N, HW)
    policy = build()
    opt = Adam([p for p in policy.parameters() if p.requires_grad], lr=LR)

    def images():
        out = {}
        for trunk, stem in trunks(policy):
            trunk._cache.prepare_trainable(trunk)
            for name, conv in trunk.named_modules():
                if isinstance(conv, nn.Conv2d):
                    out[id(trunk), name] = (conv, trunk._cache.conv(conv))
            out[id(trunk), "stem_s2d"] = (stem, trunk._cache.stem_s2d(stem))
        return out

    warm = images()   # every cache holds the step-0 image now, whatever the forward itself touches
    assert len(warm) > 40
    old = {k: conv.weight.detach().clone() for k, (conv, _) in warm.items()}
    one_step(policy, opt, inputs)
    for key, (conv, image) in images().items():
        assert not torch.equal(conv.weight, old[key]), key   # it did step
        want = conv.weight.detach().permute(0, 2, 3, 1)
        if key[1] == "stem_s2d":
            want = ops.stem_weight_s2d(want.contiguous())
        assert image.shape == want.shape and torch.equal(image, want), key


def test_graph_keys_change_with_a_trunk_step_only(sim):
    inputs = make_inputs(N, HW)
    policy = build()
    in_trunk = trunk_parameter_ids(policy)
    params = [p for p in policy.parameters() if p.requires_grad]
    tail = [p for p in params if id(p) not in in_trunk]
    assert 0 < len(tail) < len(params)
    one_step(policy, Adam(tail, lr=LR), inputs)   # (sets the RGB trunk's input transform)
    k0 = graph_keys(policy)
    act = ActGraph(policy)                        # its key carries every parameter of the policy
    obs, prev, masks, h0, _ = inputs
    a0 = act._key(obs, h0, prev, masks, True)
    moved = tail[0].detach().clone()
    one_step(policy, Adam(tail, lr=LR), inputs)
    assert not torch.equal(tail[0], moved)
    assert graph_keys(policy) == k0               # only the tail stepped
    assert a0 is not None and act._key(obs, h0, prev, masks, True) != a0
    one_step(policy, Adam(params, lr=LR), inputs)
    k1 = graph_keys(policy)
    assert k1[0] != k0[0] and k1[1] != k0[1]      # both trunks stepped
