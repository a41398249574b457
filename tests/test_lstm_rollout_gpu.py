"""GPU tier: the LSTM state-encoder rollout as ONE launch forward and ONE backward
(vlnce_lstm_rollout_fwd / _bwd, csrc/rnn_rollout.hip) -- the kernels against T step launches, the
autograd node and a CMA policy with STATE_ENCODER.rnn_type = LSTM taking that path, the shapes that
must not take it, and a captured graph of it."""
import pytest
import torch

import cases
import vlnce_amd
from oracle import thirdparty as tp
from vlnce_amd import _lib, ops
from vlnce_amd.il_harness import update_agent
from vlnce_amd.streams import capture_guard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    return _lib.get_lib()


def close(a, b, tol=1e-4, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max|d|={err:.3e} scale={scale:.3e} tol={tol:g}")
    assert err <= tol * scale + 1e-6, f"{what}: max|d|={err:.3e} scale={scale:.3e}"


class _Counting:
    """lib.<name> wrapped with a call counter for the duration of a `with` block."""

    def __init__(self, lib, *names):
        self.lib, self.names, self.calls = lib, names, {n: 0 for n in names}

    def __enter__(self):
        for n in self.names:
            inner = getattr(self.lib, n)

            def wrapped(*a, _inner=inner, _n=n, **k):
                self.calls[_n] += 1
                return _inner(*a, **k)

            setattr(self.lib, n, wrapped)  # an instance attribute shadows the method
        return self.calls

    def __exit__(self, *exc):
        for n in self.names:
            delattr(self.lib, n)


# ---------------------------------------------------------------- (a) kernels against step launches
@pytest.mark.parametrize("T,N,H,first", [(3, 2, 64, "zero"), (6, 1, 128, "one"), (5, 8, 64, "rand"),
                                         (9, 9, 256, "rand"), (17, 16, 512, "rand"),
                                         (100, 5, 512, "rand")])
def test_lstm_rollout_one_launch_equals_step_launches(hip, T, N, H, first):
    """vlnce_lstm_rollout_fwd / _bwd against T x vlnce_rnn_step_fwd / _bwd (lstm = 1): same saved
    tensors and gradients to fp32 rounding (only the summation order of the recurrent dot products
    differs), three repetitions on one workspace to catch an exchange that lets a workgroup read a
    stale state, then the NULL-operand forms of the backward.  vlnce_rnn_step_* has no LSTM
    instance at N = 16, H = 512 (its LDS tile holds N <= 10 episodes there): that case steps with the
    launches ops.MaskedRNNSeqFn issues for it -- mask_rows, the h W_hh^T GEMM, lstm_gates_fwd / _bwd --
    which is the same arithmetic step by step, at the same tolerances."""
    lib = hip
    assert lib.lstm_rollout_supported(N, H)
    torch.manual_seed(13)
    GH = 4 * H
    gi = (torch.randn(T, N, GH) * 0.7).to(DEV)
    h0 = (torch.randn(N, H) * 0.4).to(DEV)
    c0 = (torch.randn(N, H) * 0.6).to(DEV)
    w = (torch.randn(GH, H) * H ** -0.5).to(DEV)
    b = (torch.randn(GH) * 0.1).to(DEV)
    mask = (torch.rand(T, N) > 0.1).to(torch.uint8)
    if first == "zero":
        mask[0] = 0
    elif first == "one":
        mask[0] = 1
    mask = mask.to(DEV)
    dout = torch.randn(T, N, H).to(DEV)
    dhf = torch.randn(N, H).to(DEV)
    dcf = torch.randn(N, H).to(DEV)

    def nans(*shape):
        return torch.full(shape, float("nan"), device=DEV)

    def buffers():
        return [nans(T, N, H), nans(T, N, H), nans(T, N, GH), nans(T, N, H)]

    hp_s, out_s, gates_s, aux_s = buffers()
    fused = lib.rnn_step_supported(N, H, True)
    assert fused or (N, H) == (16, 512)
    h, c, gh = h0, c0, torch.empty(N, GH, device=DEV)
    for t in range(T):
        if fused:
            lib.rnn_step_fwd(True, gi[t], h, c, mask[t], w, b, hp_s[t], out_s[t], aux_s[t], gates_s[t], N, H)
        else:
            lib.mask_rows(h, mask[t], hp_s[t], N, H)
            lib.gemm(hp_s[t], H, 0, w, H, 0, gh, GH, N, GH, H, shift=b)
            lib.lstm_gates_fwd(gi[t], gh, c, mask[t], out_s[t], aux_s[t], gates_s[t], N, H)
        h, c = out_s[t], aux_s[t]
    wt = w.t().contiguous()
    zeros = torch.zeros(T, N, H, device=DEV)

    def step_bwd(dout_, dhf_, dcf_):
        dgi = torch.empty(T, N, GH, device=DEV)
        carry, acc = dhf_.clone(), torch.empty(N, H, device=DEV)
        dc, dc_prev = dcf_.clone(), torch.empty(N, H, device=DEV)
        for t in range(T - 1, -1, -1):
            c_prev = aux_s[t - 1] if t > 0 else c0
            if fused:
                lib.rnn_step_bwd(True, dout_[t], carry, dc, gates_s[t], aux_s[t], hp_s[t], c_prev, mask[t],
                                 wt, dgi[t], dgi[t], acc, dc_prev, N, H)
            else:
                lib.lstm_gates_bwd(dout_[t] + carry, dc, gates_s[t], c_prev, aux_s[t], mask[t], dgi[t],
                                   dc_prev, N, H)
                lib.gemm(dgi[t], GH, 0, w, H, 1, acc, H, N, H, GH)  # dh_{t-1} = m_t * (dgates W_hh)
                carry = acc * mask[t].view(N, 1).float()
            dc, dc_prev = dc_prev, dc
        return dgi, carry, dc

    dgi_s, dh0_s, dc0_s = step_bwd(dout, dhf, dcf)
    word = torch.empty(lib.lstm_rollout_workspace_bytes(N, H), dtype=torch.uint8, device=DEV)
    assert word.numel() == 2 * N * GH * 8
    for rep in range(3):
        hp_r, out_r, gates_r, aux_r = buffers()
        lib.lstm_rollout_fwd(gi, h0, c0, mask, w, b, hp_r, out_r, gates_r, aux_r, word, T, N, H)
        for a, r_, what in ((out_r, out_s, "out"), (hp_r, hp_s, "hp"), (gates_r, gates_s, "gates"),
                            (aux_r, aux_s, "aux")):
            close(a, r_, 2e-5, what=f"rollout fwd {what} (rep {rep})")
        dgi_r, dh0_r, dc0_r = nans(T, N, GH), nans(N, H), nans(N, H)
        lib.lstm_rollout_bwd(dout, dhf, dcf, gates_s, aux_s, hp_s, c0, mask, wt, dgi_r, dh0_r, dc0_r,
                             word, T, N, H)
        close(dgi_r, dgi_s, 1e-4, what=f"rollout dgi (rep {rep})")
        close(dh0_r, dh0_s, 1e-4, what=f"rollout dh0 (rep {rep})")
        close(dc0_r, dc0_s, 1e-4, what=f"rollout dc0 (rep {rep})")
    # no output gradient, no final-state gradients: NULL operands
    dgi_r, dh0_r, dc0_r = nans(T, N, GH), nans(N, H), nans(N, H)
    lib.lstm_rollout_bwd(None, None, None, gates_s, aux_s, hp_s, c0, mask, wt, dgi_r, dh0_r, dc0_r,
                         word, T, N, H)
    assert float(dgi_r.abs().max()) == 0.0
    assert float(dh0_r.abs().max()) == 0.0 and float(dc0_r.abs().max()) == 0.0
    # only the final cell state has a gradient
    dgi_s, dh0_s, dc0_s = step_bwd(zeros, torch.zeros(N, H, device=DEV), dcf)
    dgi_r, dh0_r, dc0_r = nans(T, N, GH), nans(N, H), nans(N, H)
    lib.lstm_rollout_bwd(None, None, dcf, gates_s, aux_s, hp_s, c0, mask, wt, dgi_r, dh0_r, dc0_r,
                         word, T, N, H)
    close(dgi_r, dgi_s, 1e-4, what="rollout dgi (dc_final only)")
    close(dh0_r, dh0_s, 1e-4, what="rollout dh0 (dc_final only)")
    close(dc0_r, dc0_s, 1e-4, what="rollout dc0 (dc_final only)")


# ---------------------------------------------------------------- (b), (c), (e): the autograd node
class _Rollout:
    """Seeded inputs of one masked LSTM rollout and the CPU loop of torch cells over them (the loop
    of test_kernels_gpu.test_masked_rnn_rollout_vs_torch_cells)."""

    def __init__(self, T, N, H, D=24, seed=5):
        torch.manual_seed(seed)
        self.T, self.N, self.H = T, N, H
        cell = torch.nn.LSTMCell(D, H)
        self.params = [p.detach().clone() for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih,
                                                    cell.bias_hh)]
        self.x = torch.randn(T * N, D) * 0.5
        self.h0, self.c0 = torch.randn(N, H) * 0.3, torch.randn(N, H) * 0.3
        self.masks = (torch.rand(T, N) > 0.15).to(torch.uint8)
        self.masks[0] = 0
        self.wts, self.wh, self.wc = torch.randn(T * N, H), torch.randn(N, H), torch.randn(N, H)

    def leaves(self, dev):
        return [t.detach().clone().to(dev).requires_grad_(True) for t in [self.x, self.h0, self.c0] + self.params]

    def loss(self, y, hT, cT, dev):
        return (y * self.wts.to(dev)).sum() + (hT * self.wh.to(dev)).sum() + (cT * self.wc.to(dev)).sum()

    def cpu(self):
        xs, h, c, w_ih, w_hh, b_ih, b_hh = leaves = self.leaves("cpu")
        T, N = self.T, self.N
        hh, cc, outs = h, c, []
        for t in range(T):
            m = self.masks[t].float().unsqueeze(1)
            gates = xs[t * N:(t + 1) * N] @ w_ih.t() + b_ih + (hh * m) @ w_hh.t() + b_hh
            i, f, g, o = gates.chunk(4, 1)
            cc = torch.sigmoid(f) * (cc * m) + torch.sigmoid(i) * torch.tanh(g)
            hh = torch.sigmoid(o) * torch.tanh(cc)
            outs.append(hh)
        y = torch.cat(outs)
        grads = torch.autograd.grad(self.loss(y, hh, cc, "cpu"), leaves)
        return [y.detach(), hh.detach(), cc.detach()] + [g.detach() for g in grads]

    def gpu(self):
        xs, h, c, w_ih, w_hh, b_ih, b_hh = leaves = self.leaves(DEV)
        gi = ops.linear(xs, w_ih, b_ih)
        y, hT, cT = ops.MaskedRNNSeqFn.apply(True, gi, h, c, self.masks.view(-1).to(DEV), w_hh, b_hh)
        grads = torch.autograd.grad(self.loss(y, hT, cT, DEV), leaves)
        return [y.detach(), hT.detach(), cT.detach()] + [g.detach() for g in grads]


_NAMES = ["out", "h_T", "c_T", "dx", "dh0", "dc0", "dW_ih", "dW_hh", "db_ih", "db_hh"]


def _compare(got, ref):
    for name, a, b in zip(_NAMES, got, ref):
        close(a, b, 1e-4 if name in ("out", "h_T", "c_T") else 3e-4, what=f"rollout {name}")


@pytest.fixture(scope="module")
def ref_7_3_64():
    r = _Rollout(7, 3, 64)
    return r, r.cpu()


def test_autograd_node_takes_the_one_launch_path(hip, ref_7_3_64):
    """ops.MaskedRNNSeqFn with an LSTM at a supported shape: no step launch, one rollout launch per
    direction; outputs and every gradient against torch cells stepped on the CPU."""
    r, ref = ref_7_3_64
    with _Counting(hip, "rnn_step_fwd", "rnn_step_bwd", "lstm_rollout_fwd", "lstm_rollout_bwd") as n:
        got = r.gpu()
    assert n == {"rnn_step_fwd": 0, "rnn_step_bwd": 0, "lstm_rollout_fwd": 1, "lstm_rollout_bwd": 1}, n
    _compare(got, ref)


@pytest.mark.parametrize("T,N,H", [(4, 17, 256), (5, 4, 24)])
def test_unsupported_shapes_take_the_step_path(hip, T, N, H):
    assert not hip.lstm_rollout_supported(N, H)
    r = _Rollout(T, N, H)
    with _Counting(hip, "rnn_step_fwd", "lstm_gates_fwd", "lstm_rollout_fwd", "lstm_rollout_bwd") as n:
        got = r.gpu()
    assert n["lstm_rollout_fwd"] == 0 and n["lstm_rollout_bwd"] == 0, n
    assert n["rnn_step_fwd"] + n["lstm_gates_fwd"] == T, n  # one (fused or unfused) step launch per step
    _compare(got, r.cpu())


def test_supported_refuses_and_single_step_stays_off_the_rollout(hip):
    assert not hip.lstm_rollout_supported(17, 256)
    assert not hip.lstm_rollout_supported(4, 24)
    assert not hip.lstm_rollout_supported(0, 64)
    assert hip.lstm_rollout_workspace_bytes(17, 256) == 0
    assert hip.lstm_rollout_supported(16, 512)  # the largest instance: 152 KB of LDS backward
    # T = 1 at a supported (N, H): the step kernels
    r = _Rollout(1, 3, 64)
    with _Counting(hip, "lstm_rollout_fwd", "lstm_rollout_bwd") as n:
        got = r.gpu()
    assert n == {"lstm_rollout_fwd": 0, "lstm_rollout_bwd": 0}, n
    _compare(got, r.cpu())
    # the entry point itself refuses N = 17 before it launches anything: the outputs stay as they were
    T, N, H = 2, 17, 64
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    out = torch.full((T, N, H), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported N/H"):
        hip.lstm_rollout_fwd(z(T, N, 4 * H), z(N, H), z(N, H), torch.ones(T, N, dtype=torch.uint8, device=DEV),
                             z(4 * H, H), z(4 * H), z(T, N, H), out, z(T, N, 4 * H), z(T, N, H),
                             torch.empty(1 << 16, dtype=torch.uint8, device=DEV), T, N, H)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0


def test_rollout_in_a_captured_graph(hip):
    """forward + backward of the node captured in a torch.cuda.graph (the workspace comes from the
    graph's pool) and replayed twice with new inputs, against the eager node."""
    T, N, H, D = 7, 3, 64, 24
    r = _Rollout(T, N, H)
    w_ih, w_hh, b_ih, b_hh = [p.to(DEV) for p in r.params]
    masks = r.masks.view(-1).to(DEV)
    wts, wh, wc = r.wts.to(DEV), r.wh.to(DEV), r.wc.to(DEV)

    def run(x, h0, c0):
        x, h0, c0 = [t.detach().requires_grad_(True) for t in (x, h0, c0)]
        w = w_hh.detach().requires_grad_(True)
        y, hT, cT = ops.MaskedRNNSeqFn.apply(True, ops.linear(x, w_ih, b_ih), h0, c0, masks, w, b_hh)
        loss = (y * wts).sum() + (hT * wh).sum() + (cT * wc).sum()
        return [y.detach(), cT.detach()] + list(torch.autograd.grad(loss, [x, h0, c0, w]))

    sx, sh, sc = r.x.to(DEV), r.h0.to(DEV), r.c0.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sx, sh, sc)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with _Counting(hip, "lstm_rollout_fwd", "lstm_rollout_bwd") as n:
        with capture_guard(), torch.cuda.graph(graph):
            outs = run(sx, sh, sc)
    assert n == {"lstm_rollout_fwd": 1, "lstm_rollout_bwd": 1}, n
    for seed in (21, 22):
        g = torch.Generator().manual_seed(seed)
        nx, nh, nc = (torch.randn(T * N, D, generator=g) * 0.5, torch.randn(N, H, generator=g) * 0.3,
                      torch.randn(N, H, generator=g) * 0.3)
        sx.copy_(nx)
        sh.copy_(nh)
        sc.copy_(nc)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = run(nx.to(DEV), nh.to(DEV), nc.to(DEV))
        for name, a, b in zip(("out", "c_T", "dx", "dh0", "dc0", "dW_hh"), got, want):
            # the same kernels on the same inputs: at most the order in which a GEMM's fp32 atomics
            # land differs (2^-24 per term over T*N = 21 rows), far inside 1e-5
            close(a, b, 1e-5, what=f"replay (seed {seed}) {name}")


# ---------------------------------------------------------------- (d) policy level
def test_cma_lstm_update_one_launch_equals_step_path(hip, monkeypatch):
    """One update_agent step of a CMA policy with STATE_ENCODER.rnn_type = LSTM on a T x N = 4 x 2
    batch: both state encoders through the one-launch rollout, then through the step kernels
    (lstm_rollout_supported patched on the library object); loss and every parameter gradient."""
    torch.distributions.Distribution.set_default_validate_args(False)
    case = dict(policy="CMAPolicy", hw=64, N=2, T=4, lengths=[6, 10], mode="train", call="update",
                overrides={"STATE_ENCODER.rnn_type": "LSTM"})
    obs, prev, masks, extra = cases.build_inputs(case)
    obs = {k: v.to(DEV) for k, v in obs.items()}
    prev, masks = prev.to(DEV), masks.to(DEV)
    tgt, wgt = extra["targets"].to(DEV), extra["weights"].to(DEV)

    def run():
        policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                       tp.synth_state_dict)
        policy.to(DEV)
        hs = policy.net.model_config.STATE_ENCODER.hidden_size
        with _Counting(hip, "lstm_rollout_fwd", "lstm_rollout_bwd", "rnn_step_fwd", "rnn_step_bwd") as n:
            loss, _, _ = update_agent(policy, None, obs, prev, masks, tgt, wgt, hs, step_grad=False)
        torch.cuda.synchronize()
        return loss, {k: p.grad.clone() for k, p in policy.named_parameters() if p.grad is not None}, dict(n)

    loss_r, grads_r, n_r = run()
    assert n_r == {"lstm_rollout_fwd": 2, "lstm_rollout_bwd": 2, "rnn_step_fwd": 0, "rnn_step_bwd": 0}, n_r
    monkeypatch.setattr(hip, "lstm_rollout_supported", lambda N, H: False, raising=False)
    loss_s, grads_s, n_s = run()
    assert n_s["lstm_rollout_fwd"] == 0 and n_s["rnn_step_fwd"] == 8 and n_s["rnn_step_bwd"] == 8, n_s
    print(f"loss one-launch {loss_r:.7f} step {loss_s:.7f}")
    assert abs(loss_r - loss_s) <= 1e-4 * max(abs(loss_s), 1.0)
    assert grads_r.keys() == grads_s.keys() and len(grads_r) > 20
    for k in grads_s:
        close(grads_r[k], grads_s[k], 1e-4, what=f"grad {k}")
