"""Independent fp64 reference of the packed-sequence LSTM / GRU layer (csrc/rnn_seq.hip).

Plain torch on the CPU in float64.  It shares no code with tests/hostsim.py and never looks at
anything a kernel saved: the forward is the textbook cell recurrence written over TIME (not over
the kernels' processing steps), the backward is torch.autograd through that same forward.

Packed semantics, as nn.LSTM / nn.GRU give them under pack_padded_sequence: row b lives at the
times t < len[b].  The forward direction walks t = 0 .. L-1, the reverse direction t = L-1 .. 0;
in either, a time t >= len[b] leaves row b's state untouched and emits zeros -- for the reverse
direction that keeps the state at zero until t = len[b]-1, which IS the walk len[b]-1 .. 0.
A row of length 0 is never alive: zeros everywhere and a zero final state (torch's own packing
rejects such a row; the kernels accept it, contract 0 <= len <= L).

Layouts are the kernels': time-major [L, B, *], gates = activated (i, f, g, o) for the LSTM and
(r, z, n) for the GRU, aux = c_t (LSTM) or W_hn h_{t-1} + b_hn (GRU).  gates / aux at dead
positions are unspecified in the kernels; here they are zeros.
"""
import torch

F64 = torch.float64


def _d(t, grad=False):
    return t.detach().to("cpu", F64).clone().requires_grad_(grad)


def _cell(kind, H, pre_x, h, c, w_hh, b_hh, leaf):
    """One step for all rows.  pre_x = gi[t]; leaf = the zero tensor added to h W_hh^T + b_hh
    (GRU only; its gradient is dgh).  Returns (h_new, c_new, gates, aux)."""
    rec = h @ w_hh.t() + b_hh
    if kind == 0:
        s = pre_x + rec
        i = torch.sigmoid(s[:, 0 * H:1 * H])
        f = torch.sigmoid(s[:, 1 * H:2 * H])
        g = torch.tanh(s[:, 2 * H:3 * H])
        o = torch.sigmoid(s[:, 3 * H:4 * H])
        c_new = f * c + i * g
        h_new = o * torch.tanh(c_new)
        return h_new, c_new, torch.cat([i, f, g, o], 1), c_new
    rec = rec + leaf
    r = torch.sigmoid(pre_x[:, 0 * H:1 * H] + rec[:, 0 * H:1 * H])
    z = torch.sigmoid(pre_x[:, 1 * H:2 * H] + rec[:, 1 * H:2 * H])
    hn = rec[:, 2 * H:3 * H]
    n = torch.tanh(pre_x[:, 2 * H:3 * H] + r * hn)
    h_new = n + z * (h - n)
    return h_new, c, torch.cat([r, z, n], 1), hn


def run(kind, dirs, H, lengths, w_hh, b_hh, *, x_tm=None, w_ih=None, b_ih=None, gi=None,
        dseq=None, dh_final=None):
    """The layer in fp64.

    kind 0 = LSTM, 1 = GRU.  lengths [B] ints in [0, L].  Per direction lists w_hh [G*H, H],
    b_hh [G*H]; the input projection is either x_tm [L*B, E] with w_ih [G*H, E], b_ih [G*H]
    (gi = x W_ih^T + b_ih), or gi [L, B, G*H] itself, or BOTH: then the forward runs on the VALUES
    of the given gi (what a kernel was fed, e.g. after fp32 rounding) while gradients still flow
    to x_tm / w_ih / b_ih through the projection.

    Returns a dict: out_tm, h_final, gates, aux (lists per direction), seq [B, L, dirs*H]; with
    dseq [B, L, dirs*H] and / or dh_final (list, entries may be None) also dgi, dgh (GRU), dw_hh,
    db_hh and -- when x_tm was given -- dw_ih, db_ih, dx [L*B, E]."""
    G = 4 if kind == 0 else 3
    lens = torch.as_tensor(lengths).to("cpu", torch.long)
    B = lens.numel()
    want_grad = dseq is not None or dh_final is not None
    w_hh = [_d(w, want_grad) for w in w_hh]
    b_hh = [_d(b, want_grad) for b in b_hh]
    have_x = x_tm is not None
    if have_x:
        x = _d(x_tm, want_grad)
        w_ih = [_d(w, want_grad) for w in w_ih]
        b_ih = [_d(b, want_grad) for b in b_ih]
        L = x.shape[0] // B
        lin = [(x @ w_ih[d].t() + b_ih[d]).view(L, B, G * H) for d in range(dirs)]
        if gi is not None:  # given values, the projection's gradient path
            gis = [_d(gi[d]).view(L, B, G * H) + (lin[d] - lin[d].detach()) for d in range(dirs)]
        else:
            gis = lin
    else:
        gis = [_d(g, want_grad) for g in gi]
        L = gis[0].shape[0]
    assert int(lens.min()) >= 0 and int(lens.max()) <= L, "contract: 0 <= len <= L"
    if want_grad and have_x:
        for g in gis:
            g.retain_grad()
    leaves = [torch.zeros(L, B, G * H, dtype=F64, requires_grad=want_grad) for _ in range(dirs)]

    res = dict(out_tm=[], h_final=[], gates=[], aux=[])
    for d in range(dirs):
        h = torch.zeros(B, H, dtype=F64)
        c = torch.zeros(B, H, dtype=F64)
        out, gates, aux = [None] * L, [None] * L, [None] * L
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            alive = (t < lens).view(B, 1)
            h_new, c_new, gt, ax = _cell(kind, H, gis[d][t], h, c, w_hh[d], b_hh[d], leaves[d][t])
            zero = torch.zeros_like(h_new)
            out[t] = torch.where(alive, h_new, zero)
            gates[t] = torch.where(alive, gt, torch.zeros_like(gt))
            aux[t] = torch.where(alive, ax, zero)
            h = torch.where(alive, h_new, h)
            c = torch.where(alive, c_new, c)
        res["out_tm"].append(torch.stack(out))
        res["h_final"].append(h)
        res["gates"].append(torch.stack(gates))
        res["aux"].append(torch.stack(aux))
    res["seq"] = torch.cat(res["out_tm"], 2).transpose(0, 1).contiguous()

    if want_grad:
        loss = torch.zeros((), dtype=F64)
        if dseq is not None:
            loss = loss + (res["seq"] * _d(dseq)).sum()
        if dh_final is not None:
            for d in range(dirs):
                if dh_final[d] is not None:
                    loss = loss + (res["h_final"][d] * _d(dh_final[d])).sum()
        wrt = list(gis) + list(w_hh) + list(b_hh) + (list(leaves) if kind == 1 else [])
        if have_x:
            wrt += [x] + list(w_ih) + list(b_ih)
        grads = torch.autograd.grad(loss, wrt, allow_unused=True)
        grads = [torch.zeros_like(w) if g is None else g for g, w in zip(grads, wrt)]
        take = lambda n: [grads.pop(0) for _ in range(n)]  # noqa: E731
        res["dgi"] = take(dirs)
        res["dw_hh"] = take(dirs)
        res["db_hh"] = take(dirs)
        if kind == 1:
            res["dgh"] = take(dirs)
        if have_x:
            res["dx"] = take(1)[0]
            res["dw_ih"] = take(dirs)
            res["db_ih"] = take(dirs)
    return {k: ([t.detach() for t in v] if isinstance(v, list) else v.detach()) for k, v in res.items()}
