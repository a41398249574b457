"""Independent fp64 reference of the single-query attention family (csrc/attn.hip), the mirror of
its three path predicates, and THE case table of tests/test_attention_fp64_gpu.py.

Plain torch on the CPU in float64; it shares no code with tests/hostsim.py.  The functions take the
layout arguments of the entry points (row pitches ld*, kv_index, which outputs are wanted):

    s[i]   = <q, K[i]>                                   in fp64
    mode 1 : masked entries only  s <- fp64(fl32(fl32(s) - 1e8))
             -- the fp32 step of the modelled project (logits - mask.float() * 1e8 on fp32 logits).
             fp32 numbers near 1e8 are 8 apart, so every |s| < 4 is absorbed into exactly -1e8 and
             a FULLY masked row comes out as the uniform average of V.  A plain fp64 "s - 1e8"
             keeps the differences between the logits and gives something else; the contract at
             that edge is the fp32 one.  Unmasked entries stay as they are.
    mode 2 : s <- s * mask                               (multiplicative: 0 flattens, 1 keeps)
    mode 0 : the mask is ignored
    a      = softmax(s * scale),   out = sum_i a[i] V[i]

The backward is written out by formula from a GIVEN a (autograd cannot see through the fp32 step):

    dV[i] = a[i] dout      da[i] = <dout, V[i]>      dl = a (da - sum_i a da) scale
    mode 2: dl <- dl * mask      dK[i] = dl[i] q      dq = sum_i dl[i] K[i]

and, for the shared form (kv_index), the per-block sums of dK and dV in row order.
"""
import collections
import functools
import zlib

import torch

F64 = torch.float64
MAXP = 1024          # csrc/attn.hip: the LDS logits array


def f32(x):
    """a Python float rounded to fp32: what a `float` argument of the C ABI receives"""
    return float(torch.tensor(x, dtype=torch.float32))


def _blocks(t, n, P, D, ld):
    """the [n, P, D] fp64 values of a buffer whose rows lie ld floats apart, starting at t's first element"""
    return t.detach().as_strided((n, P, D), (P * ld, ld, 1)).to("cpu", F64)


def _gather(K, ldk, V, ldv, mask, B, P, Dk, Dv, kv_index, U):
    U = B if kv_index is None else U
    k, v = _blocks(K, U, P, Dk, ldk), _blocks(V, U, P, Dv, ldv)
    m = None if mask is None else mask.detach().cpu().reshape(U, P)
    if kv_index is not None:
        idx = kv_index.detach().cpu().long()
        assert idx.numel() == B and int(idx.min()) >= 0 and int(idx.max()) < U
        k, v = k[idx], v[idx]
        m = None if m is None else m[idx]
    return k, v, m


def logits64(q, K, ldk, mask, B, P, Dk, kv_index=None, U=None):
    """the raw fp64 logits <q, K[i]>  [B, P], before mask and scale"""
    k, _, _ = _gather(K, ldk, K, ldk, None, B, P, Dk, Dk, kv_index, U)
    return torch.einsum("bd,bpd->bp", q.detach().to("cpu", F64), k)


def attn_fwd(q, K, ldk, V, ldv, mask, mask_mode, scale, B, P, Dk, Dv, kv_index=None, U=None):
    """-> (out [B, Dv], attn [B, P]) in fp64"""
    assert 0 < P <= MAXP and mask_mode in (0, 1, 2)
    k, v, m = _gather(K, ldk, V, ldv, mask, B, P, Dk, Dv, kv_index, U)
    s = torch.einsum("bd,bpd->bp", q.detach().to("cpu", F64), k)
    if m is not None and mask_mode == 1:
        absorbed = (s.to(torch.float32) - 1e8).to(F64)      # fp32 subtraction, then back
        assert absorbed.dtype == F64
        s = torch.where(m != 0, absorbed, s)
    if m is not None and mask_mode == 2:
        s = s * m.to(F64)
    z = s * scale
    e = torch.exp(z - z.max(dim=1, keepdim=True).values)
    a = e / e.sum(dim=1, keepdim=True)
    return torch.einsum("bp,bpd->bd", a, v), a


def attn_bwd(dout, q, K, ldk, V, ldv, mask, mask_mode, scale, attn, B, P, Dk, Dv, kv_index=None, U=None,
             want=("dq", "dK", "dV")):
    """-> {dq [B, Dk], dK [B, P, Dk], dV [B, P, Dv]} of `want` in fp64, from the given attn; with
    kv_index also dKu [U, P, Dk] / dVu [U, P, Dv], the per-block sums"""
    k, v, m = _gather(K, ldk, V, ldv, mask, B, P, Dk, Dv, kv_index, U)
    a = attn.detach().to("cpu", F64).reshape(B, P)
    g = dout.detach().to("cpu", F64).reshape(B, Dv)
    qd = q.detach().to("cpu", F64).reshape(B, Dk)
    da = torch.einsum("bd,bpd->bp", g, v)
    dl = a * (da - (a * da).sum(dim=1, keepdim=True)) * scale
    if m is not None and mask_mode == 2:
        dl = dl * m.to(F64)
    res = {}
    if "dV" in want:
        res["dV"] = a.unsqueeze(2) * g.unsqueeze(1)
    if "dK" in want:
        res["dK"] = dl.unsqueeze(2) * qd.unsqueeze(1)
    if "dq" in want:
        res["dq"] = torch.einsum("bp,bpd->bd", dl, k)
    if kv_index is not None:
        for name, D in (("dK", Dk), ("dV", Dv)):
            if name in res:
                res[name + "u"] = segment_sum(res[name], kv_index, B, U, P * D).view(U, P, D)
    return res


def segment_sum(x, index, B, U, row_elems):
    """out[u] = sum of the rows b of x with index[b] == u; a block nobody points at is zeros"""
    out = torch.zeros(U, row_elems, dtype=F64)
    xd = x.detach().to("cpu", F64).reshape(B, row_elems)
    for b, u in enumerate(index.detach().cpu().tolist()):
        out[u] += xd[b]
    return out


# ------------------------------------------------------------------ path predicates
def paths(Dk, Dv, ldk, ldv, lddk, lddv, q, K, V, dout, dq, dK, dV):
    """Mirror of the three predicates of csrc/attn.hip.  q .. dV are DATA POINTERS (ints; 0 or None
    for a null output).  -> dict(vec, vec_v, vec_k: bool; strips: the t of the vec_k strip loop that
    own columns, () on the scalar path)"""
    p = lambda *xs: sum(0 if x is None else int(x) & 15 for x in xs) == 0   # noqa: E731
    null = lambda x: x is None or x == 0                                    # noqa: E731
    vec = Dk % 4 == 0 and ldk % 4 == 0 and p(K, q)
    vec_v = Dv % 4 == 0 and ldv % 4 == 0 and (null(dV) or lddv % 4 == 0) and p(V, dout, dV)
    vec_k = (Dk % 4 == 0 and ldk % 4 == 0 and (null(dK) or lddk % 4 == 0) and Dk <= 1024
             and p(K, q, dK, dq))
    strips = tuple(t for t in range(4) if t * 256 < Dk) if vec_k else ()
    return dict(vec=vec, vec_v=vec_v, vec_k=vec_k, strips=strips)


def path_code(pt):
    """'vvv' .. 'sss': forward dot product, backward V pass, backward K pass"""
    return "".join("v" if pt[k] else "s" for k in ("vec", "vec_v", "vec_k"))


# ------------------------------------------------------------------ the case table
NULL_PATTERNS = (("attn",), ("dq",), ("dK",), ("dV",), ("dK", "dV"))
OFFSETTABLE = ("q", "K", "V", "dout", "dq", "dK", "dV")

Case = collections.namedtuple(
    "Case", "id group B U P Dk Dv mode layout nulls mask full scale qs ks ds index path")
Case.__doc__ = """One attention problem.
    U, index: None for the plain form; else the number of K / V / mask blocks and kv_index (B ints)
    layout:   contig | kv (K and V the two column ranges of one [U, P, Dk+Dv] tensor, dK and dV of
              one dkv) | pad (every K / V / dK / dV row 4 floats longer than its width) |
              off:<names> (the named buffers start one float off a 16-byte boundary) |
              nullld (null dK / dV passed with a pitch of 1)
    nulls:    outputs passed as null, of attn / dq / dK / dV
    mask:     None | partial | full (partial, and block `full` fully masked: all 1 in mode 1 with the
              queries of that block scaled to max |s| = 1.5, all 0 in mode 2)
    qs/ks/ds: factors on q, K and dout
    path:     stated paths, checked against paths() on the buffers actually passed"""


def _c(group, path, B=2, P=7, Dk=8, Dv=8, mode=0, layout="contig", nulls=(), mask=None, full=None,
       U=None, index=None, scale=None, qs=1.0, ks=1.0, ds=1.0):
    if mode and mask is None:
        mask = "partial"
    cid = f"{group}-B{B}-P{P}-Dk{Dk}-Dv{Dv}-m{mode}-{layout}"
    if U is not None:
        cid += f"-U{U}i" + "".join(map(str, index))
    if nulls:
        cid += "-no_" + "_".join(nulls)
    if mask == "full":
        cid += f"-full{full}"
    if mode == 0 and mask:
        cid += "-ignoredmask"
    if (scale, qs, ks, ds) != (None, 1.0, 1.0, 1.0):
        cid += f"-s{scale}q{qs}k{ks}d{ds}"
    scale = f32(Dk ** -0.5 if scale is None else scale)
    return Case(cid, group, B, U, P, Dk, Dv, mode, layout, tuple(nulls), mask, full, scale, qs, ks, ds,
                None if index is None else tuple(index), path)


P_EDGES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024)
DK_VEC, DK_SCALAR = (4, 252, 256, 260, 768, 1024, 1028), (1, 6, 65, 257)
DV_VEC, DV_SCALAR = (4, 256, 260, 1028), (1, 6, 257)
KV_SPLITS = ((128, 128), (8, 6), (6, 10))
SEG_INDEX = (3, 0, 3, 3, 0)          # U = 5: unsorted, blocks 1, 2 and 4 unattended
SEG_ROW_ELEMS = (4, 1020, 1024, 1028, 4100)


@functools.lru_cache(maxsize=None)
def cases():
    cs = []
    # P: the block-stride loops over the logits take 1 / 1+ / 4 trips; P < 4 leaves waves without a row
    for P in P_EDGES:
        for mode in (0, 1, 2):
            cs.append(_c("P", "vvv", P=P, mode=mode))
    # Dk: float4 dot product (second trip above 256 columns), strips t of the backward, the Dk > 1024
    # fallback of the backward to the scalar loop; then the scalar path proper
    for i, Dk in enumerate(DK_VEC):
        cs.append(_c("Dk", "vvv" if Dk <= 1024 else "vvs", Dk=Dk, mode=i % 3))
    for i, Dk in enumerate(DK_SCALAR):
        cs.append(_c("Dk", "svs", Dk=Dk, mode=(i + 1) % 3))
    for i, Dv in enumerate(DV_VEC):
        cs.append(_c("Dv", "vvv", Dv=Dv, mode=i % 3))
    for i, Dv in enumerate(DV_SCALAR):
        cs.append(_c("Dv", "vsv", Dv=Dv, mode=(i + 1) % 3))
    # vec_k and vec_v disagree
    cs += [_c("mixed", "vsv", Dk=8, Dv=6, mode=1), _c("mixed", "svs", Dk=6, Dv=8, mode=2),
           _c("mixed", "vvs", Dk=1028, Dv=8, mode=1)]
    # layouts
    for (dk, dv), path in zip(KV_SPLITS, ("vvv", "sss", "sss")):
        for mode in (0, 1):
            cs.append(_c("layout", path, B=3, P=9, Dk=dk, Dv=dv, mode=mode, layout="kv"))
    cs += [_c("layout", "vvv", layout="pad", mode=1), _c("layout", "sss", Dk=6, Dv=6, layout="pad", mode=2),
           _c("layout", "vvv", Dk=260, Dv=260, layout="pad")]
    off_paths = dict(q="svs", K="svs", V="vsv", dout="vsv", dq="vvs", dK="vvs", dV="vsv")
    for i, name in enumerate(OFFSETTABLE):     # one misaligned pointer each: the alignment term alone decides
        cs.append(_c("layout", off_paths[name], Dk=260, Dv=260, layout="off:" + name, mode=i % 3))
    cs += [_c("layout", "sss", layout="off:K,V", mode=1), _c("layout", "vss", layout="off:dq,dK,dV", mode=2)]
    # null outputs, on a vector and on a scalar case
    for nulls in NULL_PATTERNS:
        cs.append(_c("null", "vvv", P=9, Dk=260, Dv=260, mode=1, nulls=nulls))
        cs.append(_c("null", "sss", P=9, Dk=6, Dv=6, mode=2, nulls=nulls))
    cs.append(_c("null", "vvv", nulls=("dK", "dV"), layout="nullld"))   # the pitch of a null output is not looked at
    # masks
    cs += [_c("mask", "vvv", B=3, P=37, Dk=64, mode=1, mask="full", full=1, qs=0.1),
           _c("mask", "vvv", B=3, P=300, mode=1, mask="full", full=2),
           _c("mask", "sss", B=3, P=37, Dk=6, Dv=6, mode=1, mask="full", full=0),
           _c("mask", "vvv", B=3, P=37, Dk=64, mode=2, mask="full", full=1),
           _c("mask", "sss", B=3, P=37, Dk=6, Dv=6, mode=2, mask="full", full=2),
           _c("mask", "vvv", B=3, P=37, mode=0, mask="partial")]
    # conditioning
    cs += [_c("cond", "vvv", B=3, P=37, Dk=64, scale=1.0, qs=4.0, ks=4.0),
           _c("cond", "vvv", B=3, P=37, Dk=64, mode=1, ds=1e-20),
           _c("cond", "vvv", B=3, P=37, Dk=64, mode=2, ds=1e20)]
    # shared K / V / mask blocks (P * Dk and P * Dv multiples of 4: vlnce_segment_sum's rows)
    cs += [_c("shared", "vvv", B=5, U=5, index=SEG_INDEX, P=6, mode=1),
           _c("shared", "vsv", B=5, U=5, index=SEG_INDEX, P=6, Dk=260, Dv=6, mode=2),
           _c("shared", "vvv", B=5, U=5, index=SEG_INDEX, P=300, mode=1),
           _c("shared", "vvv", B=2, U=4, index=(2, 1), P=6, mode=2),
           _c("shared", "vvv", B=1, U=3, index=(1,), P=6),
           _c("shared", "vvv", B=4, U=1, index=(0, 0, 0, 0), P=6, mode=1),
           _c("shared", "vvv", B=5, U=5, index=SEG_INDEX, P=6, mode=2, mask="full", full=3),
           _c("shared", "vvv", B=5, U=5, index=SEG_INDEX, P=6, mode=1, mask="full", full=0)]
    return tuple(cs)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def blocks_of(case):
    """kv block of every query row"""
    return list(case.index) if case.index is not None else list(range(case.B))


def full_rows(case):
    """the query rows whose block is fully masked"""
    return [b for b, u in enumerate(blocks_of(case)) if case.mask == "full" and u == case.full]


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """fp32 CPU inputs of a case in their LOGICAL shapes: q [B, Dk], K [U, P, Dk], V [U, P, Dv],
    dout [B, Dv], mask uint8 [U, P] or None, index int64 [B] or None (cached: never modified)"""
    B, P, Dk, Dv = case.B, case.P, case.Dk, case.Dv
    U = case.U if case.U is not None else B
    g = _gen("attention", case.id)
    n = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    inp = dict(q=n(B, Dk) * case.qs, K=n(U, P, Dk) * case.ks, V=n(U, P, Dv), dout=n(B, Dv) * case.ds,
               mask=None, index=None if case.index is None else torch.tensor(case.index, dtype=torch.int64))
    if case.mask:
        m = (torch.rand(U, P, generator=g) < 0.4).to(torch.uint8)
        pos = torch.randint(0, P, (U,), generator=g)
        # mode 1: one position of every row stays open (not always position 0); mode 2: one stays 1
        m[torch.arange(U), pos] = 1 if case.mode == 2 else 0
        if case.mask == "full":
            m[case.full] = 0 if case.mode == 2 else 1
            if case.mode == 1:
                s = logits64(inp["q"], inp["K"], Dk, None, B, P, Dk, inp["index"], U)
                for b in full_rows(case):
                    inp["q"][b] *= 1.5 / s[b].abs().max().item()
        inp["mask"] = m
    return inp
