"""Float64 reference, derived per-element bounds, case table and CPU emulation of the single-query attention kernels
(csrc/attention_row.hip, include/cm3p_attn_row.h), shared by tests/test_attn_row_kernels_gpu.py (the kernels against them) and
tests/test_attn_row_refs_host.py (the emulation must pass every check, wrong evaluations must fail them).  No GPU and no cm3p_amd
import here.

One query - position 0 - per (sequence, head).  On this side q, dO, out, dq are [B, NH, 64], k, v, dk, dv [B, NH, S, 64], lse [B, NH].

The bounds, counted from the kernel's rounding path (its file header).  u = 2^-8 (bf16), U = 2^-24 (fp32), SECOND = 1 + 1e-3 for the
products of first-order terms (tests/row_kernel_refs.py).  p is the softmax row, dP = dO . v[kv], delta = sum_d dO out,
dS = p (dP - delta), R(x) the inverse rotation applied to magnitudes: R(x)[d] = x[d] |cos| + x[d +- 32] |sin| (x itself without tables).

  out   u p|V|              ONE bf16 rounding, the store of acc / l: p is not rounded to bf16 before it multiplies v (the band kernels
                            round it for the MFMA and pay 2 u).
  lse   e32 + 2 U |lse|     absolute, natural-log units (the floors below).
  dv    u p |dO|            the store of p * dO.
  dk    u |dk| + R(scale (p derr + floor) |q|)      the store; delta is taken from the ROUNDED out and is off by at most
                            derr = sum_d |dO[d]| bound_out[d], which enters dS as p derr.  dS itself is never rounded to bf16.
  dq    u |dq| + R(scale sum_kv (p derr + floor) |k|) + nsum U R(scale sum |dS||k|)      the store, the same delta term, and the fp32
                            summation over the keys: a group's chain of ceil(len / 32) fused multiply-adds, three butterfly steps and
                            the four waves, and the scale / rotation products behind it - nsum = ceil(len / 32) + 16.

fp32 floors, as tests/attention_refs.py counts them for the band kernels (the same 64-term fp32 dot product, the same exp2 / log2, the
stored and reloaded lse): a RELATIVE error of p and of every p-weighted sum of at most e32 = U (136 Amax + n_vis + 40), taken three
times wherever a bound has a p in it, Amax the largest scale |q|.|k| over the visible keys; dP - delta is two 64-term dot products,
edp[kv] = 70 U (|dO|.|v[kv]| + sum_d |dO out|); so dS carries the absolute floor p edp + 3 e32 |dS|.  Rotation and the two fp32
products in front of it: 8 U R(|dk|).  Pre-scaled q: the device's q' = bf16(q scale log2 e) IS the input, the reference takes
q = q' / (scale log2 e) in float64, and ln 2 q' = scale q up to one fp32 rounding (inside the 8 U).
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

from row_kernel_refs import FTZ, SECOND, U

D, SCALE = 64, 0.125
LOG2E = 1.4426950408889634
LN2 = 0.69314718055994531
SOFTMAX_Q_SCALE = SCALE * LOG2E
U16 = 2.0 ** -8
GRAD_REL_L2 = 1e-2
BWD_GROUPS = 32  # csrc/attention_row.hip: kBwdThreads / 8


@dataclass(frozen=True)
class Case:
    S: int
    nh: int
    window: int                  # -1: global
    mask: str = "none"           # none | pad (right padding, `lens`) | key0 (key 0 masked, later keys visible) | dead (sequence 1: no visible key)
    lens: Optional[tuple] = None  # pad: valid keys per sequence; packed: the sequences' lengths
    pre: bool = False
    rope: Optional[str] = None   # None | "shared" (pos_batch_stride 0) | "batch" (pos_batch_stride S); packed: per-token tables
    packed: bool = False
    peaked: bool = False         # k[0] = q: a nearly one-hot softmax, where the rounding of out matters most to delta

    @property
    def B(self):
        return len(self.lens) if self.lens else 2

    @property
    def name(self):
        return (f"S{self.S}-nh{self.nh}-w{self.window}-{self.mask}{'' if not self.lens else '-' + 'x'.join(map(str, self.lens))}-"
                f"{'pre' if self.pre else 'plain'}-{self.rope or 'norope'}{'-packed' if self.packed else ''}{'-peaked' if self.peaked else ''}")


SEQ = (1, 2, 63, 64, 65, 255, 256, 257, 1000)


def _table():
    t = []
    for i, S in enumerate(SEQ):  # the wave / workgroup seams of the key loop, nh in {1, 3}, both q modes, the three table forms
        t.append(Case(S, 1 + 2 * (i % 2), -1, pre=bool(i % 2), rope=(None, "shared", "batch")[i % 3]))
        t.append(Case(S, 3 - 2 * (i % 2), -1, pre=not i % 2, rope=("batch", None, "shared")[i % 3]))
    for S in (65, 257):          # every window edge
        for j, w in enumerate((0, 1, 63, 64, 65, S)):
            t.append(Case(S, 1 + 2 * (j % 2), w, pre=bool(j % 2), rope=("shared", None)[j % 2]))
    t.append(Case(1000, 3, 64, pre=True, rope="batch"))
    t.append(Case(257, 3, -1, "pad", (257, 130, 1), pre=True, rope="batch"))    # right padding down to one valid key
    t.append(Case(257, 1, 64, "pad", (65, 64, 1), pre=False, rope="shared"))
    t.append(Case(257, 3, -1, "key0", pre=True, rope="shared"))                 # key 0 masked, later keys visible
    t.append(Case(65, 1, 1, "key0", pre=False))
    t.append(Case(257, 3, -1, "dead", pre=True, rope="batch"))                  # a sequence with no visible key
    t.append(Case(65, 1, 0, "key0", pre=False, rope="shared"))                  # window 0 and key 0 masked: no visible key either
    t.append(Case(257, 3, -1, lens=(1, 70, 257), pre=True, rope="batch", packed=True))   # packed lengths
    t.append(Case(257, 1, 64, lens=(1, 70, 257), pre=False, packed=True))
    t.append(Case(64, 1, -1, pre=True, rope="shared", peaked=True))
    t.append(Case(64, 3, -1, pre=False, peaked=True))
    return t


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)


# ================================================================================================ data
def seq_lens(case):
    return list(case.lens) if case.packed else [case.S] * case.B


@functools.lru_cache(maxsize=None)
def _data(S, nh, B, peaked):
    g = torch.Generator().manual_seed(7100 + 31 * S + nh + 1000 * peaked)
    qkv = torch.randn(B, S, 3, nh, D, generator=g).to(torch.bfloat16)
    if peaked:
        qkv[:, 0, 1] = qkv[:, 0, 0]
    do = torch.randn(B, nh, D, generator=g).to(torch.bfloat16)
    ang = torch.rand(B * S, D // 2, generator=g) * (2 * math.pi)
    return qkv, do, torch.cos(ang).float(), torch.sin(ang).float()


def key_mask(case):
    """bool [B, S] (True = valid key) or None."""
    S = case.S
    if case.packed or case.mask == "none":
        return None
    if case.mask == "pad":
        return torch.arange(S)[None] < torch.tensor(case.lens)[:, None]
    m = torch.ones(case.B, S, dtype=torch.bool)
    if case.mask == "key0":
        m[:, 0] = False
    elif case.mask == "dead":
        m[1] = False
    return m


def inputs(case):
    """-> qkv_dev bf16 [B, S, 3, nh, 64] (padded layout; pack() makes the packed one), do bf16 [B, nh, 64], cos / sin fp32 [B * S, 32]
    (the first S rows serve pos_batch_stride 0) and q, k, v float64 as the reference takes them."""
    qkv, do, cos, sin = _data(case.S, case.nh, case.B, case.peaked)
    qkv_dev = qkv
    q = qkv[:, 0, 0].double()
    if case.pre:
        qkv_dev = qkv.clone()
        qkv_dev[:, :, 0] = (qkv[:, :, 0].float() * SOFTMAX_Q_SCALE).to(torch.bfloat16)
        q = qkv_dev[:, 0, 0].double() / SOFTMAX_Q_SCALE
    return dict(qkv_dev=qkv_dev, do=do, cos=cos, sin=sin, q=q, k=qkv[:, :, 1].double().permute(0, 2, 1, 3), v=qkv[:, :, 2].double().permute(0, 2, 1, 3))


def visible(case):
    """bool [B, S]: key_mask[b, kv] != 0 and (window < 0 or kv <= window), and kv inside the sequence (packed)."""
    S = case.S
    vis = torch.ones(case.B, S, dtype=torch.bool)
    km = key_mask(case)
    if km is not None:
        vis &= km
    if case.window >= 0:
        vis &= (torch.arange(S) <= case.window)[None]
    if case.packed:
        vis &= torch.arange(S)[None] < torch.tensor(case.lens)[:, None]
    return vis


def tables(case, x):
    """cos, sin [B, S, 32] as the kernel indexes them, or None."""
    if case.rope is None:
        return None
    B, S = case.B, case.S
    if case.rope == "shared" and not case.packed:
        return x["cos"][:S][None].expand(B, -1, -1), x["sin"][:S][None].expand(B, -1, -1)
    return x["cos"].view(B, S, -1), x["sin"].view(B, S, -1)


def unrotate(x, cs, forward=False):
    """The inverse rotary rotation a' = a cos + b sin, b' = b cos - a sin on [..., 64] (forward=True: the rotation itself)."""
    if cs is None:
        return x
    c, s = (t.to(x.dtype) for t in cs)
    a, b = x[..., :32], x[..., 32:]
    if forward:
        s = -s
    return torch.cat([a * c + b * s, b * c - a * s], -1)


def rot_abs(x, cs):
    if cs is None:
        return x
    c, s = (t.double().abs() for t in cs)
    a, b = x[..., :32], x[..., 32:]
    return torch.cat([a * c + b * s, b * c + a * s], -1)


# ================================================================================================ float64 reference and bounds
def reference(case, out_stored=None):
    """float64 forward and backward of the one-query attention and the componentwise bounds of the module docstring.
    out_stored: take delta from this out (what the kernel stored) - the bounds then lose their delta term."""
    x = inputs(case)
    vis = visible(case)[:, None, :]                                        # [B, 1, S]
    q, k, v, do = x["q"], x["k"], x["v"], x["do"].double()
    s = SCALE * torch.einsum("bhd,bhkd->bhk", q, k)
    dead = ~vis.any(-1).expand(-1, case.nh)                                # [B, nh]
    sm = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(sm.masked_fill(dead[..., None], 0.0), -1).masked_fill(dead[..., None], 0.0).masked_fill(~vis, 0.0)
    out = torch.einsum("bhk,bhkd->bhd", p, v)
    lse = torch.logsumexp(sm, -1).masked_fill(dead, float("inf"))
    A = SCALE * torch.einsum("bhd,bhkd->bhk", q.abs(), k.abs())
    amax = A.masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    nvis = vis.sum(-1, keepdim=True).double()
    e32 = U * (136.0 * amax + nvis + 40.0)                                 # [B, nh, 1]
    pv = torch.einsum("bhk,bhkd->bhd", p, v.abs())
    b_out = (U16 + 3.0 * e32) * pv * SECOND + FTZ
    b_lse = (e32[..., 0] + 2.0 * U * lse.masked_fill(dead, 0.0).abs()) * SECOND + FTZ
    o_delta = out if out_stored is None else out_stored.double()
    delta = (do * o_delta).sum(-1, keepdim=True)                            # [B, nh, 1]
    dP = torch.einsum("bhd,bhkd->bhk", do, v)
    dS = p * (dP - delta)
    dv = p[..., None] * do[:, :, None, :]
    b_dv = (U16 + 3.0 * e32[..., None]) * dv.abs() * SECOND + FTZ
    derr = (do.abs() * b_out).sum(-1, keepdim=True) if out_stored is None else 0.0
    edp = 70.0 * U * (torch.einsum("bhd,bhkd->bhk", do.abs(), v.abs()) + (do * o_delta).abs().sum(-1, keepdim=True))
    ds_err = p * derr + p * edp + 3.0 * e32 * dS.abs()
    cs = tables(case, x)
    cs_k = None if cs is None else tuple(t[:, None] for t in cs)           # [B, 1, S, 32]
    cs_q = None if cs is None else tuple(t[:, None, 0] for t in cs)        # [B, 1, 32]
    dk_un = SCALE * dS[..., None] * q[:, :, None, :]
    dk = unrotate(dk_un, cs_k)
    b_dk = (U16 * dk.abs() + rot_abs(SCALE * ds_err[..., None] * q.abs()[:, :, None, :], cs_k) + 8.0 * U * rot_abs(dk_un.abs(), cs_k)) * SECOND + FTZ
    dq = unrotate(SCALE * torch.einsum("bhk,bhkd->bhd", dS, k), cs_q)
    nsum = max(math.ceil(n / BWD_GROUPS) for n in seq_lens(case)) + 8.0
    mag = SCALE * torch.einsum("bhk,bhkd->bhd", dS.abs(), k.abs())
    b_dq = (U16 * dq.abs() + rot_abs(SCALE * torch.einsum("bhk,bhkd->bhd", ds_err, k.abs()), cs_q) + (nsum + 8.0) * U * rot_abs(mag, cs_q)) * SECOND + FTZ
    # what tests/attention_refs.py derives for query row 0 of the band / pipelined kernels (p and dS rounded to bf16 for the MFMAs: 2 u;
    # its lse tolerance), restated on this side's shapes for the cross-checks against cm3p_attn_fwd / cm3p_attn_bwd (no tables there)
    bb_out = (2.0 * U16 + 3.0 * e32) * pv * SECOND + FTZ
    t = 2.0 * U16 * dS.abs() + p * (do.abs() * bb_out).sum(-1, keepdim=True) + p * edp + 3.0 * e32 * dS.abs()
    band = dict(out=bb_out, lse=2e-3 + 1e-4 * lse.masked_fill(dead, 0.0).abs(), dv=(2.0 * U16 + 3.0 * e32[..., None]) * dv.abs() * SECOND + FTZ,
                dq=SCALE * torch.einsum("bhk,bhkd->bhd", t, k.abs()) * SECOND + FTZ, dk=SCALE * t[..., None] * q.abs()[:, :, None, :] * SECOND + FTZ)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dead=dead, vis=vis.expand(-1, case.nh, -1),
                bound=dict(out=b_out, lse=b_lse, dq=b_dq, dk=b_dk, dv=b_dv), bound_band=band)


# ================================================================================================ the checks both test files run
def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    r = err / bound
    bad = ~(err <= bound)  # (NaN fails)
    return (float("inf") if bool(torch.isnan(r).any()) else r.max().item()), int(bad.sum())


def check_float64(ref, got, quantities=("out", "lse", "dq", "dk", "dv"), factor=1.0, tag="", rel_l2=True):
    """-> (measured {quantity: worst error / bound}, failures [str]).  rel_l2: also hold the gradients to GRAD_REL_L2 as a whole - not for
    the peaked cases, whose dS is small next to the rounding of delta by construction (the componentwise bounds carry that term)."""
    seen, fails = {}, []
    for nm in quantities:
        g, w, b = got[nm], ref[nm], ref["bound"][nm] * factor
        if nm == "lse":
            live = ~ref["dead"]
            g, w, b = g[live], w[live], b[live]
            if not g.numel():
                continue
        seen[nm + tag], nbad = _ratio(g, w, b)
        if nbad:
            fails.append(f"{nm}{tag}: {nbad} elements outside the bound, worst error / bound = {seen[nm + tag]:.3f}")
        if nm in ("dq", "dk", "dv") and not tag and rel_l2:
            n = w.norm().item()
            if n > 0.0:
                rel = ((g.double() - w).norm() / n).item()
                seen[nm + "_rel_l2"] = rel
                if not rel < GRAD_REL_L2:
                    fails.append(f"{nm}: relative L2 error {rel:.3e}")
    return seen, fails


def check_conditioned(case, got):
    """dq and dk against the float64 backward that takes delta from the out the kernel STORED, within the bounds without the delta
    term: a backward whose delta comes from anything else (the unrounded acc / l, say) fails this where the softmax is nearly one-hot."""
    cond = reference(case, out_stored=got["out"])
    return check_float64(cond, got, ("dq", "dk"), tag="_given_out")


def check_exact(case, ref, got):
    """Queries without a visible key: exact zeros, lse = +inf, all-zero dq / dk / dv; live ones a finite lse; invisible and padded keys
    dk = dv = 0 exactly; nothing is NaN."""
    fails = []
    for nm in ("out", "lse", "dq", "dk", "dv"):
        if nm in got and bool(torch.isnan(got[nm].float()).any()):
            fails.append(f"{nm} has NaN")
    dead = ref["dead"]
    if dead.any():
        if not bool((got["lse"][dead] == float("inf")).all()):
            fails.append("lse of a query without a visible key is not +inf")
        for nm in ("out", "dq", "dk", "dv"):
            if nm in got and got[nm].float()[dead].abs().max().item() != 0.0:
                fails.append(f"{nm} of a query without a visible key is not exactly zero")
    if not bool(torch.isfinite(got["lse"][~dead]).all()):
        fails.append("lse of a live query is not finite")
    off = ~ref["vis"]
    if off.any():
        for nm in ("dk", "dv"):
            if nm in got and got[nm].float()[off].abs().max().item() != 0.0:
                fails.append(f"{nm} of an invisible key is not exactly zero")
    return fails


# ================================================================================================ CPU emulation
WRONG = ("window_off_by_one", "delta_unrounded", "dq_without_q_scale", "rotation_not_inverted", "padded_key_dk")


def emulate(case, wrong=None):
    """A torch fp32 restatement of the kernels' documented arithmetic: fp32 scores of the device's q (exp2 units), the exact maximum,
    p = exp2(s - m) NOT rounded, fp32 l and acc, out = bf16(acc / l); backward p = exp2(s - lse log2 e), delta from the STORED out, fp32
    dS, one bf16 rounding per stored value.  wrong: one of WRONG - the same arithmetic with one mistake."""
    x = inputs(case)
    qkv = x["qkv_dev"].float()
    qd, k, v = qkv[:, 0, 0], qkv[:, :, 1].permute(0, 2, 1, 3), qkv[:, :, 2].permute(0, 2, 1, 3)
    do = x["do"].float()
    vis = visible(case)
    if wrong == "window_off_by_one" and case.window >= 0:
        km = key_mask(case)
        vis = (torch.arange(case.S) <= case.window + 1)[None].expand(case.B, -1).clone()
        if km is not None:
            vis &= km
        if case.packed:
            vis &= torch.arange(case.S)[None] < torch.tensor(case.lens)[:, None]
    vis = vis[:, None, :]
    s2 = torch.einsum("bhd,bhkd->bhk", qd, k)
    if not case.pre:
        s2 = s2 * SOFTMAX_Q_SCALE
    s2 = s2.masked_fill(~vis, float("-inf"))
    dead = ~vis.any(-1).expand(-1, case.nh)
    m = s2.amax(-1, keepdim=True).masked_fill(dead[..., None], 0.0)
    pt = torch.exp2(s2 - m)
    l = pt.sum(-1, keepdim=True)
    o32 = torch.where(l > 0, torch.einsum("bhk,bhkd->bhd", pt, v) / l, torch.zeros(()))
    out = o32.to(torch.bfloat16)
    lse = ((m + torch.log2(l)) * LN2)[..., 0].masked_fill(dead, float("inf"))

    p = torch.exp2(s2 - (lse * LOG2E)[..., None]).masked_fill(~vis, 0.0).masked_fill(dead[..., None], 0.0)
    delta = (do * (o32 if wrong == "delta_unrounded" else out.float())).sum(-1, keepdim=True)
    dS = p * (torch.einsum("bhd,bhkd->bhk", do, v) - delta)
    cs = tables(case, x)
    cs_k = None if cs is None else tuple(t[:, None] for t in cs)
    cs_q = None if cs is None else tuple(t[:, None, 0] for t in cs)
    fwd = wrong == "rotation_not_inverted"
    dk32 = (dS * (LN2 if case.pre else SCALE))[..., None] * qd[:, :, None, :]
    if wrong == "padded_key_dk":  # the product is stored also where the key is invisible (p = 0, but a clamped row's value leaks)
        dk32 = dk32 + (~vis)[..., None] * SCALE * qd[:, :, None, :]
    dk = unrotate(dk32, cs_k, fwd).to(torch.bfloat16)
    dq32 = torch.einsum("bhk,bhkd->bhd", dS, k) * SCALE
    if wrong == "dq_without_q_scale" and case.pre:  # the gradient w.r.t. the pre-scaled q', not w.r.t. q
        dq32 = dq32 / SOFTMAX_Q_SCALE
    dq = unrotate(dq32, cs_q, fwd).to(torch.bfloat16)
    dv = (p[..., None] * do[:, :, None, :]).to(torch.bfloat16)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


# ================================================================================================ layouts
def pack(case, t):
    """[B, S, ...] -> the packed rows [total, ...] of a packed case."""
    return torch.cat([t[b, :n] for b, n in enumerate(case.lens)], 0)


def unpack_rows(case, t):
    """packed [total, ...] -> [B, S, ...], zeros behind each sequence."""
    out = t.new_zeros((case.B, case.S) + tuple(t.shape[1:]))
    o = 0
    for b, n in enumerate(case.lens):
        out[b, :n] = t[o:o + n]
        o += n
    return out
