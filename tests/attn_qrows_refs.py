"""Float64 reference, derived per-element bounds, case table and CPU emulation of the query-list attention kernels
(csrc/attention_qrows.hip, include/cm3p_attn_qrows.h), shared by tests/test_attn_qrows_kernels_gpu.py (the kernels against them) and
tests/test_attn_qrows_refs_host.py (the emulation must pass every check, wrong evaluations must fail them, the table must hold what
the GPU test states).  No GPU and no cm3p_amd import here.

On this side everything lives in the PADDED full layout - q, k, v, dO, out, dq, dk, dv [B, NH, S, 64], lse [B, NH, S] - with dO, out,
lse and dq meaningful on the listed rows only (`listed` [B, S] bool); a packed case is a right-padded one whose padding rows do not
exist on the device.  The contract restricted to a list IS the full contract with a dO that is zero off the list: dk / dv then sum
over the listed queries only and dq is zero off the list.

The bounds are tests/attention_refs.py's, unchanged: the kernels are attention_hd.hip's formulation (p and dS rounded to bf16 as MFMA
operands: 2 u; delta from the stored bf16 out; the same 64-term fp32 dot products, exp2 / log2, stored and reloaded lse), so
`_floors` and `_backward_bounds` are called as they stand with a dO that is zero off the list - every term of a bound carries a
factor |dO[q]| or dS[q], so unlisted queries contribute nothing.  Two paths differ from the band kernels and are counted here:
  - delta is a tree of eight 8-term chains instead of one 64-term chain: fewer roundings, inside edp's 70 U;
  - with rotary tables the kernels rotate the scaled fp32 accumulators and round ONCE: the rounding of the store is relative to the
    rotated value, |a cos + b sin| <= R(|x|) with R(x)[d] = x[d] |cos| + x[d +- 32] |sin| (attn_row_refs.rot_abs), so the bound is
    R(bound) plus the fp32 products of the rotation, 8 U R(|x|) as tests/attn_row_refs.py counts them.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

import attention_refs as AR
from attention_refs import D, LN2, LOG2E, NH, SCALE, SOFTMAX_Q_SCALE
from attn_row_refs import rot_abs, unrotate
from row_kernel_refs import FTZ, SECOND, U

B = 2
COUNTS = (0, 1, 31, 32, 33, 128, 129)
SEQS = (33, 128, 160)
WINDOWS = (-1, 0, 16, 64)


@dataclass(frozen=True)
class Case:
    S: int
    window: int                   # -1: global
    kinds: tuple                  # per sequence: "none" | "row0" | "last" | "all" | "third" | ("n", count) | "padq" | "far"
    mask: str = "none"            # none | pad (right padding, `lens`) | hole (key S // 2 of sequence 0 masked)
    lens: Optional[tuple] = None  # pad: valid keys per sequence; packed: the sequences' lengths
    pre: bool = False
    rope: Optional[str] = None    # None | "shared" (pos_batch_stride 0) | "batch" (pos_batch_stride S); packed: per-token tables
    packed: bool = False
    peaked: bool = False          # k = q on every row: nearly one-hot softmax rows, where the rounding of out matters most to delta

    @property
    def name(self):
        ks = "+".join(k if isinstance(k, str) else f"n{k[1]}" for k in self.kinds)
        return (f"S{self.S}-w{self.window}-{ks}-{self.mask}{'' if not self.lens else '-' + 'x'.join(map(str, self.lens))}-"
                f"{'pre' if self.pre else 'plain'}-{self.rope or 'norope'}{'-packed' if self.packed else ''}{'-peaked' if self.peaked else ''}")


TABLE = [
    Case(33, -1, ("all", ("n", 1))),
    Case(33, 0, ("row0", "last"), pre=True, rope="shared"),
    Case(33, 16, (("n", 31), ("n", 32)), rope="batch"),
    Case(33, 64, (("n", 33), "third"), pre=True),
    Case(128, -1, ("all", "third"), pre=True, rope="batch"),
    Case(128, 16, ("far", ("n", 33)), "pad", (40, 128), rope="shared"),
    Case(128, 0, ("third", "all"), pre=True),
    Case(128, 64, ("padq", "last"), "hole", rope="batch"),
    Case(128, -1, ("padq", "all"), "hole", pre=True),
    Case(128, 16, ("row0", "row0")),
    Case(160, -1, ("none", ("n", 129)), rope="shared"),
    Case(160, 16, (("n", 129), "none"), pre=True, rope="batch"),
    Case(160, 64, ("all", ("n", 128))),
    Case(160, 0, (("n", 0), "third"), pre=True, rope="shared"),
    Case(160, -1, ("row0", "row0"), "pad", (160, 70), pre=True, rope="shared"),
    Case(160, -1, ("none", "third"), lens=(0, 160), pre=True, rope="batch", packed=True),
    Case(160, 16, ("all", ("n", 31)), lens=(33, 160), packed=True),
    Case(128, 64, (("n", 32), "none"), lens=(128, 0), pre=True, packed=True),
    Case(33, -1, ("all", "row0"), peaked=True),
    Case(33, -1, ("all", "third"), pre=True, rope="shared", peaked=True),
]
BY_NAME = {c.name: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)


# ================================================================================================ data
def seq_len(case, b):
    """rows of sequence b that exist (queries may sit on any of them, valid key or not)."""
    return case.lens[b] if case.packed else case.S


@functools.lru_cache(maxsize=None)
def positions(case, b):
    """The listed positions of sequence b, ascending."""
    kind, L = case.kinds[b], seq_len(case, b)
    if kind == "none" or L == 0:
        return ()
    if kind == "row0":
        return (0,)
    if kind == "last":
        return (L - 1,)
    if kind == "all":
        return tuple(range(L))
    if kind == "third":
        return tuple(range(0, L, 3))
    if kind == "padq":    # every third row and the row whose own key is masked
        return tuple(sorted(set(range(0, L, 3)) | {case.S // 2}))
    if kind == "far":     # valid keys 0 .. lens[b] - 1; the query at lens[b] + window sees none of them
        return (0, 5, case.lens[b] + case.window, L - 1)
    n = kind[1]
    g = torch.Generator().manual_seed(911 + 7 * case.S + 13 * n + b)
    return tuple(sorted(torch.randperm(L, generator=g)[:n].tolist()))


def listed(case):
    m = torch.zeros(B, case.S, dtype=torch.bool)
    for b in range(B):
        m[b, list(positions(case, b))] = True
    return m


def key_mask(case):
    """bool [B, S] (True = valid key) as the DEVICE gets it, or None (also for packed cases)."""
    if case.packed or case.mask == "none":
        return None
    if case.mask == "pad":
        return torch.arange(case.S)[None] < torch.tensor(case.lens)[:, None]
    m = torch.ones(B, case.S, dtype=torch.bool)
    m[0, case.S // 2] = False
    return m


def valid_keys(case):
    """bool [B, S]: the key mask, or the rows that exist (packed)."""
    if case.packed:
        return torch.arange(case.S)[None] < torch.tensor(case.lens)[:, None]
    km = key_mask(case)
    return km if km is not None else torch.ones(B, case.S, dtype=torch.bool)


def visible(case, rule="contract"):
    """bool [B, 1, S, S]: key_mask[b, kv] != 0 and (window < 0 or |pos_q - kv| <= window).  rule: a wrong evaluation's."""
    S, w = case.S, case.window
    vis = valid_keys(case)[:, None, None, :].expand(B, 1, S, S).clone()
    i = torch.arange(S)
    if w >= 0:
        if rule == "row0_rule":          # kv <= window, the single-query kernel's rule for position 0
            vis &= (i <= w)[None, None, None, :]
        elif rule == "pos_as_index":     # the window is centred on the query's index in its sequence's list
            for b in range(B):
                for idx, pos in enumerate(positions(case, b)):
                    vis[b, 0, pos] &= (i - idx).abs() <= w
        else:
            vis &= ((i[:, None] - i[None, :]).abs() <= w)[None, None]
    if rule == "padded_query_masked":    # a query whose own key is masked is treated as absent
        vis &= valid_keys(case)[:, None, :, None]
    return vis


@functools.lru_cache(maxsize=None)
def _data(S, peaked):
    g = torch.Generator().manual_seed(8200 + 37 * S + 1000 * peaked)
    qkv = torch.randn(B, S, 3, NH, D, generator=g).to(torch.bfloat16)
    if peaked:
        qkv[:, :, 1] = qkv[:, :, 0]
    do = torch.randn(B, S, NH, D, generator=g).to(torch.bfloat16)
    ang = torch.rand(B * S, D // 2, generator=g) * (2 * math.pi)
    return qkv, do, torch.cos(ang).float(), torch.sin(ang).float()


def inputs(case):
    """-> qkv_dev bf16 [B, S, 3, NH, 64] (padded layout; pack() makes the packed one), do bf16 [B, S, NH, 64] ZERO off the list (the device
    gets its listed rows, compact), cos / sin fp32 [B * S, 32] and q, k, v float64 [B, NH, S, 64] as the reference takes them."""
    qkv, do, cos, sin = _data(case.S, case.peaked)
    qkv_dev = qkv
    q = qkv[:, :, 0].double()
    if case.pre:
        qkv_dev = qkv.clone()
        qkv_dev[:, :, 0] = (qkv[:, :, 0].float() * SOFTMAX_Q_SCALE).to(torch.bfloat16)
        q = qkv_dev[:, :, 0].double() / SOFTMAX_Q_SCALE
    do = do * listed(case)[:, :, None, None]
    return dict(qkv_dev=qkv_dev, do=do, cos=cos, sin=sin, q=AR.heads(q), k=AR.heads(qkv[:, :, 1].double()), v=AR.heads(qkv[:, :, 2].double()))


def tables(case, x):
    """cos, sin [B, 1, S, 32] as the kernels index them, or None."""
    if case.rope is None:
        return None
    S = case.S
    if case.rope == "shared" and not case.packed:
        return tuple(t[:S][None, None].expand(B, 1, -1, -1) for t in (x["cos"], x["sin"]))
    return tuple(t.view(B, 1, S, -1) for t in (x["cos"], x["sin"]))


# ================================================================================================ float64 reference and bounds
def reference(case, out_stored=None):
    """float64 autograd of softmax(scale q k^T + mask) v on all rows with a dO that is zero off the list, and the componentwise bounds
    of tests/attention_refs.py.  out_stored [B, NH, S, 64]: take delta from this out (what the kernel stored; off the list it is not
    read: dO is zero there) - the bounds then lose their delta term."""
    x = inputs(case)
    vis = visible(case)
    q, k, v = (x[n].clone().requires_grad_(True) for n in "qkv")
    s = (q @ k.transpose(-1, -2)) * SCALE
    dead = ~vis.any(-1)
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(s.masked_fill(dead[..., None], 0.0), dim=-1).masked_fill(dead[..., None], 0.0)
    o = p @ v
    do = AR.heads(x["do"].double())
    o.backward(do)
    with torch.no_grad():
        lse = torch.logsumexp(s, dim=-1).masked_fill(dead, float("-inf")).expand(-1, NH, -1).clone()
        p, out = p.detach(), o.detach()
        o_delta = out if out_stored is None else out_stored.double()
        dP = do @ x["v"].transpose(-1, -2)
        dS = p * (dP - (do * o_delta).sum(-1, keepdim=True))
        e32, ds_floor = AR._floors(None, x, vis, p, p, dS, o_delta, 1.0)
        b_out = (2.0 * AR.U16 + 3.0 * e32) * (p @ x["v"].abs()) * SECOND + FTZ
        b_dv = (2.0 * AR.U16 * (p.transpose(-1, -2) @ do.abs()) + 3.0 * ((e32 * p).transpose(-1, -2) @ do.abs())) * SECOND + FTZ
        derr = (do.abs() * b_out).sum(-1, keepdim=True) if out_stored is None else 0.0
        b_dq, b_dk, _ = AR._backward_bounds(x, p, dS, ds_floor, derr)
        if out_stored is None:
            dq, dk = q.grad, k.grad
        else:
            dq, dk = SCALE * (dS @ x["k"]), SCALE * (dS.transpose(-1, -2) @ x["q"])
        cs = tables(case, x)
        if cs is not None:
            b_dq = rot_abs(b_dq, cs) + 8.0 * U * rot_abs(dq.abs(), cs)
            b_dk = rot_abs(b_dk, cs) + 8.0 * U * rot_abs(dk.abs(), cs)
            dq, dk = unrotate(dq, cs), unrotate(dk, cs)
    lst = listed(case)[:, None, :].expand(-1, NH, -1)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=v.grad, dead=dead.expand(-1, NH, -1).clone(), listed=lst, vis=vis,
                bound=dict(out=b_out, dq=b_dq, dk=b_dk, dv=b_dv))


# ================================================================================================ the checks both test files run
def check_float64(ref, got, quantities=("out", "lse", "dq", "dk", "dv"), tag="", rel_l2=True, factor=1.0):
    """-> (measured {quantity: worst error / bound}, failures [str]).  out, lse and dq are compared on the listed rows; dk and dv on all.
    rel_l2: also hold the gradients to AR.GRAD_REL_L2 as a whole - not for the peaked cases, whose dS is small next to the rounding of
    delta by construction (the componentwise bounds carry that term)."""
    seen, fails = {}, []
    lst = ref["listed"]
    for nm in quantities:
        g, w = got[nm].double(), ref[nm]
        if nm == "lse":
            live = lst & ~ref["dead"]
            err = (g[live] - w[live]).abs()
            seen["lse_max_abs" + tag] = err.max().item() if err.numel() else 0.0
            if not bool((err <= factor * (AR.LSE_ATOL + AR.LSE_RTOL * w[live].abs())).all()):
                fails.append(f"lse{tag}: max abs error {seen['lse_max_abs' + tag]:.3e} on live listed rows")
            continue
        b = ref["bound"][nm] * factor
        if nm in ("out", "dq"):
            g, w, b = g[lst], w[lst], b[lst]
        if not g.numel():
            continue
        seen[nm + tag], nbad = AR._ratio(g, w, b)
        if nbad:
            fails.append(f"{nm}{tag}: {nbad} elements outside the bound, worst error / bound = {seen[nm + tag]:.3f}")
        if nm in ("dq", "dk", "dv") and not tag and rel_l2:
            nrm = w.norm().item()
            if nrm > 0.0:
                rel = ((g - w).norm() / nrm).item()
                seen[nm + "_rel_l2"] = rel
                if not rel < AR.GRAD_REL_L2:
                    fails.append(f"{nm}: relative L2 error {rel:.3e}")
    return seen, fails


def check_conditioned(case, got):
    """dq and dk against the float64 backward that takes delta from the out the kernels STORED, within the bounds without the delta
    term: a backward whose delta comes from anything else (the unrounded O / l, say) fails this where the softmax is nearly one-hot."""
    out = torch.where(listed(case)[:, None, :, None], got["out"].double(), torch.zeros((), dtype=torch.float64))
    return check_float64(reference(case, out_stored=out), got, ("dq", "dk"), tag="_given_out")


def check_exact(case, ref, got):
    """Listed queries without a visible key: exact zeros, lse = +inf, zero dq; live ones a finite lse; invalid keys and keys no listed
    query sees: dk = dv = 0 exactly; the q third is exactly zero off the list; nothing is NaN on the rows that exist."""
    fails = []
    lst, dead = ref["listed"], ref["dead"]
    exists = torch.stack([torch.arange(case.S) < seq_len(case, b) for b in range(B)])[:, None, :].expand(-1, NH, -1)
    for nm in ("dq", "dk", "dv"):
        if nm in got and bool(torch.isnan(got[nm].float()[exists]).any()):
            fails.append(f"{nm} has NaN")
    for nm in ("out", "lse"):
        if nm in got and bool(torch.isnan(got[nm].float()[lst]).any()):
            fails.append(f"{nm} has NaN")
    dl = lst & dead
    if dl.any():
        if not bool((got["lse"][dl] == float("inf")).all()):
            fails.append("lse of a listed query without a visible key is not +inf")
        for nm in ("out", "dq"):
            if nm in got and got[nm].float()[dl].abs().max().item() != 0.0:
                fails.append(f"{nm} of a listed query without a visible key is not exactly zero")
    if "lse" in got and not bool(torch.isfinite(got["lse"][lst & ~dead]).all()):
        fails.append("lse of a live listed query is not finite")
    unseen = ~(ref["vis"] & listed(case)[:, None, :, None]).any(-2).expand(-1, NH, -1) & exists  # keys no listed query sees
    if unseen.any():
        for nm in ("dk", "dv"):
            if nm in got and got[nm].float()[unseen].abs().max().item() != 0.0:
                fails.append(f"{nm} of a key that no listed query sees is not exactly zero")
    off = ~lst & exists
    if "dq" in got and off.any() and got["dq"].float()[off].abs().max().item() != 0.0:
        fails.append("the q third is not exactly zero off the list")
    return fails


# ================================================================================================ CPU emulation
WRONG = ("padded_query_masked", "pos_as_index", "dkdv_all_queries", "delta_unrounded", "q_third_not_zeroed", "row0_rule")


def _bf(x):
    return x.to(torch.bfloat16).float()


def _clamped_dout(case, do):
    """What a backward that walks ALL rows reads for an unlisted row: the compact dO entry its clamped slot number points at."""
    do = do.clone()
    for b in range(B):
        pos = positions(case, b)
        if not pos:
            continue
        for r in range(seq_len(case, b)):
            if r not in pos:
                do[b, :, r] = do[b, :, pos[min(sum(p < r for p in pos), len(pos) - 1)]]
    return do


def emulate(case, wrong=None):
    """A torch fp32 restatement of the kernels' documented arithmetic on the full layout (tests/attention_refs.py's emulate without
    dropout, plus the rotation of the scaled fp32 accumulators before the one bf16 store); dO is zero off the list, so the sums over
    queries are sums over the list.  wrong: one of WRONG - the same arithmetic with one mistake."""
    x = inputs(case)
    qkv = x["qkv_dev"].float()
    qd, k, v = (AR.heads(qkv[:, :, j]) for j in range(3))
    do = AR.heads(x["do"].float())
    lst = listed(case)[:, None, :, None]
    vis = visible(case, wrong if wrong in ("padded_query_masked", "pos_as_index", "row0_rule") else "contract")
    s2 = qd @ k.transpose(-1, -2)
    if not case.pre:
        s2 = s2 * SOFTMAX_Q_SCALE
    s2 = s2.masked_fill(~vis, float("-inf"))
    dead = ~vis.any(-1).expand(-1, NH, -1)
    m = s2.amax(-1, keepdim=True).masked_fill(dead[..., None], 0.0)
    pt = torch.exp2(s2 - m)
    l = pt.sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o32 = (_bf(pt) @ v) * inv
    out = o32.to(torch.bfloat16)
    lse = ((m + torch.log2(l)) * LN2)[..., 0].masked_fill(dead, float("inf"))

    p = torch.exp2(s2 - (lse * LOG2E)[..., None]).masked_fill(~vis, 0.0).masked_fill(dead[..., None], 0.0)
    if wrong in ("dkdv_all_queries", "q_third_not_zeroed"):
        do_all = _clamped_dout(case, do)
        do_kv = do_all if wrong == "dkdv_all_queries" else do
        do_q = do_all if wrong == "q_third_not_zeroed" else do
    else:
        do_kv = do_q = do

    def ds_of(g):
        delta = (g * (o32 if wrong == "delta_unrounded" else out.float())).sum(-1, keepdim=True)
        return _bf(p * (g @ v.transpose(-1, -2) - delta))

    cs = tables(case, x)
    dq32 = (ds_of(do_q) @ k) * SCALE
    dk32 = (ds_of(do_kv).transpose(-1, -2) @ qd) * (LN2 if case.pre else SCALE)
    dq = unrotate(dq32, cs).to(torch.bfloat16)
    if wrong != "q_third_not_zeroed":
        dq = torch.where(lst, dq, torch.zeros((), dtype=torch.bfloat16))
    dk = unrotate(dk32, cs).to(torch.bfloat16)
    dv = (_bf(p).transpose(-1, -2) @ do_kv).to(torch.bfloat16)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


# ================================================================================================ layouts
heads_of = AR.heads  # [B, S, NH, D] -> [B, NH, S, D]


def cu_seqlens(case):
    return [0] + torch.tensor(case.lens).cumsum(0).tolist()


def row_list(case):
    """-> (qrows: global row numbers, ascending; qcu: [B + 1]; qmax) as the device gets them."""
    base = cu_seqlens(case) if case.packed else [b * case.S for b in range(B)]
    rows, qcu = [], [0]
    for b in range(B):
        rows += [base[b] + p for p in positions(case, b)]
        qcu.append(len(rows))
    return rows, qcu, max(len(positions(case, b)) for b in range(B))


def pack(case, t):
    """[B, S, ...] -> the packed rows [total, ...] of a packed case."""
    return torch.cat([t[b, :n] for b, n in enumerate(case.lens)], 0)


def unpack_rows(case, t):
    """packed [total, ...] -> [B, S, ...], zeros behind each sequence."""
    out = t.new_zeros((B, case.S) + tuple(t.shape[1:]))
    o = 0
    for b, n in enumerate(case.lens):
        out[b, :n] = t[o:o + n]
        o += n
    return out


def compact(case, t):
    """[B, S, ...] -> the listed rows [n, ...] in list order."""
    parts = [t[b, list(positions(case, b))] for b in range(B)]
    return torch.cat(parts, 0)


def spread(case, t):
    """compact [n, ...] -> [B, S, ...], zeros off the list."""
    out = t.new_zeros((B, case.S) + tuple(t.shape[1:]))
    o = 0
    for b in range(B):
        pos = list(positions(case, b))
        out[b, pos] = t[o:o + len(pos)]
        o += len(pos)
    return out
