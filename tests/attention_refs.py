"""Float64 reference, derived per-element bounds, case table, CPU emulation and index-arithmetic restatement of the head-64 attention
kernels (csrc/attention.hip, attention_fwd.hip, attention_bwd_fused.hip), shared by tests/test_attention_d64_gpu.py (the kernels
against them) and tests/test_attention_refs_host.py (the emulation must pass every check, wrong evaluations must fail them, the table
must reach every branch of the band arithmetic).  The dropout forms (cm3p_attn_fwd_dropout / cm3p_attn_bwd_dropout and their packed
relatives) run TABLE_DROP x DROPOUT_PS with the host's Philox mask (tests/dropout_refs.py::attention_keep) in
tests/test_dropout_kernels_gpu.py; tests/test_dropout_refs_host.py holds the emulation and WRONG_DROP to them.  No GPU and no cm3p_amd
import here.

Tensors are [B, NH, S, 64] (lse: [B, NH, S]) on this side; the GPU test converts from the packed layouts.

The bounds.  u = 2^-8 is the unit roundoff of bf16 round-to-nearest, U = 2^-24 that of fp32 and SECOND = 1 + 1e-3 the factor
tests/row_kernel_refs.py gives the products of first-order terms.  Counting the roundings in the kernel sources, with P the softmax,
Z the dropout factor keep / (1 - p) (1 without dropout), dP = dO V^T, delta = rowsum(dO o out), dS = P o (Z o dP - delta):

  out  2 u (P o Z)|V|                  (1) p~ -> bf16 as the MFMA's B operand (acc_to_frag in attn_fwd_kernel; the pipelined forward
                                           packs the same way), (2) the bf16 store of O / l (store_rows32); |out| <= (P o Z)|V|.
  dv   2 u (P o Z)^T|dO|               (1) p (o Z, one fp32 product: floor) -> bf16 for dV^T += dO^T P, (2) the store.
  dq   scale (2 u |dS| + P derr)|K|    (1) dS -> bf16 for dQ^T += K^T dS^T, (2) the store, (3) delta is taken from the ROUNDED out
                                           (band_dq_block's `dlt`, the prep kernel of the fused backward): it is off by at most
                                           derr[q] = sum_d |dO[q, d]| bound_out[q, d] and enters dS as P derr.  bound_out <= 2 u (P|V|)
                                           up to its floor, so this is the form 2 u scale (|dS| + P E)|K| with E = sum_d |dO| (P|V|):
                                           the error of delta counts ONCE (it is an error of dS itself, not a value that is rounded
                                           again by (1) and (2), which are relative to |dS|).
  dk   the same with (...)^T |Q|.      Pre-scaled q: the products are taken with q' = bf16(q scale log2 e) and the store multiplies by
                                           the fp32 constant ln 2 (band_dkv_block's epilogue) - scale |q_ref| = ln 2 |q'| exactly, and one
                                           more fp32 rounding: floor.
  fused dq  + G u scale |dS||K|        cm3p_attn_bwd_fused, G = 2 or 4 key blocks per slab (cm3p_attn_bwd_fused_slab_group).  Counted in
                                           csrc/attention_bwd_fused.hip: every 256-key block's fp32 dQ^T accumulator is packed to bf16 ONCE
                                           (post_hook C == 2 / 3, pack_bf16x2), whether it is then stored (position 0 of its group) or handed
                                           to global_atomic_pk_add_bf16 as the operand (positions 1 .. G - 1): u |partial| each, together at
                                           most u scale |dS||K| over all blocks.  Each of the G - 1 adds of a group rounds the running bf16 sum
                                           once, and that sum is bounded by the sum of the |partials| so far, i.e. by the group's share of
                                           scale |dS||K|: (G - 1) u scale |dS||K|.  The reduce sums the slabs in fp32 (floor).  G = 2 gives
                                           the 2 u of the pair form.  tests/attention_fused_refs.py holds the table that runs G = 4, more
                                           than one slab, and the inverse rotation of the epilogues.

fp32 floors.  A score is a 64-term fp32 dot product (+ the reference point / -lse as initial accumulator, one fma for plain q): it
is off by at most 66 U (A + |m|) <= 132 U Amax[q] in natural-log units, A = scale |q|.|k|, Amax its maximum over the row's visible
keys; exp2 and log2 are good to 2 U; l and the O accumulation add n_vis terms; lse is stored and reloaded (times log2 e or 1 / scale:
2 U |lse|, |lse| <= Amax + ln n).  Together a RELATIVE error of p, 1 / l and every p-weighted sum of at most
    e32[q] = U (136 Amax[q] + n_vis[q] + 40),
taken three times (p, l, the accumulation) wherever a bound has a P in it.  dP - delta is two 64-term dot products:
    edp[q, k] = 70 U (zmax |dO[q]|.|V[k]| + sum_d |dO o out|)     (zmax = 1 / (1 - p): dropout's fma, else 1)
so dS carries the absolute floor P edp + 3 e32 |dS|.  With unit-variance data e32 ~ 1e-4 and edp ~ 1e-4: a few per cent of u.
"""
import functools
from dataclasses import dataclass
from typing import Optional

import torch

from row_kernel_refs import FTZ, SECOND, U

NH, D, SCALE = 2, 64, 0.125
LOG2E = 1.4426950408889634
LN2 = 0.69314718055994531
SOFTMAX_Q_SCALE = SCALE * LOG2E  # cm3p_amd.kernels.SOFTMAX_Q_SCALE restated (the GPU test compares the two)
U16 = 2.0 ** -8
LSE_ATOL, LSE_RTOL = 2e-3, 1e-4
GRAD_REL_L2 = 1e-2
PROBE_LSE_TOL = 1e-4

WINDOWS_A = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 200, 299, 300)
LENS_A = (300, 161, 1)
CASES_B = ((1, 0), (33, 200), (64, 31), (65, 1), (129, 33), (256, 65), (257, 127), (449, 96), (449, 449))
WINDOWS_C = (1, 33, 64, 96)
CASES_G = ((300, LENS_A), (449, None), (257, (257, 1)))
PROBE_WINDOWS = (0, 1, 33, 64, 129, 200)
PROBE_OUT_MAX_WINDOW = 64
C_ONE_KEY_WINDOWS = (0, 1, 64, 129)  # sequence 2 of table C: one visible key at these windows, none at the others (33, 96, 200)
C_RIGHT_PAD_WINDOWS = (33, 64, 129)  # sequence 1 of table C: right padding behind the left padding at these windows


@dataclass(frozen=True)
class Case:
    table: str             # "A", "B", "C", "G"; the probe cases carry the table whose masks they run on
    S: int
    window: int            # -1: global
    lens: Optional[tuple]  # valid lengths per sequence (right padding); None: B = 2 without a mask (tables A, B, G)
    pre: bool              # the device gets bf16(q * SOFTMAX_Q_SCALE) and q_prescaled = 1
    probe: bool = False    # q = k = 0, v = +-1 by the bits of the key index
    holes: bool = False    # table F: the five-sequence mask with holes at window -1 (_key_mask)
    nb: int = 0            # table F: the batch size of a case without a mask (0: 2)

    @property
    def name(self):
        m = "holes" if (self.table == "C" or self.holes) else ("nomask" if self.lens is None else "pad")
        return f"{'P' if self.probe else ''}{self.table}-S{self.S}-w{self.window}-{m}-{'pre' if self.pre else 'plain'}"

    @property
    def B(self):
        if self.holes:
            return 5
        return 4 if self.table == "C" else (len(self.lens) if self.lens else (self.nb or 2))


def _both(table, S, window, lens):
    return [Case(table, S, window, lens, pre) for pre in (False, True)]


TABLE_A = [c for w in WINDOWS_A for c in _both("A", 300, w, LENS_A)]
TABLE_B = [c for S, w in CASES_B for c in _both("B", S, w, None)]
TABLE_C = [c for w in WINDOWS_C for c in _both("C", 300, w, None)]
TABLE_G = [c for S, lens in CASES_G for c in _both("G", S, -1, lens)]
# the count probe: six windows on A and C in both q modes, and A's other windows with plain q (so that a window edge that
# is off by one key is counted at EVERY window of table A, also where one key among 300 moves lse by less than its tolerance)
TABLE_P = ([Case(t, 300, w, LENS_A if t == "A" else None, pre, True) for t in "AC" for w in PROBE_WINDOWS for pre in (False, True)]
           + [Case("A", 300, w, LENS_A, False, True) for w in WINDOWS_A if w not in PROBE_WINDOWS])
TABLE = TABLE_A + TABLE_B + TABLE_C + TABLE_G
BY_NAME = {c.name: c for c in TABLE + TABLE_P}
# attention-probability dropout (cm3p_attn_fwd_dropout / cm3p_attn_bwd_dropout: the band kernels at every window, -1 included): table A
# at the windows where a row sees one key (0), three (1), the tile seam (63, 64, 65) and everything (300), the holes of table C, the
# global instances of table G and the no-mask instances of table B at one tile, five and eight (the ring wraps); both q modes
WINDOWS_A_DROP = (0, 1, 63, 64, 65, 300)
CASES_B_DROP = ((64, 31), (257, 127), (449, 449))
TABLE_DROP = ([c for c in TABLE_A if c.window in WINDOWS_A_DROP] + TABLE_C + TABLE_G + [c for c in TABLE_B if (c.S, c.window) in CASES_B_DROP])
DROPOUT_PS = (0.1, 0.5)


def instances(case, drop=False):
    """The kernel instances of csrc/attention.hip a case's cm3p_attn_fwd + cm3p_attn_bwd calls run (launch_attn_fwd / launch_attn_bwd).
    drop: the _dropout entries, whose global pre-scaled forward is the band kernel too (the pipelined one has no dropout instance)."""
    masked = key_mask(case) is not None
    p = "true" if case.pre else "false"
    fwd = "attn_fwd_g_kernel" if (case.window < 0 and case.pre and not drop) else f"attn_fwd_kernel<1, {p}, {'true' if case.window >= 0 else 'false'}>"
    return {fwd, f"attn_bwd_dq_kernel<{p}, {'true' if masked else 'false'}>", f"attn_bwd_dkv_kernel<{p}>"}


# four forward, four dq, two dkv.  (attn_fwd_kernel<1, true, false> - global, pre-scaled q - is not among them: without dropout such a call
# takes the pipelined kernel, cm3p_attn_fwd_impl; tests/test_dropout_gpu.py runs it.)
ALL_INSTANCES = ({"attn_fwd_kernel<1, true, true>", "attn_fwd_kernel<1, false, true>", "attn_fwd_kernel<1, false, false>", "attn_fwd_g_kernel"}
                 | {f"attn_bwd_dq_kernel<{p}, {m}>" for p in ("true", "false") for m in ("true", "false")}
                 | {f"attn_bwd_dkv_kernel<{p}>" for p in ("true", "false")})


# ================================================================================================ data
@functools.lru_cache(maxsize=None)
def _key_mask(table, S, window, lens, holes=False):
    if holes:
        # table C's patterns at window -1 for the fused backward's long case (S >= 768): holes everywhere; left AND right padding in one
        # sequence; no valid key at all; one hole late in the sweep; only the keys of ONE 256-key block (the third) valid
        g = torch.Generator().manual_seed(4100 + S)
        m = torch.ones(5, S, dtype=torch.bool)
        m[0] = torch.rand(S, generator=g) < 0.7
        cut = 70 + int(torch.randint(0, 60, (1,), generator=g))
        m[1, :cut] = False
        m[1, cut + (S - cut) // 2:] = False
        m[2] = False
        m[3, S - 40] = False
        m[4] = False
        m[4, 512:768] = True
        return m
    if table != "C":
        return None if lens is None else torch.arange(S)[None] < torch.tensor(lens)[:, None]
    g = torch.Generator().manual_seed(4100 + S)
    m = torch.ones(4, S, dtype=torch.bool)
    m[0] = torch.rand(S, generator=g) < 0.7                # holes everywhere
    cut = 70 + int(torch.randint(0, 60, (1,), generator=g))
    m[1, :cut] = False                                     # left padding (ends inside the second key tile)
    if window in C_RIGHT_PAD_WINDOWS:
        m[1, cut + (S - cut) // 2:] = False                # ... and right padding behind it
    m[2] = False
    if window in C_ONE_KEY_WINDOWS:
        m[2, 150] = True                                   # one visible key; otherwise none at all
    m[3, S - 40] = False                                   # one hole late in the sweep
    return m


def key_mask(case):
    """bool [B, S] (True = valid key) or None."""
    return _key_mask(case.table, case.S, case.window, case.lens, case.holes)


def visible(case, km="own", rows=None):
    """The header's rule: key_mask[b, kv] != 0 and (window < 0 or |q - kv| <= window).  bool [B, 1, S, S]; rows (a LongTensor of query
    rows): [B, 1, len(rows), S], built without the S x S one."""
    km = key_mask(case) if isinstance(km, str) else km
    S = case.S
    qi = torch.arange(S) if rows is None else rows
    vis = torch.ones(case.B, 1, len(qi), S, dtype=torch.bool)
    if km is not None:
        vis = vis & km[:, None, None, :]
    if case.window >= 0:
        vis = vis & ((qi[:, None] - torch.arange(S)[None, :]).abs() <= case.window)[None, None]
    return vis


def heads(x):
    """[B, S, NH, D] -> [B, NH, S, D]"""
    return x.permute(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def _data(table, S, B, probe):
    g = torch.Generator().manual_seed(64000 + 977 * ord(table) + S)
    qkv = torch.randn(B, S, 3, NH, D, generator=g).to(torch.bfloat16)
    do = torch.randn(B, S, NH, D, generator=g).to(torch.bfloat16)
    if probe:
        qkv[:, :, :2] = 0
        bit = (torch.arange(S)[:, None] >> (torch.arange(D)[None, :] % 10)) & 1
        qkv[:, :, 2] = (1.0 - 2.0 * bit.float())[None, :, None, :].to(torch.bfloat16)  # +-1: exact in bf16
    return qkv, do


def inputs(case):
    """-> dict(qkv_dev bf16 [B, S, 3, NH, 64]: what the device gets; q, k, v float64 [B, NH, S, 64]: what the reference gets - in the
    pre-scaled mode q is the device's bf16(q * SOFTMAX_Q_SCALE) divided back, as tests/test_kernels_gpu.py::_attn_case does;
    do bf16 [B, S, NH, 64]).  One draw per (table, S): the windows of a table and both q modes share their data."""
    qkv, do = _data(case.table, case.S, case.B, case.probe)
    qkv_dev = qkv
    q = qkv[:, :, 0].double()
    if case.pre:
        qkv_dev = qkv.clone()
        qkv_dev[:, :, 0] = (qkv[:, :, 0].float() * SOFTMAX_Q_SCALE).to(torch.bfloat16)  # one rounding of the scaled q
        q = qkv_dev[:, :, 0].double() / SOFTMAX_Q_SCALE
    return dict(qkv_dev=qkv_dev, q=heads(q), k=heads(qkv[:, :, 1].double()), v=heads(qkv[:, :, 2].double()), do=do)


def bernoulli_keep(case, p, seed=5):
    """A host-side keep mask [B, NH, S, S] (bool) for the dropout forms of reference / emulate (the GPU test takes the kernels' own)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(case.B, NH, case.S, case.S, generator=g) >= p


# ================================================================================================ float64 reference and bounds
def softmax64(case, x, rows=None):
    vis = visible(case, rows=rows)
    s = (x["q"] @ x["k"].transpose(-1, -2)) * SCALE
    dead = ~vis.any(-1)  # [B, 1, S]
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(s.masked_fill(dead[..., None], 0.0), dim=-1).masked_fill(dead[..., None], 0.0)
    return vis, dead, s, p


def _floors(case, x, vis, p, pz, dS, out, zmax):
    """e32 [B, NH, S, 1], the dS floor [B, NH, S, S] (module docstring)."""
    A = SCALE * (x["q"].abs() @ x["k"].abs().transpose(-1, -2))
    amax = A.masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    nvis = vis.sum(-1, keepdim=True).double()
    e32 = U * (136.0 * amax + nvis + 40.0)
    do = heads(x["do"].double())
    edp = 70.0 * U * (zmax * (do.abs() @ x["v"].abs().transpose(-1, -2)) + (do * out).abs().sum(-1, keepdim=True))
    return e32, p * edp + 3.0 * e32 * dS.abs()


def _backward_bounds(x, p, dS, ds_floor, derr):
    """-> bound_dq, bound_dk and the UNIT of the fused backward's extra dq term, u scale |dS||K|: the term is G units (module docstring)."""
    t = 2.0 * U16 * dS.abs() + p * derr + ds_floor
    bq = SCALE * (t @ x["k"].abs()) * SECOND + FTZ
    bk = SCALE * (t.transpose(-1, -2) @ x["q"].abs()) * SECOND + FTZ
    unit = U16 * SCALE * (dS.abs() @ x["k"].abs()) * SECOND
    return bq, bk, unit


def bound_fused_dq(ref, G=2):
    """The dq bound of cm3p_attn_bwd_fused at G key blocks per slab (ref: what reference / conditioned return)."""
    assert G in (2, 4)
    return ref["bound"]["dq"] + float(G) * ref["fused_unit"]


def _rows_of(x, rows):
    """inputs(case) with q and dO cut to the query rows `rows` (k and v stay whole)."""
    return dict(x, q=x["q"][:, :, rows], do=x["do"][:, rows])


def reference(case, keep=None, p_drop=0.0, x=None, rows=None):
    """float64 autograd of softmax(scale q k^T + mask) v [with P o Z, Z = keep / (1 - p_drop)] and the componentwise bounds of the
    module docstring.  Dead rows: exact zeros, lse = -inf (the kernels store +inf).  x: inputs(case) with another dO (the packed
    entry points have no padded query rows: their dO is zero).
    rows (LongTensor): the same for these query rows only - out, lse, dq, dead, nvis and their bounds are [.., len(rows), ..] and equal
    the rows of the full reference; dk and dv (sums over ALL query rows) are not returned.  Nothing larger than [B, NH, len(rows), S]
    is built (no dropout form)."""
    x = x or inputs(case)
    if rows is not None:
        assert keep is None
        x = _rows_of(x, rows)
    q, k, v = (x[n].clone().requires_grad_(True) for n in "qkv")
    xx = dict(x, q=q, k=k, v=v)
    vis, dead, s, p = softmax64(case, xx, rows)
    zmax = 1.0 / (1.0 - p_drop)
    z = keep.double() * zmax if keep is not None else None
    pz = p * z if z is not None else p
    o = pz @ v
    do = heads(x["do"].double())
    o.backward(do)
    with torch.no_grad():
        lse = torch.logsumexp(s, dim=-1).masked_fill(dead, float("-inf")).expand(-1, NH, -1).clone()
        p, pz, out = p.detach(), pz.detach(), o.detach()
        dP = do @ x["v"].transpose(-1, -2)
        delta = (do * out).sum(-1, keepdim=True)
        dS = p * ((dP * z if z is not None else dP) - delta)
        e32, ds_floor = _floors(case, x, vis, p, pz, dS, out, zmax)
        pv = pz @ x["v"].abs()
        b_out = (2.0 * U16 + 3.0 * e32) * pv * SECOND + FTZ
        b_dv = (2.0 * U16 * (pz.transpose(-1, -2) @ do.abs()) + 3.0 * ((e32 * pz).transpose(-1, -2) @ do.abs())) * SECOND + FTZ
        derr = (do.abs() * b_out).sum(-1, keepdim=True)
        b_dq, b_dk, unit = _backward_bounds(x, p, dS, ds_floor, derr)
    res = dict(out=out, lse=lse, dq=q.grad, dk=k.grad, dv=v.grad, dead=dead.expand(-1, NH, -1).clone(), nvis=vis.sum(-1).expand(-1, NH, -1).clone(),
               bound=dict(out=b_out, dq=b_dq, dk=b_dk, dv=b_dv), bound_fused_dq=b_dq + 2.0 * unit, fused_unit=unit, e32=e32,
               l2_rows=rel_l2_rows(vis) if keep is not None else None)
    if rows is not None:
        for nm in ("dk", "dv"):
            del res[nm], res["bound"][nm]
    return res


def conditioned(case, out_got, keep=None, p_drop=0.0, x=None, rows=None):
    """dq and dk of the float64 backward that takes delta from the out the kernels STORED (what band_dq_block and the fused prep
    kernel do), and their bounds without the delta term: what is left is (1) and (2) of the module docstring and the floors.  A
    backward whose dq and dk do not use one and the same delta - the published one - fails this where the rounding of out matters
    most: rows whose softmax is nearly one-hot (dS small next to the rounding of delta).  rows: as in reference (out_got: those rows; dq only)."""
    x = x or inputs(case)
    if rows is not None:
        assert keep is None
        x = _rows_of(x, rows)
    with torch.no_grad():
        vis, dead, s, p = softmax64(case, x, rows)
        zmax = 1.0 / (1.0 - p_drop)
        z = keep.double() * zmax if keep is not None else None
        do = heads(x["do"].double())
        out = out_got.double()
        dP = do @ x["v"].transpose(-1, -2)
        dS = p * ((dP * z if z is not None else dP) - (do * out).sum(-1, keepdim=True))
        _, ds_floor = _floors(case, x, vis, p, p, dS, out, zmax)
        b_dq, b_dk, unit = _backward_bounds(x, p, dS, ds_floor, 0.0)
        res = dict(dq=SCALE * (dS @ x["k"]), dk=SCALE * (dS.transpose(-1, -2) @ x["q"]), bound=dict(dq=b_dq, dk=b_dk), bound_fused_dq=b_dq + 2.0 * unit,
                   fused_unit=unit)
        if rows is not None:
            del res["dk"], res["bound"]["dk"]
        return res


# ================================================================================================ the checks both test files run
def ratio(got, want, bound):
    """-> (worst error / bound, the number of elements outside their bound; NaN fails)."""
    err = (got.double() - want).abs()
    r = err / bound
    bad = ~(err <= bound)  # (NaN fails)
    return (float("inf") if bool(torch.isnan(r).any()) else r.max().item()), int(bad.sum())


_ratio = ratio


def rel_l2_rows(vis):
    """The rows the tensor-wide bound GRAD_REL_L2 is taken over in a dropout call -> dict(dq=, dk= bool [B, NH, S]).  A live row with ONE
    visible key has P = 1, out = Z v and dS = Z dP - delta = 0 in exact arithmetic: its dq, and the dk of a key that only such rows
    see, are identically zero in the reference.  The kernels take delta from the stored out = bf16(Z v), so unless Z v is a bf16 number
    (Z = 1 without dropout, Z = 2 at p = 0.5) their dS there is the rounding of out times |dO|.  The componentwise bounds count exactly
    that (the P derr term of the module docstring) and are asserted on those elements like on all others; a norm over the whole tensor
    would add their error to a reference that has nothing there (a sequence of one valid key - table A's third, table C's sequence 2 -
    puts S such rows on one key: 1.1e-2 on A-S300-w300 at p = 0.1 in the CPU emulation, 2.4e-3 at p = 0 and 0.5).  So the norm is
    taken over the complement: the dq rows that see more than one key and the dk rows of keys that such a row sees (or that no row
    sees), on every case."""
    one_key = vis.sum(-1, keepdim=True) == 1                 # [B, 1, S, 1]
    only_one_key_rows = vis.any(-2) & ~(vis & ~one_key).any(-2)  # [B, 1, S]: keys seen, but by one-key rows alone
    return dict(dq=(~one_key[..., 0]).expand(-1, NH, -1), dk=(~only_one_key_rows).expand(-1, NH, -1))


def check_float64(ref, got, fused=False, quantities=("out", "lse", "dq", "dk", "dv"), G=2):
    """-> (measured: {quantity: worst error / bound, d*_rel_l2, lse_max_abs}, failures: [str]).  got: out, dq, dk, dv [B, NH, S, 64] and
    lse [B, NH, S] (any of `quantities`).  The relative L2 error of a gradient is taken over the whole tensor, or, against a dropout
    reference, over rel_l2_rows.  fused: dq within bound_fused_dq(ref, G)."""
    seen, fails = {}, []
    for nm in quantities:
        if nm == "lse":
            live = ~ref["dead"]
            a, b = got["lse"].double()[live], ref["lse"][live]
            err = (a - b).abs()
            seen["lse_max_abs"] = err.max().item() if err.numel() else 0.0
            if not bool((err <= LSE_ATOL + LSE_RTOL * b.abs()).all()):
                fails.append(f"lse: max abs error {seen['lse_max_abs']:.3e} on live rows")
            continue
        bound = bound_fused_dq(ref, G) if (fused and nm == "dq") else ref["bound"][nm]
        seen[nm], nbad = _ratio(got[nm], ref[nm], bound)
        if nbad:
            fails.append(f"{nm}: {nbad} elements outside the bound, worst error / bound = {seen[nm]:.3f}")
        if nm != "out":
            rows = (ref.get("l2_rows") or {}).get(nm)
            g, w = (got[nm], ref[nm]) if rows is None else (got[nm][rows], ref[nm][rows])
            n = w.norm().item()
            if n > 0.0:
                seen[f"{nm}_rel_l2"] = ((g.double() - w).norm() / n).item()
                if not seen[f"{nm}_rel_l2"] < GRAD_REL_L2:
                    fails.append(f"{nm}: relative L2 error {seen[f'{nm}_rel_l2']:.3e}")
    return seen, fails


def check_conditioned(cond, got, fused=False, G=2):
    seen, fails = {}, []
    for nm in ("dq", "dk"):
        if nm not in cond:  # (a row-subset reference has no dk)
            continue
        bound = bound_fused_dq(cond, G) if (fused and nm == "dq") else cond["bound"][nm]
        seen[f"{nm}_given_out"], nbad = _ratio(got[nm], cond[nm], bound)
        if nbad:
            fails.append(f"{nm} given the stored out: {nbad} elements outside the bound, worst error / bound = {seen[f'{nm}_given_out']:.3f}")
    return seen, fails


def check_exact(case, ref, got):
    """Dead rows are exact zeros with lse = +inf, live rows have a finite lse, masked keys get dk = dv = 0 exactly, nothing is NaN."""
    fails = []
    dead = ref["dead"]
    for nm in ("out", "dq", "dk", "dv", "lse"):
        if nm in got and bool(torch.isnan(got[nm].float()).any()):
            fails.append(f"{nm} has NaN")
    if dead.any():
        if not bool((got["lse"][dead] == float("inf")).all()):
            fails.append("lse of a dead row is not +inf")
        if got["out"].float()[dead].abs().max().item() != 0.0:
            fails.append("out of a dead row is not exactly zero")
        if "dq" in got and got["dq"].float()[dead].abs().max().item() != 0.0:
            fails.append("dq of a dead row is not exactly zero")
    if not bool(torch.isfinite(got["lse"][~dead]).all()):
        fails.append("lse of a live row is not finite")
    km = key_mask(case)
    if km is not None and "dk" in got and not bool(km.all()):
        off = (~km)[:, None, :].expand(-1, NH, -1)
        if got["dk"].float()[off].abs().max().item() != 0.0 or got["dv"].float()[off].abs().max().item() != 0.0:
            fails.append("dk / dv of a masked key is not exactly zero")
    return fails


def check_probe(case, ref, got):
    """q = k = 0: every score is 0, lse = ln n_vis(q) - an exact per-row count of the mask rule -, p~ = exp2(0) = 1 and l = n are exact, so
    out = (sum of +-1) / n carries 1 / l, one fp32 product (4 U |out|: the floor) and the bf16 store (windows <= 64: n <= 129, where one
    key more or less still moves out by more than that); dq = dk = 0 exactly (every product has a zero factor)."""
    seen, fails = {}, []
    live = ~ref["dead"]
    want = torch.log(ref["nvis"].double()[live])
    err = (got["lse"].double()[live] - want).abs()
    seen["lse_count_max_abs"] = err.max().item() if err.numel() else 0.0
    if not bool((err <= PROBE_LSE_TOL).all()):
        fails.append(f"lse - ln n_vis: max {seen['lse_count_max_abs']:.3e}")
    if 0 <= case.window <= PROBE_OUT_MAX_WINDOW:
        seen["out"], nbad = _ratio(got["out"], ref["out"], probe_out_bound(ref))
        if nbad:
            fails.append(f"out: {nbad} elements outside u |out|, worst {seen['out']:.3f}")
    for nm in ("dq", "dk"):
        if nm in got and got[nm].float().abs().max().item() != 0.0:
            fails.append(f"{nm} is not exactly zero")
    return seen, fails


def probe_out_bound(ref):
    """(+ 1e-15: the float64 reference's own error - 1 / n is not a float64 number, a sum of +-1 / n that cancels comes out as ~1e-17)"""
    return (U16 * SECOND + 4.0 * U) * ref["out"].abs() + 1e-15


# ================================================================================================ CPU emulation
def _bf(x):
    return x.to(torch.bfloat16).float()


def wrong_visibility(case, wrong):
    """The visibility a wrong evaluation applies ([B, 1, S, Sk]; Sk > S only for "ragged_keys")."""
    S, w = case.S, case.window
    km = key_mask(case)
    vis = visible(case)
    i = torch.arange(S)
    d = i[None, :] - i[:, None]  # kv - q
    kmv = km[:, None, None, :] if km is not None else torch.ones(case.B, 1, 1, S, dtype=torch.bool)
    if wrong == "widen_right" and w >= 0:
        vis = kmv & ((d >= -w) & (d <= w + 1))[None, None]
    elif wrong == "narrow_left" and w >= 0:
        vis = kmv & ((d >= -w + 1) & (d <= w))[None, None]
    elif wrong == "drop_half_tile" and w >= 0:
        vis = vis.clone()
        for q0 in range(0, S, 32):
            for key0 in range(0, S, 64):
                touches = key0 <= q0 + 31 + w and key0 + 63 >= q0 - w
                inside = key0 >= q0 + 31 - w and key0 + 63 <= q0 + w
                if touches and not inside:
                    vis[:, :, q0:q0 + 32, key0:key0 + 32] = False
    elif wrong == "mask_ignored_last_tile":
        t0 = 64 * ((S - 1) // 64)
        kmv = kmv.clone()
        kmv[..., t0:] = True
        vis = kmv & ((d.abs() <= w) if w >= 0 else torch.ones(S, S, dtype=torch.bool))[None, None]
    elif wrong == "ragged_keys":
        Sk = 64 * ((S + 63) // 64)
        j = torch.arange(Sk)
        band = ((j[None, :] - i[:, None]).abs() <= w) if w >= 0 else torch.ones(S, Sk, dtype=torch.bool)
        kme = torch.ones(case.B, 1, 1, Sk, dtype=torch.bool)
        kme[..., :S] = kmv
        vis = kme & band[None, None]
    return vis


WRONG = ("widen_right", "narrow_left", "drop_half_tile", "mask_ignored_last_tile", "ragged_keys", "dead_mean", "delta_split")
# mistakes of the dropout forms (they need a keep mask).  keep_group_shifted: on the last 64-key tile the decisions of an 8-key group are
# those of the neighbouring group (the next one; the previous one where the next would leave the sequence) - in the forward, the dQ
# sweep and the dK/dV sweep, which each regenerate the mask with index arithmetic of their own, or in one of the three alone.
WRONG_DROP = ("l_dropped", "keep_transposed", "keep_group_shifted", "keep_group_shifted_fwd", "keep_group_shifted_dq", "keep_group_shifted_dkv",
              "ds_no_z", "dv_no_z", "delta_from_undropped_out", "scale_missing_fwd")


def last_tile_start(S):
    return 64 * ((S - 1) // 64)


def shift_keep_groups(keep):
    """keep [..., S, S] with the key groups of the last 64-key tile taken from their neighbours (WRONG_DROP's keep_group_shifted)."""
    S = keep.shape[-1]
    k = torch.arange(S)
    src = torch.where(k + 8 < S, k + 8, k - 8)
    src = torch.where(k >= last_tile_start(S), src, k)
    return keep[..., src]


def all_dropped_rows(case, keep):
    """bool [B, NH, S]: live query rows whose visible keys are all dropped - out is exact zeros there while lse is finite."""
    vis = visible(case)
    return vis.any(-1).expand(-1, NH, -1) & ~(vis & keep).any(-1)


WRONG_FUSED_SLABS = ("block_never_added", "last_partial_slab_dropped", "block_added_twice", "slab_of_the_other_head")


def fused_dq_sum(parts, G, wrong=None):
    """The fused backward's dQ from its per-256-key-block bf16 partials [B, NH, S, 64] (fp32 tensors holding bf16 values): the G partials
    of a group are added one after another in bf16, acc = bf16(acc + part), starting from the stored first one (the packed-bf16 atomic
    adds of positions 1 .. G - 1, stream-ordered); the slabs are summed in fp32 in slab order (dq_reduce_tile).
    wrong: block_never_added - positions 2 and 3 of every group are missing (the stage bits of G = 2 sent to a library running G = 4);
    last_partial_slab_dropped - the reduce counts full groups only; block_added_twice - position 1 of every group; slab_of_the_other_head
    - the reduce reads the LAST slab from the other head."""
    slabs = []
    for j in range(0, len(parts), G):
        grp = parts[j:j + G]
        if wrong == "block_never_added":
            grp = grp[:2]
        acc = grp[0]
        for part in grp[1:]:
            acc = _bf(acc + part)
        if wrong == "block_added_twice" and len(grp) > 1:
            acc = _bf(acc + grp[1])
        slabs.append(acc)
    if wrong == "last_partial_slab_dropped" and len(parts) % G:
        slabs[-1] = torch.zeros_like(slabs[-1])
    if wrong == "slab_of_the_other_head":
        slabs[-1] = slabs[-1].flip(1)
    return functools.reduce(lambda a, b: a + b, slabs)


def emulate(case, keep=None, p_drop=0.0, wrong=None, fused=False, G=2, x=None):
    """A torch fp32 restatement of the kernels' documented arithmetic: fp32 scores of the device's q (exp2 units), p~ = exp2(s - m),
    l = sum p~, bf16(p~ o keep) V / l [/ (1 - p)] stored as bf16; backward p = exp2(s - lse log2 e), delta from the STORED out,
    dS = p (Z dP - delta) and p o Z rounded to bf16, bf16 stores; fused: one bf16 partial dq per 256-key block, the G of a slab added in bf16.
    wrong: one of WRONG or (with a keep mask) WRONG_DROP - the same arithmetic with one mistake; fused: or one of WRONG_FUSED_SLABS, at G
    key blocks per slab (fused_dq_sum).  x: inputs(case) with another dO.  Also returned: dq_acc and dk_acc, the fp32 sums the epilogues
    rotate, scale (dk_mul for dk) and round (tests/attention_fused_refs.py)."""
    x = x or inputs(case)
    S = case.S
    qkv = x["qkv_dev"].float()
    qd, k, v = (heads(qkv[:, :, j]) for j in range(3))
    do = heads(x["do"].float())
    vis = wrong_visibility(case, wrong) if wrong in WRONG[:5] else visible(case)
    Sk = vis.shape[-1]
    if Sk > S:  # keys >= S of the ragged tile: the clamped row's data
        k = torch.cat([k, k[:, :, S - 1:S].expand(-1, -1, Sk - S, -1)], 2)
        v = torch.cat([v, v[:, :, S - 1:S].expand(-1, -1, Sk - S, -1)], 2)
    zs = 1.0 / (1.0 - p_drop)
    # the three sweeps' masks: forward, dQ, dK/dV
    keepf = keepq = keepk = keep.float() if keep is not None else None
    if keep is not None:
        if Sk > S:
            keepf = keepq = keepk = torch.cat([keepf, torch.ones(case.B, NH, S, Sk - S)], 3)
        if wrong == "keep_transposed":
            keepf = keepq = keepk = keep.float().transpose(-1, -2)
        if wrong in ("keep_group_shifted", "keep_group_shifted_fwd"):
            keepf = shift_keep_groups(keep.float())
        if wrong in ("keep_group_shifted", "keep_group_shifted_dq"):
            keepq = shift_keep_groups(keep.float())
        if wrong in ("keep_group_shifted", "keep_group_shifted_dkv"):
            keepk = shift_keep_groups(keep.float())
    s2 = qd @ k.transpose(-1, -2)
    if not case.pre:
        s2 = s2 * SOFTMAX_Q_SCALE
    s2 = s2.masked_fill(~vis, float("-inf"))
    dead = ~vis.any(-1).expand(-1, NH, -1)
    m = s2.amax(-1, keepdim=True).masked_fill(dead[..., None], 0.0)
    pt = torch.exp2(s2 - m)
    ptz = pt * keepf if keepf is not None else pt
    l = (ptz if wrong == "l_dropped" else pt).sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o32 = (_bf(ptz) @ v) * (inv * zs if (keepf is not None and wrong != "scale_missing_fwd") else inv)
    out = o32.to(torch.bfloat16)
    lse = ((m + torch.log2(l)) * LN2)[..., 0].masked_fill(dead, float("inf"))
    if wrong == "dead_mean":
        out = torch.where(dead[..., None], v.mean(2, keepdim=True).to(torch.bfloat16).expand_as(out), out)

    lse2 = (lse * LOG2E)[..., None]
    p = torch.exp2(s2 - lse2).masked_fill(~vis, 0.0).masked_fill(dead[..., None], 0.0)
    delta = (do * out.float()).sum(-1, keepdim=True)
    if wrong == "delta_from_undropped_out":
        delta = (do * ((_bf(pt) @ v) * inv).to(torch.bfloat16).float()).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)

    def z_dp(kx):
        return dP * kx * zs if (kx is not None and wrong != "ds_no_z") else dP

    dS = p * (z_dp(keepk) - delta)
    dS_q = p * (z_dp(keepq) - ((do * o32).sum(-1, keepdim=True) if wrong == "delta_split" else delta))
    ds16, dsq16 = _bf(dS), _bf(dS_q)
    if fused:
        parts = [_bf(dsq16[..., j:j + 256] @ k[:, :, j:j + 256]) for j in range(0, Sk, 256)]
        dq_acc = fused_dq_sum(parts, G, wrong)
    else:
        dq_acc = dsq16 @ k
    dq = (dq_acc * SCALE).to(torch.bfloat16)
    dk_acc, dk_mul = (ds16.transpose(-1, -2) @ qd)[:, :, :S], (LN2 if case.pre else SCALE)
    dk = (dk_acc * dk_mul).to(torch.bfloat16)
    pz16 = _bf(p * keepk * zs) if (keepk is not None and wrong != "dv_no_z") else _bf(p)
    dv = (pz16.transpose(-1, -2) @ do).to(torch.bfloat16)[:, :, :S]
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, delta=delta[..., 0], dq_acc=dq_acc, dk_acc=dk_acc, dk_mul=dk_mul)


# ================================================================================================ index arithmetic
def tile_unmasked(all_valid, key0, q0, window):
    return bool(all_valid) and (window < 0 or (key0 >= q0 + 31 - window and key0 + 63 <= q0 + window))


def _sweep_label(n):
    return f"sweep_{n}_tiles" if n <= 4 else "sweep_more_than_4_tiles"


def coverage(case):
    """Which branches of the band kernels' index arithmetic a case reaches: {"fwd" | "dq" | "dkv": set of labels}.  A restatement of
    attn_fwd_kernel (QSUB = 1), band_dq_block and band_dkv_block: 128-row workgroup blocks, 32-row wave blocks, 64-row tiles swept from
    t_lo to t_hi, the wave's own band wlo .. whi, the 32-row half tiles of the two backward kernels, tile_unmasked / plain."""
    S, w = case.S, case.window
    km = key_mask(case)
    cov = {"fwd": set(), "dq": set(), "dkv": set()}
    for b in range(case.B):
        valid = [bool(km[b, j]) if km is not None else True for j in range(S)]
        for X0 in range(0, S, 128):  # the workgroup's queries (fwd, dq) or keys (dkv)
            X1 = min(S, X0 + 128) - 1
            lo_t, hi_t = (0, (S - 1) // 64) if w < 0 else (max(0, X0 - w) // 64, min(S - 1, X1 + w) // 64)
            for g in cov:
                cov[g].add(_sweep_label(hi_t - lo_t + 1))
            for wid in range(4):
                x0 = X0 + 32 * wid
                if x0 >= S:
                    for g in cov:
                        cov[g].add("dead_wave_in_live_workgroup")
                    continue
                wlo, whi = (0, S - 1) if w < 0 else (max(0, x0 - w), min(S - 1, x0 + 31 + w))
                keys_all_ok = all(x0 + j < S and valid[x0 + j] for j in range(32))  # dkv: this wave's 32 keys
                for t in range(lo_t, hi_t + 1):
                    r0 = 64 * t
                    ragged = r0 + 63 >= S
                    if not (r0 <= whi and r0 + 63 >= wlo):
                        for g in cov:
                            cov[g].add("tile_visited_by_workgroup_skipped_by_wave")
                        continue
                    all_valid = (not ragged) and all(valid[r0:r0 + 64])
                    inside = w < 0 or (r0 >= x0 + 31 - w and r0 + 63 <= x0 + w)
                    for g in ("fwd", "dq"):
                        if ragged:
                            cov[g].add("ragged_last_tile")
                        if tile_unmasked(all_valid, r0, x0, w):
                            cov[g].add("tile_unmasked")
                        if not inside:
                            cov[g].add("tile_masked_for_the_window")
                        if not all_valid:
                            cov[g].add("tile_masked_for_an_invalid_key")
                    if ragged:
                        cov["dkv"].add("ragged_last_tile")
                    for blk in range(2):
                        h0 = r0 + 32 * blk
                        if h0 > whi or h0 + 31 < wlo:
                            cov["dq"].add("half_tile_skipped")
                            cov["dkv"].add("half_tile_skipped")
                            continue
                        plain = keys_all_ok and (w < 0 or (h0 >= x0 + 31 - w and h0 + 31 <= x0 + w))
                        cov["dkv"].add("plain" if plain else ("not_plain_for_the_window" if keys_all_ok else "not_plain_for_an_invalid_key"))
    return cov


COVERAGE_REQUIRED = {
    "fwd": {"tile_unmasked", "tile_masked_for_the_window", "tile_masked_for_an_invalid_key", "tile_visited_by_workgroup_skipped_by_wave",
            "dead_wave_in_live_workgroup", "ragged_last_tile"},
    "dq": {"tile_unmasked", "tile_masked_for_the_window", "tile_masked_for_an_invalid_key", "tile_visited_by_workgroup_skipped_by_wave",
           "half_tile_skipped", "dead_wave_in_live_workgroup", "ragged_last_tile"},
    "dkv": {"plain", "not_plain_for_the_window", "not_plain_for_an_invalid_key", "tile_visited_by_workgroup_skipped_by_wave", "half_tile_skipped",
            "dead_wave_in_live_workgroup", "ragged_last_tile"},
}
SWEEPS = {_sweep_label(n) for n in (1, 2, 3, 4, 5)}


def probs_bound(ref, p64):
    """cm3p_attn_probs: p = exp2(acc - lse log2 e), acc a 64-term fp32 fma chain over fp32(q q_mul) k, lse the forward's.  Both exponents
    carry the relative error the module docstring counts as e32 (the dot product and the stored lse), so |p - p64| <= 3 e32 p64 (twice
    for the two, once for exp2 and the q q_mul product) - about 3e-4 p64 here, not the 1e-2 the model-level test allows."""
    return 3.0 * ref["e32"] * p64 * SECOND + FTZ
