"""Float64 reference, derived per-element bounds, case table, CPU emulation and index-arithmetic restatement of the small-head attention
kernels (csrc/attention_generic.hip: attn_gen_fwd_kernel, attn_gen_dq_kernel, attn_gen_dkv_kernel at D = 16, 32, 64 and their dropout
pack), shared by tests/test_attn_generic_gpu.py (the kernels against them) and tests/test_attn_generic_refs_host.py (the emulation must
pass every check, wrong evaluations must fail a named one, the table must reach every branch of the index arithmetic).  No GPU and no
cm3p_amd import here.  The masks, windows, lengths and the Case record are tests/attention_refs.py's: the seams are the ones head 64 is
held to.  scale = D ** -0.5, plain q only (the generic entries have no pre-scaled mode).

Tensors are [B, NH, S, D] (lse: [B, NH, S]) on this side; the GPU test converts from the packed layouts.

The bounds, counted from attention_generic.hip.  u = 2^-8 (bf16), U = 2^-24 (fp32), SECOND = 1 + 1e-3.  One thread owns one query (or
key) row and everything is fp32 until ONE bf16 rounding at each store (store_row_bf16): P is never rounded to bf16, unlike the head-64
path, so every leading term is 1 u where tests/attention_refs.py has 2 u.  With P the softmax, Z = keep / (1 - p) (1 without dropout),
dP = dO V^T, delta = rowsum(dO o out), dS = P o (Z o dP - delta):

  out  u (P o Z)|V|                   the store; |out| <= (P o Z)|V|.
  dv   u (P o Z)^T|dO|                the store.
  dq   scale (u |dS| + P derr)|K|     the store (|dq| <= scale |dS||K|), and delta is taken from the ROUNDED out (attn_gen_dq_kernel's `dlt`
                                      reads o_rows): it is off by derr[q] = sum_d |dO[q, d]| bound_out[q, d] (= u |dO|.|out| up to
                                      the floor), which enters dS as P derr.
  dk   scale (u |dS| + P derr)^T|Q|   attn_gen_dkv_kernel reads the delta the dq kernel published.

fp32 floors, per query row, in natural-log units.  A[q, k] = scale |q|.|k|, Amax[q] its maximum over the row's visible keys, n = n_vis[q],
L = |lse[q]|.
  score    D fmas (D U A), times c = scale log2 e, itself two roundings (3 U A)                                 (D + 3) U Amax
  eta      what one term of l or of the o accumulation carries on top of its score: s - m (U (|s| + |m|) <= 2 U Amax), v_exp_f32
           (2 U), the per-key online rescale - up to n factors a = exp2(m - s), each 2 U for the exp2 and U for the product, their
           exponent roundings telescoping to 2 U Amax -, and the n-term accumulation (n U):               eta = U (4 Amax + 4 n + 2)
  e_f      relative error of l and of every p~-weighted forward sum:                                    e_f = (D + 3) U Amax + eta
           out = o / l [* 1 / (1 - p)]: numerator and denominator (2 e_f), 1 / l, the dropout scale and its product, the final
           product (4 U)
  e_lse    ABSOLUTE error of the stored lse = (m + v_log_f32(l)) ln 2: e_f, the logarithm (2 U ln n + 2 U), the sum and the
           product with the rounded ln 2 (3 U L):                                       e_lse = e_f + U (3 L + 2 ln n + 2)
  e_pb     relative error of the backward's p = exp2(s c - lse log2 e): the stored lse (e_lse), the score again ((D + 3) U Amax), the
           lse -> lse log2 e reload (2 U L), the subtraction (U (Amax + L)), v_exp_f32 (2 U):   e_pb = e_lse + U ((D + 4) Amax + 3 L + 2)
  edp      Z dP - delta: two D-term fma chains, the dropout fma's rounded scale and the subtraction:
                                                          edp[q, k] = (D + 4) U (zmax |dO[q]|.|V[k]| + sum_d |dO o out|)
  dS floor P edp + (e_pb + (S + 2) U)|dS|: the product with p, the accumulation over at most S keys (queries), the product with scale.
  dv floor (e_pb + (S + 4) U)(P o Z): p, the dropout scale and its product, the accumulation over at most S queries.
With unit-variance data e_f ~ 1e-4: a few per cent of u.  None of these constants is fitted to a measurement.
"""
import functools
import math
from dataclasses import dataclass

import torch

import attention_refs as AR
from attention_refs import CASES_B, CASES_G, LENS_A, PROBE_LSE_TOL, U16, WINDOWS_A, WINDOWS_C, Case, heads, key_mask, visible
from row_kernel_refs import FTZ, SECOND, U

NH = 2
HEAD_DIMS = (16, 32)
LOG2E = 1.4426950408889634
LN2 = 0.69314718055994531
DROPOUT_PS = (0.1, 0.5)
DROPOUT_WINDOWS_A = (0, 1, 63, 64, 65, 300)


@dataclass(frozen=True)
class GCase:
    D: int
    case: Case  # tests/attention_refs.py's record, always with plain q

    @property
    def name(self):
        return f"d{self.D}-{self.case.name}"

    @property
    def scale(self):
        return self.D ** -0.5

    @property
    def B(self):
        return self.case.B

    @property
    def S(self):
        return self.case.S


def _plain(cases):
    return [c for c in cases if not c.pre]


_A, _B, _C, _G = _plain(AR.TABLE_A), _plain(AR.TABLE_B), _plain(AR.TABLE_C), _plain(AR.TABLE_G)
TABLE_A = [GCase(D, c) for D in HEAD_DIMS for c in _A]
TABLE_B = [GCase(D, c) for D in HEAD_DIMS for c in _B]
TABLE_C = [GCase(D, c) for D in HEAD_DIMS for c in _C]
TABLE_G = [GCase(D, c) for D in HEAD_DIMS for c in _G]
# head 64 (the cross-check instance): one case of each table
TABLE_64 = [GCase(64, AR.BY_NAME[n]) for n in ("A-S300-w33-pad-plain", "B-S257-w127-nomask-plain", "C-S300-w64-holes-plain", "G-S257-w-1-pad-plain")]
# the count probe at every window of table A
TABLE_P = [GCase(D, Case("A", 300, w, LENS_A, False, True)) for D in HEAD_DIMS for w in WINDOWS_A]
TABLE = TABLE_A + TABLE_B + TABLE_C + TABLE_G + TABLE_64
TABLE_DROP = [g for g in TABLE_A if g.case.window in DROPOUT_WINDOWS_A] + TABLE_C + TABLE_G
BY_NAME = {g.name: g for g in TABLE + TABLE_P}


# ================================================================================================ data
@functools.lru_cache(maxsize=None)
def _data(D, table, S, B, probe):
    if D == 64:  # the draw of tests/attention_refs.py: the MFMA kernels' own bounds hold on the same tensors
        return AR._data(table, S, B, probe)
    g = torch.Generator().manual_seed(16000 + 131 * D + 977 * ord(table) + S)
    qkv = torch.randn(B, S, 3, NH, D, generator=g).to(torch.bfloat16)
    do = torch.randn(B, S, NH, D, generator=g).to(torch.bfloat16)
    if probe:
        qkv[:, :, :2] = 0
        bit = (torch.arange(S)[:, None] >> (torch.arange(D)[None, :] % 10)) & 1
        qkv[:, :, 2] = (1.0 - 2.0 * bit.float())[None, :, None, :].to(torch.bfloat16)  # +-1: exact in bf16
    return qkv, do


def inputs(g):
    """-> dict(qkv bf16 [B, S, 3, NH, D], do bf16 [B, S, NH, D]: what the device gets; q, k, v float64 [B, NH, S, D]).  One draw per
    (D, table, S): the windows of a table share their data."""
    qkv, do = _data(g.D, g.case.table, g.S, g.B, g.case.probe)
    return dict(qkv=qkv, do=do, q=heads(qkv[:, :, 0].double()), k=heads(qkv[:, :, 1].double()), v=heads(qkv[:, :, 2].double()))


def bernoulli_keep(g, p, seed=5):
    """A host-side keep mask [B, NH, S, S] (query, key) for the dropout forms (the GPU test takes the Philox restatement)."""
    return AR.bernoulli_keep(g.case, p, seed)


# ================================================================================================ float64 reference and bounds
def reference(g, keep=None, p_drop=0.0):
    """float64 out, lse, dq, dk, dv of softmax(scale q k^T + mask) v [with P o Z, Z = keep / (1 - p_drop)] in closed form (the host test
    compares them with float64 autograd) and the componentwise bounds of the module docstring.  Dead rows: zeros, lse = +inf."""
    case, D, S, scale = g.case, g.D, g.S, g.scale
    x = inputs(g)
    q, k, v = x["q"], x["k"], x["v"]
    do = heads(x["do"].double())
    vis = visible(case)
    dead = ~vis.any(-1)  # [B, 1, S]
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~vis, float("-inf"))
    p = torch.softmax(s.masked_fill(dead[..., None], 0.0), dim=-1).masked_fill(dead[..., None], 0.0)
    lse = torch.logsumexp(s, dim=-1).masked_fill(dead, float("inf"))
    zmax = 1.0 / (1.0 - p_drop) if p_drop < 1.0 else 0.0
    z = keep.double() * zmax if keep is not None else None
    pz = p * z if z is not None else p
    out = pz @ v
    dP = do @ v.transpose(-1, -2)
    delta = (do * out).sum(-1, keepdim=True)
    dS = p * ((dP * z if z is not None else dP) - delta)
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), pz.transpose(-1, -2) @ do

    A = scale * (q.abs() @ k.abs().transpose(-1, -2))
    amax = A.masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    nvis = vis.sum(-1, keepdim=True).double().expand(-1, NH, -1, -1)
    L = lse.masked_fill(dead, 0.0).abs()[..., None]
    logn = torch.log(nvis.clamp(min=1.0))
    eta = U * (4.0 * amax + 4.0 * nvis + 2.0)
    e_f = (D + 3.0) * U * amax + eta
    e_lse = e_f + U * (3.0 * L + 2.0 * logn + 2.0)
    e_pb = e_lse + U * ((D + 4.0) * amax + 3.0 * L + 2.0)
    edp = (D + 4.0) * U * (max(zmax, 1.0) * (do.abs() @ v.abs().transpose(-1, -2)) + (do * out).abs().sum(-1, keepdim=True))
    ds_floor = p * edp + (e_pb + (S + 2.0) * U) * dS.abs()

    b_out = (U16 + 2.0 * e_f + 4.0 * U) * (pz @ v.abs()) * SECOND + FTZ
    b_lse = (e_lse * SECOND)[..., 0]
    b_dv = ((U16 * pz + (e_pb + (S + 4.0) * U) * pz).transpose(-1, -2) @ do.abs()) * SECOND + FTZ
    derr = (do.abs() * b_out).sum(-1, keepdim=True)
    t = U16 * dS.abs() + p * derr + ds_floor
    b_dq = scale * (t @ k.abs()) * SECOND + FTZ
    b_dk = scale * (t.transpose(-1, -2) @ q.abs()) * SECOND + FTZ
    return dict(out=out, lse=lse.expand(-1, NH, -1).clone(), dq=dq, dk=dk, dv=dv, dead=dead.expand(-1, NH, -1).clone(),
                nvis=vis.sum(-1).expand(-1, NH, -1).clone(), bound=dict(out=b_out, lse=b_lse, dq=b_dq, dk=b_dk, dv=b_dv))


# ================================================================================================ the checks both test files run
def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    r = err / bound
    bad = ~(err <= bound)  # (NaN fails)
    return (float("inf") if bool(torch.isnan(r).any()) else (r.max().item() if r.numel() else 0.0)), int(bad.sum())


def check_float64(ref, got, quantities=("out", "lse", "dq", "dk", "dv")):
    """-> (measured {quantity: worst |got - R| / bound}, failures {check name: message}).  lse on the live rows."""
    seen, fails = {}, {}
    live = ~ref["dead"]
    for nm in quantities:
        if nm == "lse":
            seen[nm], nbad = _ratio(got["lse"][live], ref["lse"][live], ref["bound"]["lse"][live])
        else:
            seen[nm], nbad = _ratio(got[nm], ref[nm], ref["bound"][nm])
        if nbad:
            fails[nm] = f"{nbad} elements outside the bound, worst error / bound = {seen[nm]:.3f}"
    return seen, fails


def check_exact(g, ref, got):
    """Dead rows are exact zeros with lse = +inf, live rows have a finite lse, padded and masked keys get dk = dv = 0 exactly, nothing is
    NaN.  -> failures {check name: message}."""
    fails = {}
    dead = ref["dead"]
    if any(bool(torch.isnan(got[nm].float()).any()) for nm in ("out", "dq", "dk", "dv", "lse") if nm in got):
        fails["nan"] = "an output has NaN"
    if dead.any():
        bad = [nm for nm in ("out", "dq") if nm in got and got[nm].float()[dead].abs().max().item() != 0.0]
        if not bool((got["lse"][dead] == float("inf")).all()):
            bad.append("lse")
        if bad:
            fails["dead_rows"] = f"dead rows: {bad} not exactly zero / +inf"
    if not bool(torch.isfinite(got["lse"][~dead]).all()):
        fails["lse_finite"] = "lse of a live row is not finite"
    km = key_mask(g.case)
    if km is not None and "dk" in got and not bool(km.all()):
        off = (~km)[:, None, :].expand(-1, NH, -1)
        if got["dk"].float()[off].abs().max().item() != 0.0 or got["dv"].float()[off].abs().max().item() != 0.0:
            fails["padded_keys"] = "dk / dv of a masked key is not exactly zero"
    return fails


def probe_out_bound(ref):
    """q = k = 0: p~ = 1, l = n and the sum of +-1 are exact; out carries 1 / l, one product and the store (+ 1e-15: 1 / n is not a float64
    number)."""
    return (U16 * SECOND + 4.0 * U) * ref["out"].abs() + 1e-15


def check_probe(g, ref, got):
    """q = k = 0: lse = ln n_vis(q) - an exact per-row count of the mask rule: (0 + v_log_f32(n)) ln 2 is good to a few U ln n, far
    inside PROBE_LSE_TOL, which is below half of ln(301 / 300) -, out = (sum of +-1 over the visible keys) / n to one rounding, and
    dq = dk = 0 exactly (every product has a zero factor)."""
    seen, fails = {}, {}
    live = ~ref["dead"]
    err = (got["lse"].double()[live] - torch.log(ref["nvis"].double()[live])).abs()
    seen["count_lse"] = (err.max().item() if err.numel() else 0.0) / PROBE_LSE_TOL
    if not bool((err <= PROBE_LSE_TOL).all()):
        fails["count_lse"] = f"lse - ln n_vis: max {err.max().item():.3e}"
    seen["count_out"], nbad = _ratio(got["out"], ref["out"], probe_out_bound(ref))
    if nbad:
        fails["count_out"] = f"{nbad} elements outside u |out|, worst {seen['count_out']:.3f}"
    if any(nm in got and got[nm].float().abs().max().item() != 0.0 for nm in ("dq", "dk")):
        fails["probe_zero_grads"] = "dq / dk is not exactly zero"
    return seen, fails


def all_checks(g, ref, got):
    """Every check the GPU test applies to one forward + backward -> (measured, failures {check name: message})."""
    if g.case.probe:
        seen, fails = check_probe(g, ref, got)
        s2, f2 = check_float64(ref, got, quantities=("dv",))
        seen, fails = dict(seen, **s2), dict(fails, **f2)
    else:
        seen, fails = check_float64(ref, got)
    return seen, dict(fails, **check_exact(g, ref, got))


# ================================================================================================ CPU emulation
def _bf(x):
    return x.to(torch.bfloat16).float()


VISIBILITY_WRONG = ("low_edge_narrow", "low_edge_wide", "high_edge_narrow", "high_edge_wide", "tail_keys", "mask_ignored")
DROPOUT_WRONG = ("l_dropped", "keep_transposed", "ds_no_z", "dv_no_z")
WRONG = VISIBILITY_WRONG + ("dead_uniform", "dk_no_scale", "p_bf16") + DROPOUT_WRONG


def wrong_visibility(case, wrong):
    """The visibility a wrong evaluation applies ([B, 1, S, Sk]; Sk > S only for "tail_keys").  *_narrow: the source's `kk < q - window`
    / `kk > q + window` written with `<=` / `>=`; *_wide: the edge one key further out."""
    S, w = case.S, case.window
    km = key_mask(case)
    kmv = km[:, None, None, :] if km is not None else torch.ones(case.B, 1, 1, S, dtype=torch.bool)
    i = torch.arange(S)
    d = i[None, :] - i[:, None]  # kv - q
    if wrong in VISIBILITY_WRONG[:4]:
        if w < 0:
            return visible(case)
        lo = {"low_edge_narrow": -w + 1, "low_edge_wide": -w - 1}.get(wrong, -w)
        hi = {"high_edge_narrow": w - 1, "high_edge_wide": w + 1}.get(wrong, w)
        return kmv & ((d >= lo) & (d <= hi))[None, None]
    if wrong == "mask_ignored":
        return visible(case, km=None)
    if wrong == "tail_keys":  # the staged rows past the sequence (stage_kv_tile's min(key, S - 1)) taken for keys
        Sk = 64 * ((S + 63) // 64)
        j = torch.arange(Sk)
        band = ((j[None, :] - i[:, None]).abs() <= w) if w >= 0 else torch.ones(S, Sk, dtype=torch.bool)
        kme = torch.ones(case.B, 1, 1, Sk, dtype=torch.bool)
        kme[..., :S] = kmv
        return kme & band[None, None]
    return visible(case)


def emulate(g, keep=None, p_drop=0.0, wrong=None):
    """The kernels' roundings in torch fp32: fp32 scores times c = scale log2 e, p~ = exp2(s - m), l = sum p~ (undropped), out =
    bf16((p~ o keep) V / l [/ (1 - p)]) with P kept in fp32, lse = (m + log2 l) ln 2; backward p = exp2(s - lse log2 e), delta from the
    ROUNDED out, dS = p (Z dP - delta), one bf16 rounding of dq scale, dk scale and dv.  wrong: one of WRONG - the same arithmetic with
    one mistake."""
    case, S, scale = g.case, g.S, g.scale
    x = inputs(g)
    qkv = x["qkv"].float()
    q, k, v = (heads(qkv[:, :, j]) for j in range(3))
    do = heads(x["do"].float())
    vis = wrong_visibility(case, wrong) if wrong in VISIBILITY_WRONG else visible(case)
    Sk = vis.shape[-1]
    if Sk > S:
        k = torch.cat([k, k[:, :, S - 1:S].expand(-1, -1, Sk - S, -1)], 2)
        v = torch.cat([v, v[:, :, S - 1:S].expand(-1, -1, Sk - S, -1)], 2)
    zs = 1.0 / (1.0 - p_drop) if p_drop < 1.0 else 0.0
    keepf = keep.float() if keep is not None else None
    if keepf is not None and wrong == "keep_transposed":
        keepf = keepf.transpose(-1, -2).contiguous()
    if keepf is not None and Sk > S:
        keepf = torch.cat([keepf, torch.ones(case.B, NH, S, Sk - S)], 3)
    c = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    s2 = ((q @ k.transpose(-1, -2)) * c).masked_fill(~vis, float("-inf"))
    dead = ~vis.any(-1).expand(-1, NH, -1)
    m = s2.amax(-1, keepdim=True).masked_fill(dead[..., None], 0.0)
    pt = torch.exp2(s2 - m)
    ptz = pt * keepf if keepf is not None else pt
    l = (ptz if wrong == "l_dropped" else pt).sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    if wrong == "p_bf16":
        ptz = _bf(ptz)
    o32 = (ptz @ v) * (inv * zs if keepf is not None else inv)
    out = o32.to(torch.bfloat16)
    lse = torch.where(l > 0, (m + torch.log2(l)) * LN2, torch.full_like(l, float("inf")))[..., 0]
    if wrong == "dead_uniform":
        out = torch.where(dead[..., None], v[:, :, :S].mean(2, keepdim=True).to(torch.bfloat16).expand_as(out), out)
        lse = torch.where(dead, torch.full_like(lse, math.log(S)), lse)

    lse2 = (lse * LOG2E)[..., None]
    p = torch.exp2(s2 - lse2).masked_fill(~vis, 0.0)
    delta = (do * out.float()).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    if keepf is not None:
        zdp = dP * keepf * (1.0 if wrong == "ds_no_z" else zs)
        pz = p * keepf * (1.0 if wrong == "dv_no_z" else zs)
    else:
        zdp, pz = dP, p
    dS = p * (zdp - delta)
    dq = ((dS @ k) * scale).to(torch.bfloat16)
    dk = ((dS.transpose(-1, -2) @ q) * (1.0 if wrong == "dk_no_scale" else scale)).to(torch.bfloat16)[:, :, :S]
    dv = (pz.transpose(-1, -2) @ do).to(torch.bfloat16)[:, :, :S]
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, delta=delta[..., 0])


# ================================================================================================ index arithmetic
COVERAGE_REQUIRED = {"klo_gt_0", "khi_lt_S_minus_1", "first_tile_partly_visible", "last_tile_partly_visible", "tail_tile_with_keys_past_S",
                     "tile_skipped_by_the_mask", "one_tile_range", "key_block_without_a_valid_key", "key_block_partly_valid"}


def coverage(g):
    """Which branches of the generic kernels' index arithmetic a case reaches.  A restatement of attn_gen_fwd_kernel / attn_gen_dq_kernel
    (64-query blocks Q0, klo = max(0, Q0 - window), khi = min(S - 1, Q0 + 63 + window), tiles klo / 64 .. khi / 64, the per-key skip
    `kk < q - window || kk > q + window`, Ms[k] = key < S and valid) and of attn_gen_dkv_kernel (the same with 64-key blocks K0 and
    qlo / qhi over query tiles - the band labels are those of the transposed rule, which is the same rule -, key_ok per lane)."""
    S, w = g.S, g.case.window
    km = key_mask(g.case)
    km = km if km is not None else torch.ones(g.B, S, dtype=torch.bool)
    cov = set()
    for X0 in range(0, S, 64):
        lo, hi = (0, S - 1) if w < 0 else (max(0, X0 - w), min(S - 1, X0 + 63 + w))
        t0, t1 = lo // 64, hi // 64
        if lo > 0:
            cov.add("klo_gt_0")
        if hi < S - 1:
            cov.add("khi_lt_S_minus_1")
        if t0 == t1:
            cov.add("one_tile_range")
        rows = torch.arange(X0, min(S, X0 + 64))
        for t in range(t0, t1 + 1):
            cols = torch.arange(64 * t, 64 * t + 64)
            if int(cols[-1]) >= S:
                cov.add("tail_tile_with_keys_past_S")
            cols = cols[cols < S]
            if w >= 0:
                skip = (cols[None, :] < rows[:, None] - w) | (cols[None, :] > rows[:, None] + w)
                if bool(skip.any()) and not bool(skip.all()):
                    if t == t0:
                        cov.add("first_tile_partly_visible")
                    if t == t1:
                        cov.add("last_tile_partly_visible")
            if bool((~km[:, cols]).all(-1).any()):
                cov.add("tile_skipped_by_the_mask")
        ok = km[:, X0:X0 + 64]  # the dkv kernel's key_ok over this block's lanes
        if bool((~ok).all(-1).any()):
            cov.add("key_block_without_a_valid_key")
        if bool((ok.any(-1) & ~ok.all(-1)).any()):
            cov.add("key_block_partly_valid")
    return cov
