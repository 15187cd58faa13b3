"""References, derived bounds, case tables and CPU emulations of the dropout kernels: the element sites of csrc/elementwise.hip
(cm3p_dropout_f32, cm3p_geglu_fwd_dropout, cm3p_geglu_bwd_dropout, cm3p_dropout_keep) and the keep masks of head-64 attention with
dropout (csrc/attention.hip; its reference, bounds, table and emulation are tests/attention_refs.py's).  Shared by
tests/test_dropout_kernels_gpu.py (the kernels against them) and tests/test_dropout_refs_host.py (the correct emulations fit every
bound on every case, the wrong ones fail a named case).  No GPU here.

The mask.  Every keep mask is tests/test_dropout_host.py's keep_mask_ref, the numpy restatement of csrc/dropout_rng.h - never the
library's materialiser, which is itself one of the kernels under test.  A row t of an element site decides by (sequence b, position s
inside it): padded rows are (t / S, t mod S), packed rows the last sequence of cu_seqlens whose first row is <= t (a zero-length
sequence owns no row; the encoder's alignment rows are one more sequence of their own).

The contracts.
  cm3p_dropout_f32        bits: fl32(fl32(x * scale) + resid) where kept, fl32(0 + resid) where dropped (resid, or +0 without one);
                          scale = fl32(65536 / (65536 - thr)); the bf16 twin is the round-to-nearest-even of that fp32 value.  Two
                          roundings, no fused multiply-add: dropout_f32_path below IS the contract, compared with torch.equal.
  cm3p_geglu_fwd_dropout  gelu_erf(a) b Z, Z = 65536 / (65536 - thr), where kept and an exact zero where dropped.  The kernel's fp32
                          value carries the error of the GeGLU product (row_kernel_refs.geglu_fwd_ref32) times Z and one more fp32
                          rounding for the extra product (geglu_drop_fwd_kernel: `(gl.x * b[j]) * d.scale`); it is rounded to bf16 once.
  cm3p_geglu_bwd_dropout  the GeGLU derivative at dz = dg Z, UNROUNDED (geglu_drop_bwd_kernel hands the fp32 dz to geglu_bwd_item_f):
                          row_kernel_refs.geglu_bwd_ref32's error at dg Z plus one fp32 rounding for dg * scale, one rounding to bf16;
                          both halves are exact zeros where dropped.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import attention_refs as AR
import row_kernel_refs as RR
from row_kernel_refs import U
from test_dropout_host import keep_mask_ref, scale_ref, threshold_ref

SITE_EMBED, SITE_ATTN_PROBS, SITE_ATTN_OUT, SITE_MLP = 0, 1, 2, 3
DROPOUT_PS = AR.DROPOUT_PS
SEED = 0x5DEECE66D1234567
SEED_TOP_BIT = 0xC3A5C85C97CB3127  # bit 63 set
LAYER, LAYER_HIGH = 3, 11

MASK_WRONG = ("mask_shifted_group", "position_absolute", "seq_off_by_one", "halves_swapped")
ELEMENT_WRONG = MASK_WRONG + ("scale_missing", "bwd_rounds_dz")


# ================================================================================================ row layouts
@dataclass(frozen=True)
class Layout:
    name: str
    S: int                      # the entry points' S: positions per padded sequence; packed: the longest sequence (unread there)
    B: int = 0                  # padded: sequences
    lens: Optional[tuple] = None  # packed: the length of every sequence of cu_seqlens

    @property
    def packed(self):
        return self.lens is not None

    @property
    def cu(self):
        return tuple(int(c) for c in np.concatenate([[0], np.cumsum(self.lens)]))

    @property
    def rows(self):
        return self.cu[-1] if self.packed else self.B * self.S

    @property
    def n_seqs(self):
        return len(self.lens) if self.packed else self.B


def padded(B, S):
    return Layout(f"padded-{B}x{S}", S, B=B)


def packed(name, lens):
    return Layout(f"packed-{name}", max(lens), lens=tuple(lens))


def padded_twin(layout):
    """The padded batch with the same (sequence, position) pairs, and the rows of it the packed rows are."""
    twin = padded(layout.n_seqs, layout.S)
    b, s = rows_to_seq(layout)
    return twin, b * twin.S + s


# the packed layouts: mixed lengths with single-row sequences at both ends and 64 / 65 (a tile and one more), one sequence only,
# 300 sequences of one row (nine levels of the binary search, every row a first row), a zero-length sequence in the middle
# (cu = [0, 5, 5, 9]) and the encoder's own form: 153 tokens and a trailing pseudo-sequence of 39 alignment rows up to 192 = 3 * 64
PACKED = (packed("mixed", (1, 1, 7, 64, 65, 200, 1)), packed("one", (137,)), packed("ones300", (1,) * 300),
          packed("empty_middle", (5, 0, 4)), packed("encoder", (70, 33, 50, 39)))
PADDED_SMALL, PADDED_BIG = padded(2, 200), padded(8, 513)  # 400 rows; 4104 rows: past the 2048 x 256 grid at H = I = 1024
assert PADDED_BIG.rows * (1024 // 8) > 2048 * 256


def rows_to_seq(layout, wrong=None):
    """(b, s) of every row (numpy int64): cm3p_drop::row_to_seq restated.  wrong: 'position_absolute' (the row index as the position)
    or 'seq_off_by_one' (the binary search answers b - 1 at the first row of a sequence b >= 1)."""
    t = np.arange(layout.rows, dtype=np.int64)
    if not layout.packed:
        b = t // layout.S
        s = t - b * layout.S
    else:
        first = np.asarray(layout.cu[:-1], dtype=np.int64)
        b = np.searchsorted(first, t, side="right") - 1  # the last sequence whose first row is <= t
        if wrong == "seq_off_by_one":
            b = np.where((first[b] == t) & (b > 0), b - 1, b)
        s = t - first[b]
    if wrong == "position_absolute":
        s = t
    return b, s


def keep_rows(layout, F, layer, site, thr, seed, wrong=None):
    """bool [rows, F]: the contract's decision of every element of an element site, through keep_mask_ref.  wrong: one of MASK_WRONG."""
    b, s = rows_to_seq(layout, wrong)
    shift = 8 if wrong == "mask_shifted_group" else 0  # feature group c + 1
    m = keep_mask_ref(int(b.max()) + 1, int(s.max()) + 1, F + shift, layer, site, thr, seed)[b, s][:, shift:]
    if wrong == "halves_swapped":  # decision j from the 16-bit half j ^ 1
        m = m[:, np.arange(F) ^ 1]
    return torch.from_numpy(np.ascontiguousarray(m)).bool()


@functools.lru_cache(maxsize=None)
def keep_rows_cached(layout, F, layer, site, thr, seed):
    return keep_rows(layout, F, layer, site, thr, seed)


@functools.lru_cache(maxsize=None)
def attention_keep(case, thr, seed=SEED, layer=LAYER):
    """bool [B, NH, S, S] of head-64 attention: counters (key >> 3, query, b nh + h, 4 layer + 1)."""
    m = keep_mask_ref(case.B * AR.NH, case.S, case.S, layer, SITE_ATTN_PROBS, thr, seed)
    return torch.from_numpy(m).bool().view(case.B, AR.NH, case.S, case.S)


def z64(thr):
    """The dropout factor of the float64 references."""
    return 0.0 if thr >= 65536 else 65536.0 / (65536.0 - thr)


# ================================================================================================ element references and bounds
def geglu_fwd_dropout_ref(h, keep, thr):
    """h [T, 2I] float64 (bf16 values), keep bool [T, I] -> (ref, bound).  Dropped elements: ref 0 and bound 0 (exact)."""
    ref0, e0 = RR.geglu_fwd_ref32(h)
    Z = z64(thr)
    ref = ref0 * Z
    bound = RR.bf16_bound(ref, Z * e0 + U * ref.abs())
    return torch.where(keep, ref, torch.zeros_like(ref)), torch.where(keep, bound, torch.zeros_like(bound))


def geglu_bwd_dropout_ref(dg, h, keep, thr):
    """dg [T, I], h [T, 2I] float64, keep bool [T, I] -> (ref [T, 2I], bound)."""
    ref, e0 = RR.geglu_bwd_ref32(dg * z64(thr), h)
    bound = RR.bf16_bound(ref, e0 + U * ref.abs())
    kk = torch.cat([keep, keep], 1)
    return torch.where(kk, ref, torch.zeros_like(ref)), torch.where(kk, bound, torch.zeros_like(bound))


def check(got, ref, bound):
    """-> (worst error / bound over the elements with a bound > 0, the number of elements outside their bound).  An element with
    bound 0 (a dropped one) must be an exact zero; NaN fails."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    live = bound > 0
    worst = (err[live] / bound[live]).max().item() if bool(live.any()) else 0.0
    return (float("inf") if worst != worst else worst), int(bad.sum())


# ================================================================================================ fp32-path emulations
def _scale32(thr, wrong):
    return torch.tensor(1.0 if wrong == "scale_missing" else scale_ref(thr), dtype=torch.float32)


def _mask_wrong(wrong):
    return wrong if wrong in MASK_WRONG else None


def dropout_f32_path(x, resid, layout, layer, site, thr, seed, wrong=None):
    """The contract of cm3p_dropout_f32 in fp32 torch -> (y_f32, y_bf16).  wrong: one of MASK_WRONG or 'scale_missing'."""
    keep = keep_rows(layout, x.shape[1], layer, site, thr, seed, _mask_wrong(wrong))
    v = torch.where(keep, x * _scale32(thr, wrong), torch.zeros_like(x))
    if resid is not None:
        v = v + resid
    return v, v.to(torch.bfloat16)


def geglu_fwd_dropout_f32_path(h, layout, layer, thr, seed, wrong=None):
    """fp32 (a Phi(a) b) scale where kept, rounded to bf16 once (as row_kernel_refs.geglu_fwd_f32_path evaluates the product)."""
    I = h.shape[1] // 2
    keep = keep_rows(layout, I, layer, SITE_MLP, thr, seed, _mask_wrong(wrong))
    a, b = h[:, :I].float(), h[:, I:].float()
    gl = a * (0.5 * torch.special.erfc(a * torch.tensor(-1.0 / math.sqrt(2.0))))
    y = (gl * b) * _scale32(thr, wrong)
    return torch.where(keep, y, torch.zeros_like(y)).to(torch.bfloat16)


def geglu_bwd_dropout_f32_path(dg, h, layout, layer, thr, seed, wrong=None):
    """fp32 dz = dg scale where kept (0 where dropped) into the GeGLU derivative, each half rounded to bf16 once.  wrong also:
    'bwd_rounds_dz' (dz rounded to bf16 first, what a chain of the plain kernels would do)."""
    I = h.shape[1] // 2
    keep = keep_rows(layout, I, layer, SITE_MLP, thr, seed, _mask_wrong(wrong))
    a, b = h[:, :I].float(), h[:, I:].float()
    dz = torch.where(keep, dg.float() * _scale32(thr, wrong), torch.zeros(()))
    if wrong == "bwd_rounds_dz":
        dz = dz.to(torch.bfloat16).float()
    cdf = 0.5 * torch.special.erfc(a * torch.tensor(-1.0 / math.sqrt(2.0)))
    pdf = torch.exp(a * a * torch.tensor(-0.5)) * torch.tensor(1.0 / math.sqrt(2.0 * math.pi))
    return torch.cat([dz * b * (a * pdf + cdf), dz * (a * cdf)], 1).to(torch.bfloat16)


# ================================================================================================ element case tables
@dataclass(frozen=True)
class GegluCase:
    layout: Layout
    I: int
    p: float

    @property
    def name(self):
        return f"{self.layout.name}-I{self.I}-p{self.p}"

    @property
    def thr(self):
        return threshold_ref(self.p)


# (T, I) = (400, 8): one group per row; (400, 136): 17 groups; (4104, 1024): past the grid; the packed layouts at I = 136
GEGLU_CASES = ([GegluCase(PADDED_SMALL, I, p) for I in (8, 136) for p in DROPOUT_PS] + [GegluCase(PADDED_BIG, 1024, p) for p in DROPOUT_PS]
               + [GegluCase(lay, 136, p) for lay in PACKED for p in DROPOUT_PS])
GEGLU_BY_NAME = {c.name: c for c in GEGLU_CASES}


@functools.lru_cache(maxsize=None)
def geglu_data(T, I):
    """bf16 h [T, 2I] with the GELU tails planted (row_kernel_refs.geglu_h) and dg [T, I]; one draw per shape."""
    g = torch.Generator().manual_seed(8800 + 31 * T + I)
    return RR.geglu_h(T, I, g), torch.randn(T, I, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def geglu_reference(case):
    """-> dict(keep, fwd = (ref, bound), bwd = (ref, bound)) of one case at (LAYER, SEED); computed once and shared."""
    h, dg = geglu_data(case.layout.rows, case.I)
    keep = keep_rows_cached(case.layout, case.I, LAYER, SITE_MLP, case.thr, SEED)
    return dict(keep=keep, fwd=geglu_fwd_dropout_ref(h.double(), keep, case.thr), bwd=geglu_bwd_dropout_ref(dg.double(), h.double(), keep, case.thr))


def check_geglu(case, fwd=None, bwd=None):
    """-> (measured {quantity: worst error / bound}, failures) of a forward [T, I] and / or a backward [T, 2I] result."""
    ref = geglu_reference(case)
    seen, fails = {}, []
    for nm, got in (("geglu_fwd", fwd), ("geglu_bwd", bwd)):
        if got is None:
            continue
        want, bound = ref[nm[-3:]]
        seen[nm], nbad = check(got, want, bound)
        if nbad:
            fails.append(f"{nm}: {nbad} elements outside the bound, worst error / bound = {seen[nm]:.3f}")
        kk = ref["keep"] if nm == "geglu_fwd" else torch.cat([ref["keep"], ref["keep"]], 1)
        if bool((got.float()[~kk] != 0).any()):
            fails.append(f"{nm}: a dropped element is not an exact zero")
    return seen, fails


@functools.lru_cache(maxsize=None)
def f32_data(rows, H):
    g = torch.Generator().manual_seed(5100 + 7 * rows + H)
    return torch.randn(rows, H, generator=g), torch.randn(rows, H, generator=g)
