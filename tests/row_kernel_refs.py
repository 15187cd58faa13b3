"""Float64 references and derived per-element error bounds of the encoder's row kernels (csrc/norm.hip and the GeGLU / RoPE /
pooling part of csrc/elementwise.hip), shared by tests/test_row_kernels_gpu.py (the kernels against them) and
tests/test_row_kernel_bounds_host.py (a torch fp32 walk of the kernels' addition paths against them, and wrong evaluations that
must fail them).  No GPU and no cm3p_amd import here.

u = 2^-24 is the fp32 unit roundoff: one rounded operation moves its result by at most u |result|.  A chain of n roundings costs
(1 + u)^n - 1 <= n u (1 + n u); every bound below counts its roundings n along the kernel's longest addition path, states the count
next to it, and is multiplied once by SECOND = 1 + 1e-3 for the products of such terms that the first-order count leaves out
(n u < 1e-5 here, the row-dependent terms are stated where they are not small).  Results below ~1e-37 may be flushed to zero: FTZ.
"""
import math

import torch

from test_conv_head_kernels_gpu import _bits_equal as bits_equal  # noqa: F401  (one definition of the comparison semantics)
from test_conv_head_kernels_gpu import _check as check  # noqa: F401
from test_conv_head_kernels_gpu import _gelu64 as gelu64
from test_conv_head_kernels_gpu import _gelu_grad64 as gelu_grad64
from test_conv_head_kernels_gpu import _gen as gen  # noqa: F401
from test_conv_head_kernels_gpu import _phi_cdf as phi_cdf

U = 2.0 ** -24
SECOND = 1.0 + 1e-3
FTZ = 1e-37
LN_EPS = 1e-5
# the eps the kernels compute with: the fp32 nearest to 1e-5 (a `float eps` argument)
LN_EPS32 = float(torch.tensor(LN_EPS, dtype=torch.float32).double())


def half_ulp_bf16(v):
    """Half a bf16 ulp at |v| (float64 tensor): bf16 has an 8-bit significand, so for 2^e <= |v| < 2^(e+1) an ulp is 2^(e-7) and
    round-to-nearest-even moves a value by at most 2^(e-8).  That is between 2^-9 |v| and 2^-8 |v|: the relative form 2^-9 |v| is
    only its lower end and would refuse correctly rounded results just above a power of two.  Below the smallest normal the
    spacing is that of the smallest normal binade."""
    v = v.abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(v)  # v = m 2^e, 1/2 <= m < 1: floor(log2 v) = e - 1
    return torch.ldexp(torch.ones_like(v), e - 9)


def bf16_bound(ref, e32):
    """Bound of a bf16 result that is the RNE rounding of an fp32 value within e32 of ref: the fp32 value lies below |ref| + e32, so
    its rounding moves it by at most half an ulp of that binade."""
    return half_ulp_bf16(ref.abs() + e32) + e32


# ================================================================================================ LayerNorm
def ln_nc(H):
    """Live 256-column chunks of a row (CM3P_NC_SWITCH rounds 5, 6, 7 up to the NC = 8 instance; its empty chunks add exact zeros)."""
    return -(-H // 256)


def ln_depth(H):
    """Roundings on the longest path from an element to a row mean (row_stats, and s1 / s2 of the backward): two for the
    (x + y) + (z + w) of a lane's four values, one per chunk for the lane's running sum, six butterfly steps of wave_sum, one
    for the division by H."""
    return 2 + ln_nc(H) + 6 + 1


def ln_fwd_ref(x, w, eps=LN_EPS32):
    """x [R, H], w [H] float64 -> dict of float64 mean, rstd, y and the row quantities the bounds are written in."""
    H = x.shape[1]
    mean = x.mean(1)
    c = x - mean[:, None]
    var = (c * c).mean(1)
    rstd = (var + eps) ** -0.5
    D = ln_depth(H)
    # mean: D roundings over sum |x| / H
    mean_b = D * U * x.abs().mean(1) * SECOND
    # d = fl(x - mean_k) = c (1 + delta) + (mean - mean_k)(1 + delta): |d - c| <= u |c| + mean_b (1 + u)
    d_err = U * c.abs() + mean_b[:, None] * (1 + U)
    # var_k = fl(sum d^2 / H).  sum d^2 / H - var = 2 sum c eta / H + sum eta^2 / H with eta = d - c = c delta_i + dm (1 + delta_i),
    # dm = mean - mean_k constant over the row and sum c = 0: <= 2 u var + 2 u |dm| mean|c| + dm^2 (1 + u)^2 + u^2 var.  Its fp32
    # evaluation: one rounding for each square, then the D of the mean path: (D + 1) u (var + the above).
    mc = c.abs().mean(1)
    var_b = ((D + 3) * U * var + 2 * U * mean_b * mc + mean_b ** 2) * SECOND
    # rstd = 1 / sqrt(var_k + eps): the add, sqrtf and the division round once each when division and square root are correctly
    # rounded (hipcc's default), u/2 + u + u on rstd; 8 u also covers a 1-ulp sqrtf and a 2.5-ulp division.  var_k >= 0 whatever
    # the rounding (a sum of squares), so rstd_k <= eps^-1/2 (1 + 8u) always.
    lo = (var + eps + var_b) ** -0.5 * (1 - 8 * U)
    hi = torch.minimum((var - var_b).clamp_min(0.0) + eps, var + eps) ** -0.5 * (1 + 8 * U)
    rstd_b = torch.maximum(hi - rstd, rstd - lo)
    y = c * rstd[:, None] * w
    # y_k = fl(fl(d rstd_k) w): |d rstd_k - c rstd| <= |d - c| hi + |c| rstd_b, times |w|, plus the two products' roundings
    y_b = (w.abs() * (d_err * hi[:, None] + c.abs() * rstd_b[:, None]) + 2 * U * w.abs() * (c.abs() + d_err) * hi[:, None]) * SECOND + FTZ
    return dict(mean=mean, rstd=rstd, y=y, mean_b=mean_b, rstd_b=rstd_b, rstd_hi=hi, y_b=y_b, c=c)


def ln_bwd_ref(dy, x, w, mean, rstd, dres=None):
    """LayerNorm backward in float64 at the given statistics: dx = rstd (g - mean_H g - xhat mean_H(g xhat)) [+ dres], g = dy w,
    and the terms p = dy xhat of dw = sum_rows p.  dx_b bounds the kernel fed the same mean / rstd:
      g = fl(dy w): u |g|;  s1_k: (D + 1) u mean|g| (the mean path and g's rounding);  xhat_k: 2 u |xhat|;
      s2_k: (D + 4) u mean|g xhat| (g 1, xhat 2, the product 1, the path D);
      a = fl(fl(g_k - s1_k) - fl(xhat_k s2_k)): |a - t| <= 2u |g| + u |s1| + e_s1 + |xhat| (e_s2 + 3u |s2|) + u |t|;
      dx = fl(a rstd) [then fl(. + dres)]: one rounding each of the result."""
    H = x.shape[1]
    D = ln_depth(H)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    s1 = g.mean(1, keepdim=True)
    s2 = (g * xh).mean(1, keepdim=True)
    t = g - s1 - xh * s2
    dx_ln = t * rstd[:, None]
    dx = dx_ln + dres if dres is not None else dx_ln
    e_s1 = (D + 1) * U * g.abs().mean(1, keepdim=True)
    e_s2 = (D + 4) * U * (g * xh).abs().mean(1, keepdim=True)
    inner = 2 * U * g.abs() + U * s1.abs() + e_s1 + xh.abs() * (e_s2 + 3 * U * s2.abs()) + U * t.abs()
    dx_b = (rstd[:, None] * inner + U * dx_ln.abs() + (U * dx.abs() if dres is not None else 0)) * SECOND + FTZ
    return dict(dx=dx, dx_b=dx_b, p=dy * xh, xh=xh, g=g, s2=s2, t=t)


def ln_bwd_stats_slack(fwd, bwd, dy):
    """What the kernel's dx and dw terms may add to ln_bwd_ref's bounds when the reference runs at the float64 statistics while
    the kernel runs at its own (within fwd's mean_b / rstd_b): xhat moves by ex <= hi mean_b + |c| rstd_b, s2 by mean(|g| ex),
    t by |xhat| es2 + ex (|s2| + es2), dx by rstd_hi times that plus rstd_b |t|; a dw term by |dy| ex."""
    ex = fwd["rstd_hi"][:, None] * fwd["mean_b"][:, None] + fwd["c"].abs() * fwd["rstd_b"][:, None]
    es2 = (bwd["g"].abs() * ex).mean(1, keepdim=True)
    dx_s = fwd["rstd_hi"][:, None] * (bwd["xh"].abs() * es2 + ex * (bwd["s2"].abs() + es2)) + fwd["rstd_b"][:, None] * bwd["t"].abs()
    return dx_s * SECOND, (dy.abs() * ex) * SECOND


def ln_dw_c(rows, nblk):
    """Roundings from a term dy xhat to dw[col] (layernorm_bwd_kernel + colsum_kernel): xhat 2 and the product 1; a wave adds its
    ceil(rows / (4 nblk)) rows in registers; two adds combine a block's four waves; colsum's 32 slices take per = ceil(nblk / 32)
    partials each into eight accumulators (per // 8 adds, up to 7 more on the first), three adds combine the eight, eight adds a
    slice quarter and two the quarters.  dw is bounded by ln_dw_c u sum_rows |dy xhat|."""
    per = -(-nblk // 32)
    return 3 + -(-rows // (4 * nblk)) + 2 + per // 8 + 7 + 3 + 8 + 2


def ln_bwd_blocks(rows, cap=1024):
    """cm3p_layernorm_bwd_blocks restated (one block per four rows, capped)."""
    return max(1, min(cap, (rows + 3) // 4))


LN_SPECIAL_ROWS = ("mean 1e3, spread 1e-1", "mean 1e3 on the bf16 grid (spacing 4)", "constant 3.7", "constant 2.0", "all zero",
                   "N(0,1) with one element 1e4")


def ln_special_rows(H, g):
    """One row of each kind of LN_SPECIAL_ROWS, fp32 [6, H]."""
    x = torch.zeros(6, H)
    x[0] = 1e3 + 1e-1 * torch.randn(H, generator=g)
    x[1] = 1000.0 + 4.0 * torch.randint(-1, 2, (H,), generator=g).float()
    x[2] = 3.7
    x[3] = 2.0
    x[5] = torch.randn(H, generator=g)
    x[5, H // 3] = 1e4
    return x


# ---- the kernel's addition path in torch fp32 on the CPU (elementwise IEEE operations: the same roundings, no fused multiply-add)
def _wave_sum32(v):
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def _lanes(x):
    """[R, H] fp32 -> [R, nc, 64, 4] zero-padded (lane l of chunk c owns columns 256 c + 4 l .. + 3) and the live-column mask."""
    R, H = x.shape
    nc = ln_nc(H)
    xp = torch.zeros(R, nc * 256, dtype=torch.float32)
    xp[:, :H] = x
    live = torch.zeros(nc * 256, dtype=torch.bool)
    live[:H] = True
    return xp.view(R, nc, 64, 4), live.view(nc, 64, 4)


def _row_sum32(v):
    s = torch.zeros(v.shape[0], 64, dtype=torch.float32)
    for c in range(v.shape[1]):
        s = s + ((v[:, c, :, 0] + v[:, c, :, 1]) + (v[:, c, :, 2] + v[:, c, :, 3]))
    return _wave_sum32(s)


def ln_fwd_f32_path(x, w, eps=LN_EPS, wrong=None):
    """row_stats + store_norm in fp32.  wrong: 'mean_h_minus_1' (the mean over the first H - 1 columns) or 'one_pass'
    (var = E[x^2] - mean^2)."""
    x, w = x.float(), w.float()
    H = x.shape[1]
    Hf, eps = torch.tensor(float(H)), torch.tensor(eps, dtype=torch.float32)
    v, live = _lanes(x)
    if wrong == "mean_h_minus_1":
        x1 = x.clone()
        x1[:, H - 1] = 0
        mean = _row_sum32(_lanes(x1)[0]) / torch.tensor(float(H - 1))
    else:
        mean = _row_sum32(v) / Hf
    if wrong == "one_pass":
        var = _row_sum32(v * v) / Hf - mean * mean
    else:
        d = torch.where(live, v - mean[:, None, None, None], torch.zeros(()))
        var = _row_sum32(d * d) / Hf
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None] * w
    return y, mean, rstd


def ln_bwd_f32_path(dy, x, w, mean, rstd, dres=None, wrong=None):
    """layernorm_bwd_kernel in fp32 with the rows added to dw one after another.  wrong: 'dw_drops_a_row'."""
    dy, x, w = dy.float(), x.float(), w.float()
    R, H = x.shape
    Hf = torch.tensor(float(H))
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    s1 = _row_sum32(_lanes(g)[0]) / Hf
    s2 = _row_sum32(_lanes(g * xh)[0]) / Hf
    dx = (g - s1[:, None] - xh * s2[:, None]) * rstd[:, None]
    if dres is not None:
        dx = dx + dres.float()
    p = dy * xh
    dw = torch.zeros(H, dtype=torch.float32)
    for r in range(R):
        if wrong == "dw_drops_a_row" and r == R // 2:
            continue
        dw = dw + p[r]
    return dx, dw


# ================================================================================================ GeGLU
GELU_FIT_REL = 3.3e-6  # csrc/common.h: the erfcc fit of Phi "3.3e-6 as evaluated here in fp32 over EVERY bf16 input", relative
GELU_MARGIN = 2.0      # twice that: the products a Phi(a) and (.) b add one fp32 rounding each (2u = 1.2e-7 of the result)


def geglu_fwd_ref32(h):
    """h [R, 2I] float64 (bf16 values) -> (ref, e32): y = gelu_erf(a) b, a = h[:, :I], b = h[:, I:], and the error of the kernel's
    fp32 value before it is rounded to bf16 (tests/dropout_refs.py multiplies both by the dropout factor before that rounding)."""
    I = h.shape[1] // 2
    a, b = h[:, :I], h[:, I:]
    ref = gelu64(a) * b
    return ref, GELU_MARGIN * GELU_FIT_REL * ref.abs() + FTZ


def geglu_fwd_ref(h):
    """-> (ref, bound) of y = gelu_erf(a) b rounded to bf16."""
    ref, e32 = geglu_fwd_ref32(h)
    return ref, bf16_bound(ref, e32)


def geglu_bwd_ref32(dg, h):
    """-> (ref [R, 2I], e32): d/da = dg b gelu'(a), d/db = dg gelu(a) and the error of the kernel's fp32 values.  gelu'(a) =
    Phi(a) + a phi(a) can vanish (a ~ -0.75) where neither of its terms does, so its fp32 error is taken against Phi(a) + |a| phi(a):
    both terms come out of exponentials of the same fp32 argument -a^2 / 2 log2 e, the source of the fit's 3.3e-6."""
    I = h.shape[1] // 2
    a, b = h[:, :I], h[:, I:]
    pdf = torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    da = dg * b * gelu_grad64(a)
    db = dg * gelu64(a)
    e_da = GELU_MARGIN * GELU_FIT_REL * (dg * b).abs() * (phi_cdf(a) + a.abs() * pdf) + FTZ
    e_db = GELU_MARGIN * GELU_FIT_REL * db.abs() + FTZ
    return torch.cat([da, db], 1), torch.cat([e_da, e_db], 1)


def geglu_bwd_ref(dg, h):
    """-> (ref [R, 2I], bound), each half rounded to bf16."""
    ref, e32 = geglu_bwd_ref32(dg, h)
    return ref, bf16_bound(ref, e32)


def geglu_h(T, I, g):
    """bf16 h [T, 2I]: N(0, 2^2) with |a| up to 12 (the negative tail of Phi and its mirror) and zeros planted in every row."""
    h = (torch.randn(T, 2 * I, generator=g) * 2).to(torch.bfloat16)
    planted = torch.tensor([-12.0, 12.0, -8.5, -6.0, -0.75, 0.0, -0.0, 5.0], dtype=torch.bfloat16)
    h[:, :8] = planted  # a of the first item of each row (b stays random, both signs)
    return h


def geglu_fwd_f32_path(h, wrong=None):
    """fp32 a Phi(a) b with Phi = erfc(-a / sqrt 2) / 2 (relative accuracy in the negative tail, as the kernel's fit), rounded to
    bf16.  wrong: 'tanh' (the tanh approximation of GELU) or 'swapped' (gelu(b) a)."""
    I = h.shape[1] // 2
    a, b = h[:, :I].float(), h[:, I:].float()
    if wrong == "swapped":
        a, b = b, a
    if wrong == "tanh":
        gl = torch.nn.functional.gelu(a, approximate="tanh")
    else:
        gl = a * (0.5 * torch.special.erfc(a * torch.tensor(-1.0 / math.sqrt(2.0))))
    return (gl * b).to(torch.bfloat16)


def geglu_bwd_f32_path(dg, h):
    I = h.shape[1] // 2
    a, b, d = h[:, :I].float(), h[:, I:].float(), dg.float()
    cdf = 0.5 * torch.special.erfc(a * torch.tensor(-1.0 / math.sqrt(2.0)))
    pdf = torch.exp(a * a * torch.tensor(-0.5)) * torch.tensor(1.0 / math.sqrt(2.0 * math.pi))
    return torch.cat([d * b * (a * pdf + cdf), d * (a * cdf)], 1).to(torch.bfloat16)


# ================================================================================================ RoPE
def rope_inv_freq(theta, head_dim):
    """The fp32 inverse frequencies theta^(-2j / head_dim), j < head_dim / 2 (any fp32 vector serves as the kernel's input)."""
    return (1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))).float()


def rope_table_ref(pos, inv_freq):
    """The documented contract: ONE fp32 product float(pos) * inv_freq (IEEE: the same bits on any machine), then cos / sin of
    that fp32 angle - here in float64."""
    ang = (pos.reshape(-1, 1).float() * inv_freq.reshape(1, -1).float()).double()
    return torch.cos(ang), torch.sin(ang)


def rope_apply_ref(qkv, cos, sin, inverse):
    """qkv [B, S, 3, nh, D] float64 (bf16 values), cos / sin [B or 1, S, D / 2] float64 (the kernel's fp32 tables) -> (ref, bound)
    for the q and k thirds: pairs (j, j + D / 2), y1 = x1 c -+ x2 s, y2 = x2 c +- x1 s in fp32 (two products and a sum: three
    roundings, each at most u times the sum of the two |terms|), rounded once to bf16."""
    half = qkv.shape[-1] // 2
    x1, x2 = qkv[:, :, :2, :, :half], qkv[:, :, :2, :, half:]
    c, s = cos[:, :, None, None, :], sin[:, :, None, None, :]
    sg = -1.0 if inverse else 1.0
    y1 = x1 * c - sg * x2 * s
    y2 = x2 * c + sg * x1 * s
    e1 = 3 * U * ((x1 * c).abs() + (x2 * s).abs()) + FTZ
    e2 = 3 * U * ((x2 * c).abs() + (x1 * s).abs()) + FTZ
    return torch.cat([y1, y2], -1), torch.cat([bf16_bound(y1, e1), bf16_bound(y2, e2)], -1)


# ================================================================================================ pooling
POOL_CHUNK = 128


def pool_ref(h, mask, cls):
    """h [Bn, S, H] float64, mask [Bn, S] (0 / 1) or None -> (pooled, count, bound).  cls: row 0, exact.  Mean: pool_partial_kernel
    adds a chunk's min(S, 128) products h m (exact for m in {0, 1}) one after another, pool_final_kernel the chunks one after
    another, then one product with fl(1 / count) (or one division by S): min(S, 128) + nchunks + 2 roundings over
    sum |h m| / count.  count is a sum of at most S <= 2^24 ones: exact.  A row with no kept position: sum 0 times 1 / 1e-9 = 0.
    (A chain of n one-after-another adds of random-sign terms errs like sqrt(n) u, so random data sits near 1 / sqrt(n) of this
    worst case - a few hundredths; the bound is still two orders below one position counted by mistake, which the host test shows.)"""
    Bn, S, H = h.shape
    if cls:
        return h[:, 0], torch.full((Bn,), float(S), dtype=torch.float64), torch.zeros(Bn, H, dtype=torch.float64)
    m = torch.ones(Bn, S, dtype=torch.float64) if mask is None else mask.double()
    count = m.sum(1)
    den = count.clamp_min(1e-9)[:, None]
    pooled = (h * m[:, :, None]).sum(1) / den
    n = min(S, POOL_CHUNK) + -(-S // POOL_CHUNK) + 2
    bound = n * U * (h.abs() * m[:, :, None]).sum(1) / den * SECOND
    return pooled, count, bound


def pool_bwd_ref(dp, mask, count, S, cls):
    """dh[b, s] = dp[b] scale(b, s) -> (ref, bound).  cls: scale in {0, 1}, a product of two floats with an exact result.  Mean:
    scale = fl(m / max(count, 1e-9)) or fl(1 / S), one rounded division (u; 3u covers a 2.5-ulp division rounded either way less
    the product's own u) and the product: 4u |ref|; exactly zero where m = 0."""
    Bn, H = dp.shape
    if cls:
        sc = torch.zeros(Bn, S, dtype=torch.float64)
        sc[:, 0] = 1.0
    elif mask is None:
        sc = torch.full((Bn, S), 1.0 / S, dtype=torch.float64)
    else:
        sc = mask.double() / count.clamp_min(1e-9)[:, None]
    ref = dp[:, None, :] * sc[:, :, None]
    return ref, (0.0 if cls else 4 * U) * ref.abs()


def pool_fwd_f32_path(h, mask, wrong=None):
    """The two pooling kernels' sums in fp32, position after position and chunk after chunk.  wrong: 'counts_a_masked_row' (one
    position with m = 0 is added all the same)."""
    h = h.float()
    Bn, S, H = h.shape
    m = torch.ones(Bn, S) if mask is None else mask.float()
    madd = m.clone()
    if wrong == "counts_a_masked_row":
        b, s = (m == 0).nonzero()[0].tolist()
        madd[b, s] = 1.0
    tot = torch.zeros(Bn, H)
    for s0 in range(0, S, POOL_CHUNK):
        acc = torch.zeros(Bn, H)
        for s in range(s0, min(S, s0 + POOL_CHUNK)):
            acc = acc + h[:, s] * madd[:, s, None]
        tot = tot + acc
    if mask is None:
        return tot / torch.tensor(float(S))
    inv = 1.0 / m.sum(1).clamp_min(1e-9)
    return tot * inv[:, None]
