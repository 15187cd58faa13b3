"""Float64 references and derived error bounds of the masked-LM loss kernels, the remaining kernels of csrc/head.hip (inverse valid
count, the one-workgroup sum, scale_by, L2 normalisation, first-zero index) and of the masked-LM head as a whole, shared by
tests/test_loss_head_gpu.py (the kernels and the autograd nodes against them) and tests/test_loss_head_refs_host.py (a torch fp32
walk of each kernel's addition path against them, and wrong evaluations that must fail them).  No GPU and no cm3p_amd import here.

Conventions as tests/row_kernel_refs.py: u = 2^-24, one rounded fp32 operation moves its result by at most u |result|, every bound
counts the roundings along the kernel's longest path, states the count next to it and is multiplied once by SECOND; results below
FTZ may be flushed.  A stage's reference is fed the kernel's own inputs to that stage (dlogits gets the fp32 lse it is handed,
l2norm_bwd the fp32 y and norm).  expf and logf are taken as accurate to LIBM_ULPS units in the last place, an ulp being at most
2u of the result; the device library documents 1.
"""
import math

import torch
import torch.nn.functional as F

from row_kernel_refs import FTZ, SECOND, U, bf16_bound, bits_equal, check, gen  # noqa: F401  (re-exported to the two test files)
from row_kernel_refs import _wave_sum32

LIBM_ULPS = 2
LIBM = LIBM_ULPS * 2 * U  # relative error allowed to one expf / logf result
IGNORE = -100
PAD_VALUE = 3e38  # what the pad columns [cols, pitch) of a test's logits hold: a pad read as a logit shows up as inf


def _f32(v):
    """A Python float as the fp32 tensor a `float` kernel argument becomes."""
    return torch.tensor(v, dtype=torch.float32)


# ================================================================================================ masked cross entropy: data
# (cols, pitch): one column; below, at and past the 256-thread seam; the model's own padding; one 4096-column window exactly, a second
# window of a single 4-column group, three windows.  The pitch is a multiple of 4 (cm3p_ce_masked_dlogits_bf16 refuses others).
CE_COLS = ((1, 4), (37, 40), (255, 256), (256, 256), (257, 260), (3167, 3200), (4096, 4096), (4097, 4100), (8197, 8200))
CE_ROWS = (1, 63, 64, 65, 130)  # rows per 64-row workgroup of the dlogits kernel: 1, 63, 64, 64 + 1, 64 + 64 + 2
CE_SCALES = ((0.37, None), (-2.0, None), (0.0, None))  # (scale_a, scale_b); None: 1 / n, n = #(labels != IGNORE)
CE_KINDS = ("random", "all equal", "one +100 rest -100, target on the +100", "one +100 rest -100, target on a -100", "all about -90",
            "all about +88", "target at column 0", "target at column cols - 1", "label cols", "label -5", "label -100")
DL_ROWS, DL_WINDOW = 64, 4096  # csrc/head.hip: kDlRows, 4 * 256 * kDlQuads


def ce_case(cols, pitch, rows, g, first_block_ignored=False):
    """fp32 logits [rows, pitch] and int64 labels [rows]: row r < 22 is of kind CE_KINDS[r % 11] (twice each when rows allow), the
    rest N(0, 3^2) rows of which a third are ignored.  A single row is random; cols = 1 keeps only the kinds that do not need two
    columns.  first_block_ignored: rows 0 .. 63 all carry IGNORE (their data stays)."""
    x = torch.randn(rows, pitch, generator=g) * 3
    lab = torch.randint(0, cols, (rows,), generator=g)
    lab = torch.where(torch.rand(rows, generator=g) < 1 / 3, torch.full_like(lab, IGNORE), lab)
    kinds = []
    for r in range(rows):
        k = CE_KINDS[r % len(CE_KINDS)] if r < 2 * len(CE_KINDS) and rows > 1 else "random"
        if cols == 1 and k not in ("random", "all equal", "label cols", "label -5", "label -100"):
            k = "random"
        kinds.append(k)
        hot = int(torch.randint(0, cols, (1,), generator=g))
        if k == "random":
            lab[r] = int(torch.randint(0, cols, (1,), generator=g))
        elif k == "all equal":
            x[r] = 1.7
            lab[r] = hot
        elif k.startswith("one +100"):
            x[r] = -100.0
            x[r, hot] = 100.0
            lab[r] = hot if k.endswith("the +100") else (hot + 1) % cols
        elif k == "all about -90":
            x[r] = -90.0 + 0.01 * torch.randn(pitch, generator=g)
            lab[r] = hot
        elif k == "all about +88":
            x[r] = 88.0 + 0.01 * torch.randn(pitch, generator=g)
            lab[r] = hot
        elif k == "target at column 0":
            lab[r] = 0
        elif k == "target at column cols - 1":
            lab[r] = cols - 1
        else:
            lab[r] = {"label cols": cols, "label -5": -5, "label -100": IGNORE}[k]
    if first_block_ignored:
        lab[:DL_ROWS] = IGNORE
    x[:, cols:] = PAD_VALUE
    return x, lab, kinds


def ce_live(lab, cols):
    """Rows the loss kernels compute: the label is inside [0, cols).  (IGNORE and every other label outside are skipped.)"""
    return (lab >= 0) & (lab < cols)


# ================================================================================================ ce_masked_stats
def ce_sum_depth(cols):
    """Adds on the longest path of a row's sum of exponentials: ceil(cols / 256) sequential adds in a thread, six butterfly steps of
    wave_sum, two adds of (w0 + w1) + (w2 + w3)."""
    return -(-cols // 256) + 6 + 2


def ce_stats_ref(x, cols, lab):
    """x [rows, pitch] float64 (the fp32 logits), lab [rows] -> dict of float64 lse, loss (zero on skipped rows) and their bounds.
      mx: a maximum, exact.  d = fl(x - mx): u |d|, which moves exp(d) by u |d| exp(d).  e = expf(d): LIBM.  Every e <= 1 and the
      largest is exactly 1, so S = sum e >= 1 and a flushed e (d < -87) costs at most FTZ of it.
      S_k: sum_i e_i (u |d_i| + LIBM) / S + ce_sum_depth u =: rS relative.
      logf(S_k): |log S_k - log S| <= rS (1 + rS), then LIBM |log S|.  lse = fl(mx + .): u |lse|.
      loss = fl(lse_k - x[t]): u |loss| more.  The bound of loss does not vanish with the loss: a row with lse = 100 and loss ~ 0 keeps
      the absolute floor u |lse| (+ rS), which is the spacing of the fp32 numbers lse_k - x[t] is formed from."""
    live = ce_live(lab, cols)
    v = x[:, :cols]
    mx = v.max(1).values
    d = v - mx[:, None]
    e = torch.exp(d)
    S = e.sum(1)
    logS = torch.log(S)
    lse = mx + logS
    t = lab.clamp(0, cols - 1)
    xt = v.gather(1, t[:, None])[:, 0]
    loss = lse - xt
    rS = (e * (U * d.abs() + LIBM)).sum(1) / S + ce_sum_depth(cols) * U
    lse_b = (rS + LIBM * logS.abs() + U * lse.abs()) * SECOND + FTZ
    loss_b = lse_b + U * loss.abs() * SECOND
    z = torch.zeros_like(lse)
    return dict(live=live, lse=torch.where(live, lse, z), loss=torch.where(live, loss, z), lse_b=torch.where(live, lse_b, z),
                loss_b=torch.where(live, loss_b, z))


def ce_stats_f32_path(x, cols, lab, wrong=None):
    """ce_masked_stats_kernel in torch fp32: thread t adds columns t, t + 256, ... one after another, wave_sum, (w0 + w1) + (w2 + w3),
    logf, mx + ., . - x[t].  wrong: 'no_max' (log sum exp x) or 'sum_over_pitch' (the sum runs over the pad columns too).
    -> (loss_rows, lse_rows) fp32."""
    x = x.float()
    rows, pitch = x.shape
    live = ce_live(lab, cols)
    n = pitch if wrong == "sum_over_pitch" else cols
    mx = torch.zeros(rows) if wrong == "no_max" else x[:, :cols].max(1).values
    nch = -(-n // 256)
    e = torch.zeros(rows, nch * 256)
    e[:, :n] = torch.exp(x[:, :n] - mx[:, None])
    e = e.view(rows, nch, 256)
    se = torch.zeros(rows, 256)
    for c in range(nch):
        se = se + e[:, c]
    w = [_wave_sum32(se[:, 64 * i:64 * i + 64].contiguous()) for i in range(4)]
    lse = mx + torch.log((w[0] + w[1]) + (w[2] + w[3]))
    loss = lse - x.gather(1, lab.clamp(0, cols - 1)[:, None])[:, 0]
    z = torch.zeros(rows)
    return torch.where(live, loss, z), torch.where(live, lse, z)


# ================================================================================================ ce_masked_dlogits
def ce_colsum_depth(rows):
    """Adds on the longest path from a value to colsum[c]: a workgroup adds its min(rows, 64) rows one after another; colsum_final's
    wave takes per = ceil(nblk / 4) partials in four interleaved sums, ceil(per / 4) adds each, two adds combine the four, two more the
    four waves."""
    nblk = -(-rows // DL_ROWS)
    per = -(-nblk // 4)
    return min(rows, DL_ROWS) + -(-per // 4) + 2 + 2


def ce_dlogits_ref(x, cols, lab, lse_in, sa, sb):
    """x [rows, pitch] float64, lse_in [rows] float64 (the fp32 values the kernel is handed), sa / sb the fp32 scalars as floats
    -> dict g (float64, unrounded, [rows, pitch], zero on skipped rows and pad columns), dl_b (bound of the bf16 store), colsum,
    colsum_b.  s = fl(sa sb): u.  a = fl(x - lse): u |a|, which moves p = exp(a) by u |a| p; expf: LIBM p.  q = fl(p - onehot): u |q|
    (exact where p >= 1/2).  g = fl(s_k q_k): u.  So the fp32 value is within
        e32 = |s| (p (u |a| + LIBM) + 3u |q|)
    of g (s's rounding, q's and the product's: 3u |s q|), plus FTZ for an exponential flushed below the normal range, and the stored
    value within one bf16 rounding of that: bf16_bound.
    colsum[c] sums the unrounded fp32 values: sum_r e32 + ce_colsum_depth u sum_r |g|."""
    rows, pitch = x.shape
    live = ce_live(lab, cols)
    s = sa * sb
    a = torch.where(live[:, None], x[:, :cols] - lse_in[:, None], torch.zeros((), dtype=torch.float64))  # (skipped rows: not computed)
    p = torch.exp(a)
    onehot = torch.zeros(rows, cols, dtype=torch.float64)
    onehot[torch.arange(rows), lab.clamp(0, cols - 1)] = 1.0
    q = p - onehot
    m = live[:, None].double()
    g = torch.zeros(rows, pitch, dtype=torch.float64)
    e32 = torch.zeros(rows, pitch, dtype=torch.float64)
    g[:, :cols] = s * q * m
    e32[:, :cols] = (abs(s) * (p * (U * a.abs() + LIBM) + 3 * U * q.abs()) * SECOND + FTZ * (1 + abs(s))) * m
    dl_b = bf16_bound(g, e32) * torch.cat([m.expand(rows, cols), torch.zeros(rows, pitch - cols, dtype=torch.float64)], 1)
    colsum_b = (e32.sum(0) + ce_colsum_depth(rows) * U * g.abs().sum(0)) * SECOND
    return dict(g=g, dl_b=dl_b, e32=e32, colsum=g.sum(0), colsum_b=colsum_b, live=live)


def ce_dlogits_f32_path(x, cols, lab, lse_in, sa, sb, wrong=None):
    """ce_masked_dlogits_kernel + colsum_final_kernel in torch fp32 -> (dl bf16 [rows, pitch], colsum fp32 [pitch], partial fp32
    [nblk, pitch]).  wrong: 'onehot_t_plus_1', 'ignored_row_gradient' (a skipped row gets its softmax gradient all the same),
    'no_scale_b', 'colsum_of_rounded' (the column sums add the bf16 values)."""
    x, lse_in = x.float(), lse_in.float()
    rows, pitch = x.shape
    live = ce_live(lab, cols)
    s = _f32(sa) if wrong == "no_scale_b" else _f32(sa) * _f32(sb)
    t = lab.clamp(0, cols - 1)
    if wrong == "onehot_t_plus_1":
        t = (t + 1) % cols
    onehot = torch.zeros(rows, cols)
    onehot[torch.arange(rows), t] = 1.0
    g = torch.zeros(rows, pitch)
    g[:, :cols] = s * (torch.exp(x[:, :cols] - lse_in[:, None]) - onehot)
    if wrong == "ignored_row_gradient":
        fake = x[:, :cols].double().logsumexp(1).float()
        g[:, :cols] = torch.where(live[:, None], g[:, :cols], s * (torch.exp(x[:, :cols] - fake[:, None]) - onehot))
    else:
        g = torch.where(live[:, None], g, torch.zeros(()))  # (a skipped row is not computed at all: its lse_in is 0)
    dl = g.to(torch.bfloat16)
    add = dl.float() if wrong == "colsum_of_rounded" else g
    nblk = -(-rows // DL_ROWS)
    partial = torch.zeros(nblk, pitch)
    for r in range(rows):
        partial[r // DL_ROWS] = partial[r // DL_ROWS] + add[r]
    per = -(-nblk // 4)
    waves = []
    for w in range(4):
        b0, b1 = w * per, min(w * per + per, nblk)
        s4 = [torch.zeros(pitch) for _ in range(4)]
        b = b0
        while b + 3 < b1:
            for j in range(4):
                s4[j] = s4[j] + partial[b + j]
            b += 4
        while b < b1:
            s4[0] = s4[0] + partial[b]
            b += 1
        waves.append((s4[0] + s4[1]) + (s4[2] + s4[3]))
    return dl, (waves[0] + waves[1]) + (waves[2] + waves[3]), partial


# ================================================================================================ inv_valid_count, sum_f32, scale_by
REDUCE_N = (1, 1023, 1024, 1025, 3073, 4095, 4096, 4097, 7169, 131072 + 777)  # around the 1024-thread and 4096-element seams
SCALE_BY_N = (1, 255, 257, 262144 + 77)  # the last is past the 1024 x 256 grid: the grid-stride loop takes a second turn


def inv_valid_count_ref(lab, ignore=IGNORE, wrong=None):
    """fp32(1) / fp32(max(#(lab != ignore), 1)), one correctly rounded division of two exact fp32 numbers: equal in bits.  The rule is
    the header's: everything != ignore counts, a label outside the vocabulary too.  wrong: 'count_plus_1'."""
    n = int((lab != ignore).sum()) + (1 if wrong == "count_plus_1" else 0)
    return (_f32(1.0) / _f32(float(max(n, 1)))).reshape(1)


def sum_depth(n):
    """Roundings on the longest path of sum_kernel: ceil(n / 4096) adds in one of a thread's four sums and up to three more of the
    tail on the first, two adds combine the four, six butterfly steps, sixteen waves one after another, the product with scale."""
    return -(-n // 4096) + 3 + 2 + 6 + 16 + 1


def sum_ref(x, scale, out0=None):
    """x float64 [n], scale the fp32 argument as a float, out0 the fp32 value out[0] holds with accumulate -> (ref, bound):
    sum_depth u |scale| sum |x|, and with accumulate one more rounding of the result (fused or not, the product's own rounding is in
    the count)."""
    ref = scale * x.sum()
    b = sum_depth(x.numel()) * U * abs(scale) * x.abs().sum()
    if out0 is not None:
        ref = ref + out0
        b = b + U * abs(ref)
    return ref.reshape(1), (b * SECOND + FTZ).reshape(1)


def sum_f32_path(x, scale, out0=None, wrong=None):
    """sum_kernel in torch fp32.  wrong: 'drops_tail' (the elements past the last multiple of 4096 are not added)."""
    x = x.float()
    n = x.numel()
    s = [torch.zeros(1024) for _ in range(4)]
    # thread t's unrolled loop runs while t + 3072 + 4096 k < n: whole 4096-blocks for every thread, then the last, partial block for
    # the threads whose fourth element is still inside
    i = 0
    while i < n:
        blk = torch.zeros(4096)
        m = min(4096, n - i)
        blk[:m] = x[i:i + m]
        if m == 4096:
            for j in range(4):
                s[j] = s[j] + blk[1024 * j:1024 * j + 1024]
        elif wrong != "drops_tail":
            full = torch.arange(1024) + 3072 < m  # threads still in the unrolled loop
            for j in range(4):
                s[j] = s[j] + torch.where(full, blk[1024 * j:1024 * j + 1024], torch.zeros(()))
            for j in range(4):  # the others add their remaining elements to s0, in order
                s[0] = s[0] + torch.where(~full, blk[1024 * j:1024 * j + 1024], torch.zeros(()))
        i += 4096
    v = (s[0] + s[1]) + (s[2] + s[3])
    w = _wave_sum32(v.view(16, 64))
    r = torch.zeros(())
    for k in range(16):
        r = r + w[k]
    r = _f32(scale) * r
    return (r + out0.float() if out0 is not None else r).reshape(1)


def scale_by_ref(x, s):
    """The fp32 product, one IEEE operation: equal in bits."""
    return x.float() * s.float().reshape(())


# ================================================================================================ l2norm
L2_ROWS = (1, 3, 4, 5, 9)  # four rows per workgroup
L2_D = (1, 63, 64, 65, 512, 768, 1000)
L2_KINDS = ("random", "scaled 1e-3", "scaled 1e3", "one-hot", "one nonzero at the last column")


def l2_case(rows, D, g):
    """fp32 x, dy [rows, D]; row r is of kind L2_KINDS[r % 5]."""
    x = torch.randn(rows, D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    kinds = []
    for r in range(rows):
        k = L2_KINDS[r % len(L2_KINDS)]
        kinds.append(k)
        if k == "scaled 1e-3":
            x[r] *= 1e-3
        elif k == "scaled 1e3":
            x[r] *= 1e3
        elif k == "one-hot":
            v = x[r, (7 * r) % D].clone()
            x[r] = 0
            x[r, (7 * r) % D] = v if v != 0 else 1.0
        elif k.startswith("one nonzero"):
            v = x[r, D - 1].clone()
            x[r] = 0
            x[r, D - 1] = v if v != 0 else -2.5
    return x, dy, kinds


def l2_depth(D):
    """Roundings of a row's sum of products: ceil(D / 64) fused multiply-adds in a lane (one rounding each; an unfused product rounds
    once more, counted as the +1), six butterfly steps."""
    return -(-D // 64) + 1 + 6


def l2norm_fwd_ref(x):
    """x float64 [rows, D] -> dict y, norm and bounds.  ss_k = sum x^2 within l2_depth u ss (all terms positive); sqrtf halves the
    relative error and rounds once (2u covers a 1-ulp sqrtf): norm within (l2_depth / 2 + 2) u norm.  y = fl(x / norm_k): that
    relative error and the division's rounding (3u covers a 2.5-ulp division)."""
    ss = (x * x).sum(1)
    norm = ss.sqrt()
    rn = (l2_depth(x.shape[1]) / 2 + 2) * U
    y = x / norm[:, None]
    return dict(y=y, norm=norm, norm_b=rn * norm * SECOND + FTZ, y_b=(rn + 3 * U) * y.abs() * SECOND + FTZ)


def l2norm_fwd_f32_path(x, wrong=None):
    """l2norm_fwd_kernel in torch fp32 (unfused squares).  wrong: 'eps' (sqrt(ss + 1e-6))."""
    x = x.float()
    rows, D = x.shape
    nch = -(-D // 64)
    xp = torch.zeros(rows, nch * 64)
    xp[:, :D] = x
    xp = xp.view(rows, nch, 64)
    s = torch.zeros(rows, 64)
    for c in range(nch):
        s = s + xp[:, c] * xp[:, c]
    ss = _wave_sum32(s)
    if wrong == "eps":
        ss = ss + _f32(1e-6)
    norm = torch.sqrt(ss)
    return x / norm[:, None], norm


def l2norm_bwd_ref(dy, y, norm):
    """float64 dy, y [rows, D], norm [rows] (the kernel's fp32 inputs) -> (dx, bound), dx = (dy - y s) / norm, s = <y, dy>.
      s_k: l2_depth u sum |y dy| =: e_s.  t = fl(dy - fl(y s_k)) (or one fused operation): |y| e_s + u |y s| + u |t|.
      inv = fl(1 / norm): u.  dx = fl(t_k inv_k): 3u |dx| covers inv's rounding (2.5-ulp division included) and the product's."""
    D = y.shape[1]
    p = y * dy
    s = p.sum(1, keepdim=True)
    e_s = l2_depth(D) * U * p.abs().sum(1, keepdim=True)
    t = dy - y * s
    dx = t / norm[:, None]
    b = ((y.abs() * e_s + U * (y * s).abs() + U * t.abs()) / norm[:, None] + 3 * U * dx.abs()) * SECOND + FTZ
    return dx, b


def l2norm_bwd_f32_path(dy, y, norm, wrong=None):
    """l2norm_bwd_kernel in torch fp32.  wrong: 'no_projection' (dx = dy / norm) or 'times_norm' (multiplies by norm, not 1 / norm)."""
    dy, y, norm = dy.float(), y.float(), norm.float()
    rows, D = y.shape
    nch = -(-D // 64)
    pp = torch.zeros(rows, nch * 64)
    pp[:, :D] = y * dy
    pp = pp.view(rows, nch, 64)
    s = torch.zeros(rows, 64)
    for c in range(nch):
        s = s + pp[:, c]
    s = _wave_sum32(s)
    inv = norm if wrong == "times_norm" else 1.0 / norm
    if wrong == "no_projection":
        return dy * inv[:, None]
    return (dy - y * s[:, None]) * inv[:, None]


# ================================================================================================ first_zero_index
FZ_B = (1, 63, 64, 65, 200)  # 64 rows per workgroup
FZ_V = (1, 3, 17)


def fz_case(B, V, g):
    """int64 classes [B, V]: negative and large values, row b's zero placed by b % 4: first, last, absent, repeated (first and last)."""
    c = torch.randint(1, 2 ** 40, (B, V), generator=g) * (torch.randint(0, 2, (B, V), generator=g) * 2 - 1)
    for b in range(B):
        k = b % 4
        if k in (0, 3):
            c[b, 0] = 0
        if k in (1, 3):
            c[b, V - 1] = 0
        if k == 3 and V > 2:
            c[b, V // 2] = 0
    return c


def first_zero_ref(classes):
    return (classes == 0).int().argmax(1).to(torch.int64)


# ================================================================================================ the head as a whole
# (T, H, V): two row blocks + 2 with a small vocabulary; one block + 1 at Vp = 1024; the model's own padding 3167 -> 3200; V == Vp and
# exactly one row block.
HEAD_SHAPES = ((130, 64, 37), (65, 128, 1000), (130, 64, 3167), (64, 64, 128))
HEAD_MAX_LABELLED = 40
HEAD_EPS = 1e-5
GRADS = ("dh", "dWd", "dbd", "dnw", "dWdec", "dbdec")

# Margin of the node bound  |got - R| / |R| <= M |E - R| / |R|  over the distance between the float64 formula R and the same formula
# with the node's bf16 operand roundings E.  What the GPU adds to E is fp32 accumulation order and bf16 roundings that flip near ties,
# both small against E - R, so got - R is about E - R and 3 leaves a factor for the realisation of the rounding errors (E's float64
# GEMMs and the GPU's fp32 ones round the same operands, not the same sums).  The largest |got - R| / |E - R| measured over every
# variant of tests/test_loss_head_gpu.py is 1.003 (dbd; the loss 1.002, everything else within 1e-3 of 1: profiles/loss_head_err.txt,
# "node ..." entries).  That is below 1.5, so M stays at its starting value 3.
# M may not exceed 6: with at most 40 labelled rows a "mean" denominator that is off by one moves every quantity by at least 1 / 41.
M_NODE = 3.0
M_NODE_MAX = 6.0


def vp_of(V):
    return (V + 63) // 64 * 64


def head_params(T, H, V, g, bias=True):
    """fp32 h [T, H], Wd ~ N(0, 1 / H), bd, norm weight about 1, Wdec ~ N(0, 4 / H) (logits with spread), bdec."""
    return dict(h=torch.randn(T, H, generator=g), Wd=torch.randn(H, H, generator=g) / math.sqrt(H),
                bd=0.1 * torch.randn(H, generator=g) if bias else None, nw=1.0 + 0.1 * torch.randn(H, generator=g),
                Wdec=torch.randn(V, H, generator=g) * 2 / math.sqrt(H), bdec=0.1 * torch.randn(V, generator=g) if bias else None)


def head_labels(T, V, g, kind="quarter"):
    """int64 [T].  'quarter': about 25 % labelled, at most HEAD_MAX_LABELLED; 'none'; 'all'; 'out_of_range': 'quarter' with one label
    == V (skipped by the loss kernels, counted by the mean's denominator)."""
    lab = torch.randint(0, V, (T,), generator=g)
    if kind == "none":
        return torch.full((T,), IGNORE, dtype=torch.int64)
    if kind == "all":
        assert T <= HEAD_MAX_LABELLED
        return lab
    keep = torch.rand(T, generator=g) < 0.25
    keep[0], keep[T - 1] = True, False  # the first row labelled, the last ignored
    idx = keep.nonzero()[:, 0]
    keep[idx[HEAD_MAX_LABELLED - 1:]] = False  # (leaves room for the out-of-range one)
    lab = torch.where(keep, lab, torch.full_like(lab, IGNORE))
    lab[0], lab[int(idx[1])] = 0, V - 1  # the first and the last vocabulary entry are targets
    if kind == "out_of_range":
        lab[T - 1] = V
    return lab


class _GradBf16(torch.autograd.Function):
    """Identity whose backward rounds the gradient to bf16: a gradient tensor the node stores in bf16."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _round_ste(x):
    """The bf16 rounding of x with the gradient of the identity: a forward operand the node stores in bf16."""
    return x + (x.detach().to(torch.bfloat16).to(x.dtype) - x.detach())


def head_eval(p, lab, rounded, num_items=None, w_ext=None, dloss=1.0, use_loss=True, wrong=None, out_bf16=()):
    """The head's formula in float64 with autograd: logits = decoder(LayerNorm_no_bias(gelu_erf(dense(h)))), loss =
    F.cross_entropy(ignore_index=-100) (sum over the rows whose label is inside [0, V), divided by #(labels != -100), at least 1: the
    loss kernels skip a label outside the vocabulary while cm3p_inv_valid_count counts it, as include/cm3p_hip.h states), or that sum
    divided by num_items.  Objective: dloss * loss [+ (logits * w_ext).sum()].

    p: dict of h, Wd, bd | None, nw, Wdec, bdec | None holding the values the node is given (a bf16 parameter's bf16 values).
    rounded=False is R.  rounded=True is E: bf16 where _mlm_head_forward / _mlm_head_backward round -
      h, Wd, Wdec as GEMM operands; the LayerNorm output y; the gradient of the logits entering the decoder's dgrad / wgrad GEMMs
      (rounded once for the loss's part and once more after w_ext's part is added to it, as _MLMHeadLossFn.backward does; the decoder
      bias gradient sums the unrounded values); dy as linear_dgrad stores it; dz as bias_gelu_bwd stores it (the dense bias gradient
      sums the rounded values); and each returned gradient named in out_bf16 (a bf16 parameter's, a bf16 h's).
    wrong: 'denominator_plus_1', 'no_dbdec', 'ln_bwd_without_mean_dy', 'gelu_grad_without_x_pdf'.
    -> dict logits [T, V], loss, and the six gradients (None for an absent bias)."""
    q = {k: (v.detach().double().clone().requires_grad_(True) if v is not None else None) for k, v in p.items()}
    V = q["Wdec"].shape[0]
    op = _round_ste if rounded else (lambda t: t)
    gr = _GradBf16.apply if rounded else (lambda t: t)
    z = op(q["h"]) @ op(q["Wd"]).T
    if q["bd"] is not None:
        z = z + q["bd"]
    z = gr(z)
    cdf = 0.5 * torch.special.erfc(-z / math.sqrt(2.0))
    a = z * (cdf.detach() if wrong == "gelu_grad_without_x_pdf" else cdf)
    mean = a.mean(1, keepdim=True)
    c = a - (mean.detach() if wrong == "ln_bwd_without_mean_dy" else mean)
    eps = float(_f32(HEAD_EPS).double())
    y = c * ((c * c).mean(1, keepdim=True) + eps) ** -0.5 * q["nw"]
    y = op(gr(y))
    g0 = gr(y @ op(q["Wdec"]).T)
    bdec = q["bdec"] if q["bdec"] is not None else 0.0
    logits = g0 + bdec          # what w_ext's gradient enters through
    logits_l = gr(g0) + bdec    # the same values; the loss's gradient is rounded on its own first
    live = ce_live(lab, V)
    n = num_items if num_items is not None else max(int((lab != IGNORE).sum()), 1)
    if wrong == "denominator_plus_1":
        n = n + 1
    loss = F.cross_entropy(logits_l, torch.where(live, lab, torch.full_like(lab, IGNORE)), ignore_index=IGNORE, reduction="sum") / n
    obj = dloss * loss if use_loss else 0.0
    if w_ext is not None:
        obj = obj + (logits * w_ext.double()).sum()
    obj.backward()
    out = dict(logits=logits.detach(), loss=loss.detach())
    for name, key in zip(GRADS, ("h", "Wd", "bd", "nw", "Wdec", "bdec")):
        t = q[key]
        gd = None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t))
        if gd is not None and wrong == "no_dbdec" and name == "dbdec":
            gd = torch.zeros_like(gd)
        if gd is not None and rounded and name in out_bf16:
            gd = gd.to(torch.bfloat16).double()
        out[name] = gd
    return out


def rel_l2(a, b):
    """|a - b| / |b| (Frobenius), 0 / 0 = 0."""
    d, n = float((a.double() - b.double()).norm()), float(b.double().norm())
    return d / n if n > 0 else (0.0 if d == 0 else math.inf)


def node_check(got, R, E, what, m=M_NODE):
    """The node bound: |got - R| / |R| <= m |E - R| / |R|.  Prints and returns |got - R| / |E - R| (the ratio the margin is chosen
    from); NaN / inf in `got` fail."""
    got = got.detach().double().cpu()
    assert got.shape == R.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(R.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    e_got, e_E = rel_l2(got, R), rel_l2(E, R)
    assert e_E > 0, f"{what}: the rounded formula equals the float64 one; nothing to scale the bound by"
    ratio = e_got / e_E
    print(f"{what}: |got - R| / |R| {e_got:.3g}, |E - R| / |R| {e_E:.3g}, ratio {ratio:.3g} (margin {m:g})")
    assert e_got <= m * e_E, f"{what}: |got - R| / |R| = {e_got:.3g} above {m:g} x |E - R| / |R| = {m * e_E:.3g}"
    return ratio
