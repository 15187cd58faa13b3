"""Float64 references, fp32 path restatements, derived bounds and the case tables of the optimizer step's kernels (csrc/muon.hip behind
cm3p_muon_partials / _momentum / _normalize / _apply and cm3p_adamw_multi) and of one Newton-Schulz iteration as cm3p_amd.muon's
newton_schulz_batched issues it (three cm3p_gemm_bf16_batched calls), shared by tests/test_muon_kernels_gpu.py (the kernels against
them) and tests/test_muon_refs_host.py (the path restatements must pass, the wrong evaluations must fail).  No GPU and no cm3p_amd
import here.

Every operation has a `*_check` (what the GPU test asserts: the float64 meaning with a bound counted from the kernel's roundings, or the
exact bits where the operation is a chain of single IEEE operations) and a `*_f32_path` (the kernel's arithmetic in torch fp32 on the
CPU, rounding where the kernel rounds; `wrong=` names the evaluations a kernel could fall into).  Each stage is checked from the
kernel's OWN previous output, so a bound never has to carry an earlier stage's error.

u = 2^-24, SECOND = 1 + 1e-3, FTZ, bf16_bound and half_ulp_bf16 are those of tests/row_kernel_refs.py.  torch's CPU elementwise ops are
single IEEE operations, its fp32 -> bf16 conversion is RNE, and its fp32 sqrt and division are correctly rounded - as the GPU's are
under hipcc's defaults (cm3p_amd/build.py FLAGS pass nothing that relaxes them).
"""
import math

import torch

import gemm_refs as G
from row_kernel_refs import FTZ, SECOND, U, bf16_bound, bits_equal, check, gen, half_ulp_bf16  # noqa: F401
from row_kernel_refs import _wave_sum32

MOMENTUM = 0.95
NS_EPS = 1e-7                               # cm3p_amd.muon.NS_EPS restated (the GPU test compares the two)
NS_A, NS_B, NS_C = 3.4445, -4.7750, 2.0315  # cm3p_amd.muon.NS_A / NS_B / NS_C restated
N_MAT = 3
EPI_AXPBY = 4
K128, KRING = 0, 2                          # cm3p_gemm_route's kernel numbers


def f32(v):
    """The fp32 nearest to a Python float, as a 0-d tensor: what a `float` argument of a C entry point holds."""
    return torch.tensor(v, dtype=torch.float32)


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 tensors: the product of two fp32 numbers is exact in float64 (48 bits), its sum with an fp32 number is
    rounded to float64 and then to fp32.  Where that first rounding matters (a sum needing more than 53 bits that lands within 2^-53
    of an fp32 tie) the result can be the other neighbour of the exact value; no check below is bit for bit on a value made here."""
    return (a.double() * b.double() + c.double()).float()


def up8(n):
    return (n + 7) // 8 * 8


def rne64_bf16(x):
    """float64 -> bf16 in ONE round-to-nearest-even (torch converts float64 -> fp32 -> bf16, two roundings), normal range."""
    m, e = torch.frexp(x)  # 1/2 <= |m| < 1
    return torch.ldexp(torch.round(m * 256.0), e - 8).float().to(torch.bfloat16)


def half_ulp_f32(v):
    """Half an fp32 ulp at |v| (float64 tensor): 2^(e - 24) for 2^e <= |v| < 2^(e + 1): the most that ONE rounding of the exact value v
    to fp32 moves it."""
    v = v.abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 25)


# ================================================================================================ case tables
# (rows, cols): the smallest shapes that reach each seam of the stage kernels
STAGE_SHAPES = [
    (8, 4),
    (13, 21),      # odd, ldx 24
    (24, 30),      # cols % 4 = 2
    (96, 32),
    (128, 128),    # exactly 16384 elements: one block
    (113, 145),    # 16385 elements: two blocks, scalar
    (129, 128),    # two blocks, float4
    (1032, 1020),  # 1 052 640 elements: 65 blocks wanted, 64 given, the last one short; apply and normalise loop past 128 blocks
]
DATA_SHAPES = [(13, 21), (96, 32)]  # the two data cases: 'tiny' (magnitude 1e-8) and 'zero_mat' (one all-zero matrix of the three)
STAGE_CASES = [(r, c, "normal") for r, c in STAGE_SHAPES] + [(r, c, kind) for kind in ("tiny", "zero_mat") for r, c in DATA_SHAPES]
ZERO_MAT = 1  # which matrix of a 'zero_mat' group is all zero

ADAMW_NUMELS = [1, 255, 1024, 1025, 65536, 65537, 200003]
ADAMW_LAUNCHES = {"all": ADAMW_NUMELS, "first3": ADAMW_NUMELS[:3]}  # first3: max_numel 1024 -> a grid of one block
ADAMW_WEIGHTS = [(0.1, 0.05), (0.6, 0.7)]  # both branches of torch.lerp's weight test
ADAMW_DECAYS = [1.0, 1.0 - 5e-5]
ADAMW_EPS = 1e-8
ADAMW_STEP_ALPHA = -0.02 / ((1 - 0.9 ** 3) / (1 - 0.95 ** 3) ** 0.5)  # -lr / scale of the third step at betas (0.9, 0.95)

# (n, rows, cols) of one Newton-Schulz iteration; the last two reach the ring kernel in all three calls
NS_SMALL = [(1, 13, 21), (1, 21, 13), (2, 32, 32), (3, 96, 32), (3, 32, 48)]
NS_RING = [(32, 768, 512), (32, 512, 768)]
NS_CASES = NS_SMALL + NS_RING
NS_ODD = [(1, 13, 21), (1, 21, 13)]
NS_RING_DISTINCT = 3


def ns_ring_order(n):
    """Which of the 3 distinct matrices each of the n ring-case matrices copies: a fixed shuffle that uses all three."""
    order = torch.randperm(n, generator=gen("ns-ring-order", n)) % NS_RING_DISTINCT
    assert set(order.tolist()) == set(range(NS_RING_DISTINCT))
    return order


# ================================================================================================ data
def stage_data(rows, cols, kind, n=N_MAT):
    """-> fp32 g, buf (a non-zero starting buffer), p [n, rows, cols], distinct per matrix.  'tiny': gradient and buffer of magnitude
    1e-8, so that ||X|| ~ 1e-7 sqrt(numel / 100) and bf16(norm + eps) differs from norm.  'zero_mat': matrix ZERO_MAT has a zero gradient
    and a zero buffer (a weight no batch has used yet)."""
    gn = gen("muon-stage", rows, cols, kind)
    g = torch.randn(n, rows, cols, generator=gn) * 0.1
    buf = torch.randn(n, rows, cols, generator=gn) * 0.3
    p = torch.randn(n, rows, cols, generator=gn) * 0.5
    if kind == "tiny":
        g, buf = g * 1e-7, buf * 1e-7
    elif kind == "zero_mat":
        g[ZERO_MAT], buf[ZERO_MAT] = 0.0, 0.0
    return g, buf, p


def adamw_data(numels, w):
    """Per tensor fp32 p, g, m1, m2 (m2 in [0.0025, 0.0125]: |u| stays below ~5, so that 3 u |alpha u| stays inside the fixture test's
    tolerance at every element).  Every seventh element has g = 0 and m2 = 0 (m2' = 0: the denominator is eps alone), there m1 is of
    magnitude 1e-9 so that the step m1' / eps stays of order 0.1."""
    out = []
    for numel in numels:
        gn = gen("muon-adamw", numel, w)
        p = torch.randn(numel, generator=gn) * 0.5
        g = torch.randn(numel, generator=gn) * 0.1
        m1 = torch.randn(numel, generator=gn) * 0.05
        m2 = 0.0025 + 0.01 * torch.rand(numel, generator=gn)
        z = torch.arange(numel) % 7 == 0
        g[z], m2[z], m1[z] = 0.0, 0.0, m1[z] * 1e-8
        out.append((p, g, m1, m2))
    return out


def ns_data(n, rows, cols):
    """Normalised iterates as the stage kernels leave them: bf16 [n, rows, cols] of Frobenius norm ~ 1 (singular values inside the
    quintic's band), zero-padded to [n, rp, cp].  Ring cases: copies of NS_RING_DISTINCT distinct matrices in ns_ring_order."""
    gn = gen("muon-ns", n, rows, cols)
    distinct = min(n, NS_RING_DISTINCT) if (n, rows, cols) in NS_RING else n
    x = (torch.randn(distinct, rows, cols, generator=gn) / math.sqrt(rows * cols)).to(torch.bfloat16)
    if distinct != n:
        x = x[ns_ring_order(n)]
    img = torch.zeros(n, up8(rows), up8(cols), dtype=torch.bfloat16)
    img[:, :rows, :cols] = x
    return img


# ================================================================================================ momentum
def momentum_f32_path(g, buf, momentum, nesterov, wrong=None):
    """muon_momentum_kernel's element math -> (buf', u, X).  wrong: 'one_rounding' (buf' = fma(buf, m, g)), 'u_is_buf' (u = buf' in
    place of g + m buf'), 'flag_ignored' (the other value of nesterov), 'trunc' (X truncated, not rounded to nearest)."""
    m = f32(momentum)
    buf2 = fma32(buf, m, g) if wrong == "one_rounding" else buf * m + g
    if wrong == "flag_ignored":
        nesterov = not nesterov
    if wrong == "u_is_buf":
        u = buf2
    else:
        u = fma32(m, buf2, g) if nesterov else g.clone()
    x = G.trunc_bf16(u).to(torch.bfloat16) if wrong == "trunc" else u.to(torch.bfloat16)
    return buf2, u, x


def momentum_check(got_buf, got_x, g, buf, momentum, nesterov, what):
    """buf' = fl32(fl32(buf m) + g) bit for bit (buf.mul_(m).add_(g) is two kernels in the reference: two roundings).  X against the
    float64 u = g + m buf' taken from the kernel's own buf' (u = g without nesterov): the fma rounds u once (u |u|), then one bf16
    rounding: bf16_bound(u64, u |u64|).  Returns X's err / bound."""
    m = f32(momentum)
    bits_equal(got_buf, buf * m + g, f"{what}: buf'")
    u64 = g.double() + float(m) * got_buf.double() if nesterov else g.double()
    return check(got_x.float(), u64, bf16_bound(u64, U * u64.abs()), f"{what}: X")


# ================================================================================================ partials
def n_partials(rows, cols):
    """cm3p_muon_partials restated: one block per 16384 elements, at most 64."""
    return max(1, min(64, -(-(rows * cols) // 16384)))


def is_vec(cols, aligned16):
    """cm3p_muon_momentum's choice: the float4 kernel when rows end on a quad and the host vouches for 16-byte aligned pointers."""
    return cols % 4 == 0 and bool(aligned16)


def partition(rows, cols, vec):
    """-> (per, [(beg, end) in elements per block]).  The float4 kernel splits numel / 4 quads into ceil(n4 / blocks) per block, the
    scalar kernel numel elements the same way; the last block takes what is left (possibly nothing)."""
    q = 4 if vec else 1
    n = rows * cols // q
    blocks = n_partials(rows, cols)
    per = -(-n // blocks)
    return per, [(min(n, per * b) * q, min(n, per * b + per) * q) for b in range(blocks)]


def partials_depth(per, vec):
    """Roundings on the longest path from a square to a block's partial.  The squares are exact (a bf16 value has 8 significand
    bits).  A thread makes ceil(per / 256) passes; a scalar pass is one add into its sum, a float4 pass three adds for the quad and
    one into the sum.  Then six butterfly levels of wave_sum and the four wave sums added one after another."""
    return (4 if vec else 1) * -(-per // 256) + 6 + 4


def partials_f32_path(x, rows, cols, vec, wrong=None, u=None):
    """One matrix: x bf16 [rows, cols] -> fp32 [blocks], every thread's chain, the butterfly and the ordered wave sums as the kernel
    adds them.  wrong: 'tail_dropped' (the last block leaves out its last pass of 256 threads), 'block_twice' (block 1 sums block 0's
    range again - with a single block its sum is doubled), 'sum_of_u2' (squares of the fp32 u, not of the rounded X)."""
    v = (u if wrong == "sum_of_u2" else x).float().reshape(-1)
    q = 4 if vec else 1
    _, ranges = partition(rows, cols, vec)
    out = []
    for b, (beg, end) in enumerate(ranges):
        if wrong == "tail_dropped" and b == len(ranges) - 1:
            left = (end - beg) % (256 * q)
            end -= left if left else min(256 * q, end - beg)
        if wrong == "block_twice" and b == 1:
            beg, end = ranges[0]
        sq = v[beg:end] * v[beg:end]
        passes = -(-(end - beg) // (256 * q))
        lanes = torch.zeros(passes * 256 * q)
        lanes[:end - beg] = sq
        lanes = lanes.view(passes, 256, q)  # thread t of pass k owns item beg / q + 256 k + t
        ss = torch.zeros(256)
        for k in range(passes):
            t = lanes[k]
            ss = ss + (((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3] if vec else t[:, 0])
        waves = _wave_sum32(ss.view(4, 64))
        tot = torch.zeros(())
        for w in range(4):
            tot = tot + waves[w]
        out.append(tot)
    if wrong == "block_twice" and len(ranges) == 1:
        out[0] = out[0] * 2
    return torch.stack(out)


def partials_check(got, x, rows, cols, vec, what):
    """got fp32 [blocks] of one matrix against the float64 sums of squares of the kernel's own X (bf16 [rows, cols]) over each block's
    range, and their sum against the float64 total.  All terms are non-negative, so every rounding is at most u times the final sum:
    partials_depth(per) u sum.  (Same-sign terms with random roundings err like sqrt(depth) u: random data sits near a tenth of this.)
    Returns (worst block err / bound, total err / bound)."""
    assert tuple(got.shape) == (n_partials(rows, cols),), (what, got.shape)
    x2 = x.double().reshape(-1).square()
    per, ranges = partition(rows, cols, vec)
    ref = torch.stack([x2[b:e].sum() for b, e in ranges])
    rel = partials_depth(per, vec) * U * SECOND
    r_blk = check(got, ref, rel * ref, f"{what}: partials")
    r_tot = check(got.double().sum().reshape(1), x2.sum().reshape(1), rel * x2.sum().reshape(1), f"{what}: sum of partials")
    return r_blk, r_tot


# ================================================================================================ normalise
def normalize_f32_path(x_img, partials, eps=NS_EPS, wrong=None):
    """x_img bf16 [n, rp, cp], partials fp32 [n, blocks] -> bf16 [n, rp, cp]: total = the partials added in ascending order in fp32,
    norm = bf16(sqrt32(total)), denom = bf16(norm + eps), X' = bf16(X / denom) with an fp32 division.  wrong: 'norm_fp32' (the norm
    stays an fp32 scalar: denom = sqrt32(total) + eps, unrounded), 'no_eps' (denom = norm), 'quotient_f64' (the quotient taken in
    float64 and rounded once to bf16)."""
    e = f32(eps)
    out = torch.empty_like(x_img)
    for i in range(x_img.shape[0]):
        total = torch.zeros(())
        for j in range(partials.shape[1]):
            total = total + partials[i, j]
        root = torch.sqrt(total)
        norm = root.to(torch.bfloat16).float()
        if wrong == "norm_fp32":
            denom = root + e
        elif wrong == "no_eps":
            denom = norm
        else:
            denom = (norm + e).to(torch.bfloat16).float()
        if wrong == "quotient_f64":
            out[i] = rne64_bf16(x_img[i].double() / denom.double())
        else:
            out[i] = (x_img[i].float() / denom).to(torch.bfloat16)
    return out


def normalize_check(got_img, x_img, partials, what, eps=NS_EPS):
    """Bit for bit over the whole padded image, from the kernel's own X and partials: every step is one correctly rounded IEEE
    operation or an RNE conversion."""
    bits_equal(got_img, normalize_f32_path(x_img, partials, eps), f"{what}: normalised X")


# ================================================================================================ apply
def shape_scale(rows, cols):
    """ref:utils/muon_utils.py:175 as cm3p_amd.muon passes it."""
    return max(1, rows / cols) ** 0.5


def _gather(x_img, rows, cols, ldx):
    """What a kernel reading element (r, c) at x[r ldx + c] sees of one padded image."""
    idx = torch.arange(rows)[:, None] * ldx + torch.arange(cols)[None, :]
    return x_img.reshape(-1)[idx]


def apply_f32_path(p, x_img, rows, cols, neg_lr, wrong=None):
    """p fp32 [n, rows, cols], x_img bf16 [n, rp, cp] -> p' = fma(neg_lr, o, p), o = bf16(fl32(float(X) shape_scale)).  wrong: 'no_bf16'
    (o = fl32(X scale)), 'ldx_cols' (rows read at a pitch of cols), 'padded_scale' (shape_scale of the padded extents),
    'two_roundings' (fl32(fl32(neg_lr o) + p))."""
    rp, cp = x_img.shape[1:]
    s = f32(shape_scale(rp, cp) if wrong == "padded_scale" else shape_scale(rows, cols))
    lr = f32(neg_lr)
    x = torch.stack([_gather(xi, rows, cols, cols if wrong == "ldx_cols" else cp) for xi in x_img]).float()
    o = x * s
    if wrong != "no_bf16":
        o = o.to(torch.bfloat16).float()
    return lr * o + p if wrong == "two_roundings" else fma32(lr, o, p)


def apply_check(got_p, p, x_img, rows, cols, neg_lr, what):
    """o in float64: float(X) scale is exact there (8 + 24 bits), rounded to fp32 and then to bf16 as the kernel does.  p' against the
    float64 neg_lr o + p (the product exact, 24 + 8 bits): the fma is ONE rounding of that value, half an fp32 ulp; 2^-52 |ref| on
    top is the float64 sum's own rounding."""
    s, lr = float(f32(shape_scale(rows, cols))), float(f32(neg_lr))
    x = x_img[:, :rows, :cols].double()
    o = (x * s).float().to(torch.bfloat16).double()
    ref = lr * o + p.double()
    return check(got_p, ref, half_ulp_f32(ref) + 2.0 ** -52 * ref.abs(), f"{what}: p'")


# ================================================================================================ AdamW rule
def adamw_stride(max_numel):
    """Elements one grid-stride pass of adamw_multi_kernel covers: 256 threads times min(64, ceil(max_numel / 1024)) blocks."""
    return 256 * min(64, -(-max_numel // 1024))


def _lerp32(a, b, w, contract, d=None):
    """lerp_like_torch.  contract: the multiply-adds the compiler may fuse, fused (b - d (1 - w) as fma(-d, 1 - w, b)).  d: the
    difference b - a where the caller has it from a fused product-difference."""
    d = b - a if d is None else d
    if abs(float(w)) < 0.5:
        return fma32(w, d, a)
    one_minus = 1.0 - w
    return fma32(-d, one_minus, b) if contract else b - d * one_minus


def adamw_f32_path(p, g, m1, m2, w1, w2, eps, decay, step_alpha, wrong=None, contract=False, max_numel=None):
    """adamw_multi_kernel on one tensor -> (p', m1', m2').  wrong: 'decay_after' ((p + alpha u) decay), 'eps_inside' (sqrt(m2' + eps)),
    'pass_skipped' (a tensor above 65536 elements keeps the elements of its last grid-stride pass as they were)."""
    w1, w2, eps, decay, alpha = f32(w1), f32(w2), f32(eps), f32(decay), f32(step_alpha)
    a = _lerp32(m1, g, w1, contract)
    b = _lerp32(m2, g * g, w2, contract, d=fma32(g, g, -m2) if contract else None)  # (fused: g^2 - m2 from the exact square)
    if wrong == "eps_inside":
        u = a / torch.sqrt(b + eps)
    else:
        u = a / (eps + torch.sqrt(b))
    if wrong == "decay_after":
        pn = (p + alpha * u) * decay
    else:
        pn = fma32(alpha, u, p * decay)
    if wrong == "pass_skipped" and p.numel() > 65536:
        stride = adamw_stride(max_numel)
        first = (p.numel() - 1) // stride * stride
        pn[first:], a[first:], b[first:] = p[first:], m1[first:], m2[first:]
    return pn, a, b


def adamw_check(got_p, got_m1, got_m2, p, g, m1, m2, w1, w2, eps, decay, step_alpha, what):
    """Float64 m' = m + w (b - m) (both branches of torch.lerp mean this), b = g for m1 and g^2 for m2, from the inputs; p' from the
    kernel's own m1', m2'.  With d = b - m:
      |w| < 1/2, fma(w, d, m):  d rounds once (u |d|, weighted w) and the fma once: w u |d| + u |m'|.
      otherwise, b - d (1 - w): d, 1 - w and their product round once each, the difference once: 3 u (1 - w) |d| + u |m'|
                                (a fused product-difference drops one of the three).
      m2 only: b = fl32(g^2) adds u g^2 with weight w where d is taken from the same rounded square (b - (b - m)(1 - w)).  The
               compiler fuses d = fma(g, g, -m2) (the exact square, one rounding: the u |d| above); b itself, which the second
               branch subtracts from, stays the rounded square, and its error no longer cancels against d's: weight 1 there.
      p' = fma(alpha, u, fl32(p decay)), u = m1' / (eps + sqrt32(m2')): sqrt, sum and quotient round once each (3 u |u|), the product
           p decay once, the fma once: 3 u |alpha u| + u |p decay| + u |p'|.
    All far inside the fixture test's rtol 2e-6 / atol 1e-7 (the host test asserts it).  Returns the three err / bound."""
    w1d, w2d, epsd, decd, ald = (float(f32(v)) for v in (w1, w2, eps, decay, step_alpha))

    def lerp64(m, b, w):
        d = b - m
        ref = m + w * d
        k = w * d.abs() if abs(w) < 0.5 else 3 * (1 - w) * d.abs()
        return ref, k

    g64, m1_64, m2_64 = g.double(), m1.double(), m2.double()
    r1, k1 = lerp64(m1_64, g64, w1d)
    r2, k2 = lerp64(m2_64, g64 * g64, w2d)
    b1 = U * (k1 + r1.abs()) * SECOND + FTZ
    b2 = U * (k2 + (w2d if abs(w2d) < 0.5 else 1.0) * g64 * g64 + r2.abs()) * SECOND + FTZ
    u = got_m1.double() / (epsd + got_m2.double().sqrt())
    rp = ald * u + p.double() * decd
    bp = U * (3 * (ald * u).abs() + (p.double() * decd).abs() + rp.abs()) * SECOND + FTZ
    return (check(got_p, rp, bp, f"{what}: p'"), check(got_m1, r1, b1, f"{what}: m1'"), check(got_m2, r2, b2, f"{what}: m2'"),
            dict(p=(rp, bp), m1=(r1, b1), m2=(r2, b2)))


# ================================================================================================ one Newton-Schulz iteration
def ns_gemm_calls(rows, cols):
    """newton_schulz_batched's three calls restated as (M, N, K, lda, ldb, a_kc, b_kc) for cm3p_gemm_route."""
    rp, cp = up8(rows), up8(cols)
    s = min(rp, cp)
    if rp > cp:  # tall: A = X^T X, X' = a X + X B
        return [(s, s, rp, cp, cp, 0, 0), (s, s, s, s, s, 1, 1), (rp, cp, s, cp, s, 1, 1)]
    return [(s, s, cp, cp, cp, 1, 1), (s, s, s, s, s, 1, 1), (rp, cp, s, s, cp, 1, 0)]


def _mm_nt(a, b):
    """a [n, M, K], b [n, N, K] -> a b^T per matrix."""
    return torch.einsum("bmk,bnk->bmn", a, b)


def ns_f32_path(x_img, wrong=None, resid_other=None):
    """One iteration on bf16 [n, rp, cp] -> (A, B, X') bf16: fp32 matmuls, alpha acc + beta R in fp32, one bf16 rounding per GEMM.
    A = X X^T (X^T X for rp > cp), B = bf16(b A + c (A A^T)), X' = bf16(a X + B X) (a X + X B^T).
    wrong: 'ca_rounded' (c A rounded to bf16 before the product, as a chain of bf16 tensor ops would), 'x_from_a' (the last GEMM
    multiplies by A, not B), 'resid_other_buffer' (its residual read from the other workspace image, `resid_other`),
    'tall_on_wide' (the tall argument list on a wide weight: the top-left s x s of X^T X)."""
    x = x_img.float()
    rp, cp = x.shape[1:]
    s = min(rp, cp)
    tall = rp > cp
    rnd = lambda t: t.to(torch.bfloat16)  # noqa: E731
    a_, b_, c_ = f32(NS_A), f32(NS_B), f32(NS_C)
    if wrong == "tall_on_wide":
        assert not tall
        A = rnd(_mm_nt(x[:, :, :s].transpose(1, 2), x[:, :, :s].transpose(1, 2)))
    else:
        A = rnd(_mm_nt(x.transpose(1, 2), x.transpose(1, 2)) if tall else _mm_nt(x, x))
    Af = A.float()
    if wrong == "ca_rounded":
        B = rnd(rnd(c_ * Af).float() @ Af.transpose(1, 2) + b_ * Af)
    else:
        B = rnd(c_ * _mm_nt(Af, Af) + b_ * Af)
    Mf = Af if wrong == "x_from_a" else B.float()
    r = resid_other.float() if wrong == "resid_other_buffer" else x
    Xn = rnd((_mm_nt(x, Mf) if tall else Mf @ x) + a_ * r)
    return A, B, Xn


def _axpby_check(got, a, b, alpha, r, beta, what):
    """got bf16 against float64 alpha (a b^T) + beta r of the bf16 operands.  fp32 side: the accumulator is within gemm_refs'
    random_bound of the float64 product (K u sum |a||b|, doubled for truncating adds inside the MFMA); alpha acc rounds once, beta r
    once (not at all when fused), their sum once - 2 u (|alpha acc| + |beta r|) covers the three; then one bf16 rounding."""
    al, be = float(f32(alpha)), float(f32(beta))
    n = a.shape[0]
    acc = _mm_nt(a.double(), b.double())
    accb = torch.stack([G.random_bound(a[i], b[i]) for i in range(n)])
    ref = al * acc
    mag = ref.abs()
    if r is not None:
        ref = ref + be * r.double()
        mag = mag + (be * r.double()).abs()
    e32 = abs(al) * accb + 2 * U * mag * SECOND + FTZ
    return check(got.float(), ref, bf16_bound(ref, e32), what)


def ns_check(got_a, got_b, got_x, x_img, what):
    """Each GEMM from the kernel's own previous output: A from X, B from the kernel's A, X' from the kernel's B and X, as the three
    argument lists of newton_schulz_batched spell them (A A^T and X B^T: the k-contiguous forms; A and B are symmetric).
    Returns the three err / bound."""
    rp, cp = x_img.shape[1:]
    s = min(rp, cp)
    tall = rp > cp
    assert tuple(got_a.shape[1:]) == (s, s) and tuple(got_b.shape[1:]) == (s, s) and tuple(got_x.shape[1:]) == (rp, cp), what
    xt = x_img.transpose(1, 2)
    ra = _axpby_check(got_a, xt, xt, 1.0, None, 0.0, f"{what}: A") if tall else _axpby_check(got_a, x_img, x_img, 1.0, None, 0.0, f"{what}: A")
    rb = _axpby_check(got_b, got_a, got_a, NS_C, got_a, NS_B, f"{what}: B")
    if tall:
        rx = _axpby_check(got_x, x_img, got_b, 1.0, x_img, NS_A, f"{what}: X'")
    else:
        rx = _axpby_check(got_x, got_b, xt, 1.0, x_img, NS_A, f"{what}: X'")
    return ra, rb, rx


def padding_is_zero(img, rows, cols):
    """Every element of bf16 [n, rp, cp] outside rows x cols is +0 (bit pattern 0)."""
    bits = img.contiguous().view(torch.int16).clone()
    bits[:, :rows, :cols] = 0
    return not bool(bits.any())
