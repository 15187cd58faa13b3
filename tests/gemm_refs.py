"""Data generators, float64 references, bounds and the case table of the three bf16 GEMM kernels (gemm_bf16_kernel of csrc/gemm.hip,
gemm256_kernel of csrc/gemm256.hip, gemm8p_kernel - "the ring" - of csrc/gemm8p.hip), shared by tests/test_gemm_kernels_gpu.py (the
kernels against them) and tests/test_gemm_refs_host.py (a torch fp32 restatement of the kernels' arithmetic that must pass, and wrong
evaluations that must fail).  No GPU and no cm3p_amd import here.

Exact data.  Operands are m 2^e with integer |m| <= mmax and one exponent e per row of A and per row of B (a row = one output row or
column, whatever the storage layout).  With mmax^2 K < 2^24 every product and every partial sum of a dot product, in any order and
any grouping (MFMA blocks, k-tiles, split-K partials and their ordered reduce), is an integer below 2^24 times 2^(e_a + e_b): an
fp32 number.  The fp32 accumulator is therefore EXACT and the float64 matmul is its reference at tolerance 0, with all eight
significand bits of bf16 and its exponent in play.  What follows the accumulator is stated per epilogue (epilogue_refs) in the
roundings the kernels document; everything that is a single IEEE operation is asserted bit for bit.

u = 2^-24, SECOND = 1 + 1e-3, bf16_bound and half_ulp_bf16 are those of tests/row_kernel_refs.py.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

import row_kernel_refs as R
from row_kernel_refs import FTZ, SECOND, U, bf16_bound

EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_ROPE, EPI_F32_BIAS, EPI_GEGLU, EPI_BF16_RESID = 0, 1, 2, 3, 5, 6, 7  # include/cm3p_hip.h
PLAIN_EPILOGUES = (EPI_F32, EPI_BF16, EPI_F32_RESID, EPI_F32_BIAS, EPI_BF16_RESID)
SMALL, G256, RING = "gemm_bf16_kernel", "gemm256_kernel", "gemm8p_kernel"
EXPS = (-3, -2, -1, 0, 1, 2, 3)
SOFTMAX_Q_SCALE = 64 ** -0.5 * 1.4426950408889634  # cm3p_amd.kernels.SOFTMAX_Q_SCALE restated (the GPU test compares the two)


# ================================================================================================ data
def mmax_for(K):
    """The widest significand for which mmax^2 K < 2^24: 255 (K <= 256), 127 (K <= 1040), 31 (K <= 17457)."""
    for mmax in (255, 127, 31):
        if mmax * mmax * K < 2 ** 24:
            return mmax
    raise ValueError(f"K = {K}: no exact data")


def exact_operand(rows, K, g, mmax=None, exps=EXPS, parts=False):
    """[rows, K] fp32 holding bf16 values m 2^e(row), |m| <= mmax uniform.  parts: -> (x, m, e)."""
    mmax = mmax_for(K) if mmax is None else mmax
    m = torch.randint(-mmax, mmax + 1, (rows, K), generator=g)
    e = torch.tensor(exps, dtype=torch.int32)[torch.randint(0, len(exps), (rows,), generator=g)]
    x = torch.ldexp(m.float(), e[:, None])
    return (x, m, e) if parts else x


def small_int_operand(rows, K, g):
    """The data of the older exact tests (tests/test_kernels_gpu.py): integers in [-4, 4], three significand bits."""
    return torch.randint(-4, 5, (rows, K), generator=g).float()


def geglu_exps(K):
    """Row exponents (A's, B's) that put h = x Wi^T of exact_operand data at a standard deviation between 1 and 2 for the rows with
    the largest exponents and down to an eighth of that for the others - inside [-6, 6] (three standard deviations) and on GELU's
    slope, not in its flat tails: a uniform integer in [-m, m] has variance m (m + 1) / 3, a dot product of K such products
    var^2 K."""
    mmax = mmax_for(K)
    shift = math.ceil(math.log2(mmax * (mmax + 1) / 3 * math.sqrt(K) / 2))
    ea, eb = -(shift // 2), -(shift - shift // 2)
    return (ea - 2, ea - 1, ea), (eb - 1, eb)


def random_operand(rows, K, g):
    """bf16 normal data as fp32."""
    return torch.randn(rows, K, generator=g).to(torch.bfloat16).float()


def stored(x, kc):
    """The storage form of a logical [idx, K] operand: k-contiguous [idx, K] or k-strided [K, idx]."""
    return x.contiguous() if kc else x.t().contiguous()


def rne_bf16(x):
    """Round-to-nearest-even to bf16 of an fp32 / float64 tensor holding fp32 values, returned in the input's dtype."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def trunc_bf16(x):
    """The wrong rounding: the low 16 bits of the fp32 pattern dropped."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


def clear_low_bits(x, nbits=4):
    """bf16 values with the low nbits of the 7 stored significand bits cleared (what damaged staging or fragment code would feed)."""
    return (x.float().contiguous().view(torch.int32) & ~((1 << (16 + nbits)) - 1)).view(torch.float32)


# ================================================================================================ accumulator and plain epilogues
def acc64(a, b):
    """a [M, K], b [N, K] (bf16 values) -> the float64 matmul a b^T: THE reference of the accumulator."""
    return a.double() @ b.double().t()


def epilogue_refs(acc, r32=None, r16=None, bias=None):
    """acc: the exact accumulator as float64 (every value an fp32 number).  -> {epilogue: expected output, exact bits}.
      EPI_F32        fp32(acc)
      EPI_BF16       RNE_bf16(acc)
      EPI_F32_RESID  the single fp32 add fp32(acc) + r            EPI_F32_BIAS  fp32(acc) + bias[n]
      EPI_BF16_RESID bf16(float(bf16(acc)) + float(r)): the projection is rounded, then the sum is rounded once more
    torch's CPU elementwise ops are single IEEE operations and its fp32 -> bf16 conversion is RNE."""
    a32 = acc.float()
    assert torch.equal(a32.double(), acc), "the accumulator is not an fp32 number: the data is not exact"
    out = {EPI_F32: a32, EPI_BF16: a32.to(torch.bfloat16)}
    if r32 is not None:
        out[EPI_F32_RESID] = a32 + r32
    if bias is not None:
        out[EPI_F32_BIAS] = a32 + bias[None, :]
    if r16 is not None:
        out[EPI_BF16_RESID] = (a32.to(torch.bfloat16).float() + r16.float()).to(torch.bfloat16)
    return out


def residuals(M, N, acc, g):
    """Residuals at the accumulator's own magnitude, so that either order of add and rounding moves the result: fp32 r (random
    significands), bf16 r, and an fp32 bias per column."""
    s = acc.abs().mean().item()
    r32 = (torch.randn(M, N, generator=g) * s).float()
    r16 = (torch.randn(M, N, generator=g) * s).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g) * s).float()
    return r32, r16, bias


def gemm_f32_path(a, b, epi, r=None, wrong=None, kchunk=None):
    """The kernels' arithmetic in torch fp32: an fp32 matmul (any order: exact on this data) and the epilogue's roundings.
    wrong: 'drop_chunk' (an 8-wide k chunk of A is not accumulated), 'swap_chunks' (two 16-byte chunks of A's rows change
    places), 'clear_bits' (A's low 4 significand bits cleared), 'trunc' (bf16 output truncated), 'resid_first' (the residual added
    before the bf16 rounding), 'skip_last_split' (the k range past the last full kchunk is not accumulated)."""
    a, b = a.float().clone(), b.float()
    K = a.shape[1]
    if wrong == "drop_chunk":
        a[:, 8 * (K // 16):8 * (K // 16) + 8] = 0
    elif wrong == "swap_chunks":
        a[:, :16] = torch.cat([a[:, 8:16], a[:, :8]], 1)
    elif wrong == "clear_bits":
        a = clear_low_bits(a)
    elif wrong == "skip_last_split":
        a[:, (K - 1) // kchunk * kchunk:] = 0
    acc = a @ b.t()
    rnd = trunc_bf16 if wrong == "trunc" else rne_bf16
    if epi == EPI_F32:
        return acc
    if epi == EPI_BF16:
        return rnd(acc).to(torch.bfloat16)
    if epi == EPI_F32_RESID:
        return acc + r
    if epi == EPI_F32_BIAS:
        return acc + r[None, :]
    if epi == EPI_BF16_RESID:
        if wrong == "resid_first":
            return (acc + r.float()).to(torch.bfloat16)
        return rnd(rnd(acc) + r.float()).to(torch.bfloat16)
    raise ValueError(epi)


# ================================================================================================ random data
def random_bound(a, b):
    """Per-element bound of an fp32-accumulated dot product of exact bf16 x bf16 products (8 + 8 significand bits: an fp32 number):
    K u sum_k |a_k b_k| bounds any-order fp32 summation of K exact terms (K - 1 roundings on the longest path, each at most u times
    a partial sum of absolute values); the factor 2 covers adds inside the MFMA that truncate rather than round (a truncation moves a
    value by up to one ulp = 2u relative, not u), its internal order and rounding not being documented.  Derived, not measured."""
    K = a.shape[1]
    return 2 * K * U * (a.double().abs() @ b.double().abs().t()) * SECOND


# ================================================================================================ RoPE epilogue
def rope_ref(acc, cos, sin, S, per_batch, q_scale, nh, small):
    """acc [T, 3 nh 64] float64 (exact accumulator), cos / sin [rows, 32] float64 holding cm3p_rope_table's own fp32 output
    (rows = T for per_batch, else S: row m uses table row m % S) -> (ref, bound) of the whole [T, 3 nh 64] output.

    The two specifications (head dims d < 32 pair with d + 32; a = y[d], b = y[d + 32], qs = fp32(q_scale) on the q third, 1 on k):
      256 x 256 kernels (small=False): y = RNE_bf16(acc) - the projection is rounded first, as the unfused GEMM + cm3p_rope_apply
          chain and the reference model's autocast path do - out = RNE_bf16(qs (a c - b s)), partner RNE_bf16(qs (b c + a s)).
      128 x 128 kernel (small=True): y = acc, the fp32 accumulator is rotated, multiplied by qs and rounded once.
    Bound: the fp32 evaluation of qs (a c -+ b s) rounds the two products (u |a c| + u |b s|), their sum (u of at most
    |a c| + |b s|) and the product with qs (the same): e32 = 3 u (|a c| + |b s|) qs, and with a fused multiply-add one product
    rounding falls away, so the count holds either way; then one bf16 rounding: bf16_bound(ref, e32).  The v third is RNE_bf16(acc)
    exactly (bound 0)."""
    T = acc.shape[0]
    qs32 = float(torch.tensor(q_scale, dtype=torch.float32))
    v = acc.view(T, 3, nh, 64)
    y = v if small else rne_bf16(v)
    prow = torch.arange(T) if per_batch else torch.arange(T) % S
    c, s = cos[prow][:, None, None, :], sin[prow][:, None, None, :]
    a, b = y[:, :2, :, :32], y[:, :2, :, 32:]
    qs = torch.tensor([qs32, 1.0], dtype=torch.float64)[None, :, None, None]
    ra, rb = qs * (a * c - b * s), qs * (b * c + a * s)
    ea = 3 * U * ((a * c).abs() + (b * s).abs()) * qs * SECOND + FTZ
    eb = 3 * U * ((b * c).abs() + (a * s).abs()) * qs * SECOND + FTZ
    ref = torch.cat([torch.cat([ra, rb], -1), rne_bf16(v[:, 2:])], 1)
    bound = torch.cat([torch.cat([bf16_bound(ra, ea), bf16_bound(rb, eb)], -1), torch.zeros_like(v[:, 2:])], 1)
    return ref.reshape(T, -1), bound.reshape(T, -1)


def rope_f32_path(acc32, cos32, sin32, S, per_batch, q_scale, nh, small, fma=False, wrong=None):
    """The epilogue in torch fp32 (elementwise IEEE operations).  fma: a c -+ b s evaluated as fma(a, c, -+ fl(b s)) - the product
    a c (24 + 24 bits) and its sum with an fp32 number are formed in float64 and rounded to fp32.  wrong: 'wrong_side' (the other
    kernel's side of the bf16 rounding), 'wrong_modulus' (table row m % (S + 1))."""
    T = acc32.shape[0]
    if wrong == "wrong_side":
        small = not small
    qs = torch.tensor([float(torch.tensor(q_scale, dtype=torch.float32)), 1.0], dtype=torch.float32)[None, :, None, None]
    v = acc32.float().view(T, 3, nh, 64)
    y = v if small else rne_bf16(v)
    if per_batch:
        prow = torch.arange(T)
    else:
        prow = torch.arange(T) % (S + 1 if wrong == "wrong_modulus" else S) % S
    c, s = cos32.float()[prow][:, None, None, :], sin32.float()[prow][:, None, None, :]
    a, b = y[:, :2, :, :32], y[:, :2, :, 32:]
    if fma:
        ra = (a.double() * c.double() - (b * s).double()).float()
        rb = (b.double() * c.double() + (a * s).double()).float()
    else:
        ra, rb = a * c - b * s, b * c + a * s
    out = torch.cat([torch.cat([qs * ra, qs * rb], -1), v[:, 2:]], 1)
    return out.to(torch.bfloat16).reshape(T, -1)


def rope_positions(S, B, per_batch):
    """Shared positions 0 .. S - 1, or one row of positions per sequence with a distinct offset and stride."""
    if not per_batch:
        return torch.arange(S).unsqueeze(0)
    return torch.stack([torch.arange(S) * (1 + b % 3) + 7 * b for b in range(B)])


# ================================================================================================ GeGLU epilogue
def geglu_interleave_index(I):
    """cm3p_amd.kernels.geglu_interleave_index restated: row 64 q + r of the interleaved Wi copy is Wi row 32 q + r (r < 32) or
    I + 32 q + r - 32."""
    n = torch.arange(2 * I)
    r = n % 64
    j = (n // 64) * 32 + r % 32
    return torch.where(r < 32, j, I + j)


def geglu_ref(acc):
    """acc [T, 2 I] float64 = x Wi^T (Wi in its natural row order) -> (ref, bound): R.geglu_fwd_ref of the RNE_bf16(acc) rows."""
    return R.geglu_fwd_ref(rne_bf16(acc))


# ================================================================================================ which kernel
def kchunk_of(K, split_k):
    """cm3p_gemm_bf16's k-split length and the split count it recomputes."""
    if split_k <= 1:
        return K, 1
    q = 128 if K % 128 == 0 else 64
    kchunk = -(-(-(-K // split_k)) // q) * q
    return kchunk, -(-K // kchunk)


@dataclass(frozen=True)
class Case:
    """One GEMM shape.  kernel / rebal: where it lands by default, stated here by hand from the routing rule (csrc/gemm.hip
    cm3p_gemm_route_of) and compared on the host with the rule restated below (restated_kernel) and with the library's own answer
    (cm3p_gemm_route, which the entry points launch from), and again on the GPU before every launch - three statements of one rule,
    the third being the one that runs."""
    name: str
    M: int
    N: int
    K: int
    a_kc: bool = True
    b_kc: bool = True
    split_k: int = 1
    kernel: str = RING
    rebal: Optional[bool] = None

    def tag(self, epi, impl=None):
        """The profiler tag under CM3P_GEMM_IMPL = impl (None, '256', '128')."""
        b2s = lambda v: "true" if v else "false"  # noqa: E731
        kernel = self.kernel
        if impl == "128" or kernel == SMALL:
            kernel = SMALL
        elif impl == "256":
            kernel = G256
        tail = f", {b2s(self.rebal)}" if kernel == RING else ""
        return f"{kernel}<{b2s(self.a_kc)}, {b2s(self.b_kc)}, {epi}{tail}>"

    def epilogues(self):
        """The plain epilogues cm3p_gemm_bf16 accepts for this shape and layout."""
        out = [EPI_F32, EPI_BF16, EPI_F32_RESID]
        if self.a_kc and self.b_kc:
            out.append(EPI_F32_BIAS)
        if self.N % 8 == 0:
            out.append(EPI_BF16_RESID)
        return out if self.split_k == 1 else [EPI_F32]


def restated_kernel(c):
    """(kernel, rebal) by the library's rule, restated: big when K and the k-split are multiples of 64 and there are 200 work items
    of 256 x 256; the ring unless M or N is no multiple of 8; REBAL when every item has an even number of k-tiles."""
    kchunk, splits = kchunk_of(c.K, c.split_k)
    big = c.K % 64 == 0 and kchunk % 64 == 0 and -(-c.M // 256) * -(-c.N // 256) * splits >= 200
    if not big:
        return SMALL, None
    if c.M % 8 or c.N % 8:
        return G256, None
    last = c.K - (splits - 1) * kchunk
    return RING, (kchunk // 64) % 2 == 0 and (last // 64) % 2 == 0


def _ring(name, M, N, K, a_kc=True, b_kc=True, split_k=1):
    kchunk, splits = kchunk_of(K, split_k)
    last = K - (splits - 1) * kchunk
    return Case(name, M, N, K, a_kc, b_kc, split_k, RING, (kchunk // 64) % 2 == 0 and (last // 64) % 2 == 0)


# Forward (1, 1), 200 tiles of one column: 1 to 5 k-tiles, the plain instance (odd) and REBAL (even) alternating.
FORWARD = [Case(f"fwd_k{K}", 51200, 256, K, rebal=(K // 64) % 2 == 0) for K in (64, 128, 192, 256, 320)]

# Forward edges at one and three k-tiles (both the plain instance).
EDGE_K = (64, 192)
EDGES = []
for _K in EDGE_K:
    EDGES += [Case(f"edge_m{r}_k{_K}", 51200 + r, 256, _K, rebal=False) for r in (8, 64, 136, 248)]
    EDGES += [Case(f"edge_n{N}_k{_K}", M, N, _K, rebal=False) for N, M in ((8, 51200), (72, 51200), (248, 51200), (264, 25600), (520, 17152))]
    EDGES += [Case(f"edge_mn_k{_K}", 25736, 328, _K, rebal=False),
              Case(f"edge_mod4_k{_K}", 51204, 252, _K, kernel=G256)]  # M % 8 = N % 8 = 4: the ring refuses it

# dgrad (1, 0): B k-strided with an 8- and a 72-column remainder, a ragged last row tile.
DGRAD = [Case(f"dgrad_n{N}_k{_K}", 25608, N, _K, True, False, rebal=False) for N in (264, 328) for _K in (64, 192)]
# (0, 1): A k-strided, a 72-row remainder under it and an 8-column remainder of the k-contiguous B.
KS_A = [Case("ksa_k192", 25672, 264, 192, False, True, rebal=False), Case("ksa_k128", 25672, 264, 128, False, True, rebal=True)]

# wgrad (0, 0) on 2 x 3 ragged tiles, 34 splits:
WGRAD = [
    _ring("wgrad_equal_even", 264, 520, 34 * 128, False, False, 34),        # kchunk 128: every item 2 k-tiles -> REBAL
    _ring("wgrad_short_even", 264, 520, 33 * 256 + 128, False, False, 34),  # kchunk 256 (4 k-tiles), the last split 2 -> REBAL
    _ring("wgrad_short_odd", 264, 520, 33 * 128 + 64, False, False, 34),    # K % 128 = 64: kchunk 128 (2), the last split 1 -> plain
]
# linear_wgrad with the library's own split count: dy [8256, 1032], x [8256, 2312] -> 5 x 10 tiles x 4 splits of 33 k-tiles, the
# last one 30 (cm3p_gemm_wgrad_splits: min(256 / 50, 8256 / 2048) = 4; 8256 = 8192 + 64 is no multiple of 2048).  At 4 splits the
# 200-item threshold needs 50 tiles, so no smaller shape reaches the big kernels this way: a 39 GFLOP reference, well above the
# 10 GFLOP of every other case here (the GPU test takes the device's float64 matmul for it)
LINEAR_WGRAD = _ring("linear_wgrad", 1032, 2312, 8256, False, False, 4)

# The 128 x 128 kernel natively: the edges of the older tests with the new data, every layout, split-K with a k tail.
SMALL_CASES = [
    Case("small_200_72_96", 200, 72, 96, kernel=SMALL), Case("small_130_8_8", 130, 8, 8, kernel=SMALL),
    Case("small_300_140_64_mod4", 300, 140, 64, kernel=SMALL),
    Case("small_dgrad", 200, 72, 96, True, False, kernel=SMALL), Case("small_ksa", 200, 72, 96, False, True, kernel=SMALL),
    Case("small_wgrad", 200, 72, 96, False, False, kernel=SMALL),
    Case("small_splitk_tail", 200, 72, 1000, True, True, 3, kernel=SMALL),  # kchunk 384, the last split 232 = 3 x 64 + 40
    Case("small_wgrad_splitk_tail", 72, 136, 777, False, False, 3, kernel=SMALL),
]

# Pitched forms (lda = K + 8, ldb = K + 16, ldc = N + 8), both extents ragged: 201 x 1 tiles.
PITCHED = [Case(f"pitched_k{_K}", 51208, 248, _K, rebal=False) for _K in EDGE_K]

# Random data, K = 768: 68 x 3 tiles, both extents ragged (and multiples of 8 for the k-strided layouts).
RANDOM = [Case(f"random_{int(a)}{int(b)}", 17160, 520, 768, a, b, rebal=True) for a in (True, False) for b in (True, False)]

# RoPE: nh = 2 (N = 384, the rotated 256 columns end on a tile boundary), K = 64.  (S, B): S < 256 (the modulo branch), S = 300
# (a sequence end inside tiles, the one-subtraction branch, and a ragged last row tile: 25800 = 100 x 256 + 200), S = 512.
ROPE_NH = 2
ROPE_BIG = [(200, 128), (300, 86), (512, 50)]
ROPE_SMALL = [(200, 3), (300, 3), (512, 2)]  # the same sequence lengths below the 200-tile threshold


def rope_case(S, B):
    T = S * B
    big = -(-T // 256) * 2 >= 200
    return Case(f"rope_s{S}_b{B}", T, 3 * ROPE_NH * 64, 64, kernel=RING if big else SMALL, rebal=False if big else None)


# GeGLU (T, I, K): 200 x 1, 201 x 1 (a ragged row tile and 64 dead columns) and 200 x 4 tiles.
GEGLU = [(51200, 128, 64), (51208, 96, 192), (51200, 512, 128)]

ALL_CASES = FORWARD + EDGES + DGRAD + KS_A + WGRAD + [LINEAR_WGRAD] + SMALL_CASES + PITCHED + RANDOM + [rope_case(S, B) for S, B in ROPE_BIG + ROPE_SMALL]
