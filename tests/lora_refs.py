"""Float64 references and rounded restatements of the low-rank adapter kernels (csrc/lora.hip, include/cm3p_lora.h), shared by
tests/test_lora_kernels_gpu.py (the kernels against them) and tests/test_lora_refs_host.py (the restatements against them, and wrong
evaluations that must fail them).  No GPU and no cm3p_amd import here.

Merged cast.  R = W + s B A in float64 (W, A, B, s the fp32 values).  The kernel forms acc = sum_j B[n, j] A[j, k] as r fused
multiply-adds in fp32, d = fl(s acc), v = fl(W + d) and rounds v to bf16 once.  |v - R| <= err with
    err = SECOND u ((r + 1) |s| sum_j |B A| + |R|)        r roundings of the chain and one of the scaling; one of the add
so wherever bf16(R - err) and bf16(R + err) agree the kernel's bits are fixed; elsewhere R sits within err of a bf16 rounding boundary
and either neighbour is accepted (where W and s B A cancel to a value whose bf16 spacing is below err, every bf16 number between the two
roundings).  At most AMBIGUOUS_CAP of a matrix may take that branch.

Adapter gradients.  R: dB = s DY^T (X A^T), dA = s (DY B)^T X in float64 from the bf16 X, DY and the fp32 A, B.  E: the same with
a = bf16(A), b = bf16(B), u = bf16(fp32 X a^T), v = bf16(fp32 DY b), fp32 sums over the tokens, one fp32 multiplication by s.  The bound
is the node rule of tests/loss_head_refs.py: |got - R| <= M_NODE |E - R| in the Frobenius norm.
"""
import torch

from loss_head_refs import M_NODE, node_check, rel_l2  # noqa: F401  (re-exported to the two test files)
from row_kernel_refs import SECOND, U, bits_equal  # noqa: F401

AMBIGUOUS_CAP = 0.01
RANKS = (8, 16, 32, 64)


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def bf16_rne64(x):
    """float64 -> the nearest bf16 value (ties to even) as float64, rounding ONCE from the float64 (normal range)."""
    i = x.contiguous().view(torch.int64)
    i = (i + (((i >> 45) & 1) + ((1 << 44) - 1))) & ~((1 << 45) - 1)
    return i.view(torch.float64)


def bf16_bits(x64):
    """float64 values that are bf16 numbers -> their int16 bit patterns."""
    return x64.float().to(torch.bfloat16).view(torch.int16)


def interleave_index(I):
    """Row order of a Wi copy for the GeGLU store phases: out row 64 q + t <- row 32 q + t (t < 32), row I + 32 q + t - 32 otherwise."""
    q = torch.arange(2 * I) // 64
    t = torch.arange(2 * I) % 64
    return torch.where(t < 32, 32 * q + t, I + 32 * q + t - 32)


# ================================================================================================ merged cast
def merge_case(N, K, r, seed, zero_b=False):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * 0.05
    A = (torch.rand(r, K, generator=g) * 2 - 1) * K ** -0.5
    B = torch.zeros(N, r) if zero_b else torch.randn(N, r, generator=g) * 0.01
    return W, A, B


# (N, K, r, interleaved Wi): a partial tile in both directions; three row tiles; partial tiles with the largest r; the interleaved order
MERGE_SHAPES = ((24, 8, 8, False), (192, 64, 16, False), (200, 72, 64, False), (128, 64, 8, True))


def merge_single_cases():
    """[(W, A, B, s, interleave)]: one matrix per launch, s = alpha / r with alpha = 32."""
    return [(*merge_case(N, K, r, seed=100 + N), 32.0 / r, il) for N, K, r, il in MERGE_SHAPES]


def merge_table_cases():
    """One table that mixes the shapes above and a wide r = 32 matrix, each entry with a scale of its own."""
    return [(*merge_case(N, K, r, seed=200 + i), 0.5 + 0.25 * i, il) for i, (N, K, r, il) in enumerate(MERGE_SHAPES + ((64, 136, 32, False),))]


def merge_ref(W, A, B, s):
    """-> (R, err) float64 [N, K]."""
    sd = f32(s).double()
    R = W.double() + sd * (B.double() @ A.double())
    r = A.shape[0]
    err = SECOND * U * ((r + 1) * sd.abs() * (B.double().abs() @ A.double().abs()) + R.abs())
    return R, err


def merge_rounded(W, A, B, s, interleave=False, wrong=None):
    """E: -> (out, out_t) as float64 holding bf16 values; fp32 arithmetic, one rounding."""
    sv = f32(s)
    if wrong == "s_twice":
        sv = sv * sv
    v = W + sv * (B @ A)
    out = v.to(torch.bfloat16)
    out_t = out.t().contiguous()
    if interleave:
        out = out[interleave_index(W.shape[0] // 2)]
        if wrong == "interleave_on_transpose":
            out_t = out.t().contiguous()
    return out.double(), out_t.double()


def merge_check(out, out_t, W, A, B, s, interleave, what):
    """out [N, K], out_t [K, N]: tensors of bf16 VALUES (any dtype).  Exact bits where R is further than err from a rounding boundary,
    bf16(R - err) <= out <= bf16(R + err) elsewhere; -> the fraction of elements on the either-neighbour branch (asserted <= AMBIGUOUS_CAP)."""
    R, err = merge_ref(W, A, B, s)
    lo, hi = bf16_rne64(R - err), bf16_rne64(R + err)
    amb = lo != hi
    frac = float(amb.double().mean())
    assert frac <= AMBIGUOUS_CAP, f"{what}: {frac:.3%} of the reference is within the fp32 error of a bf16 boundary"
    lo_t, hi_t = lo.t(), hi.t()
    if interleave:
        idx = interleave_index(W.shape[0] // 2)
        lo, hi = lo[idx], hi[idx]
    for name, got, l, h in (("out", out, lo, hi), ("out_t", out_t, lo_t, hi_t)):
        got = got.detach().double().cpu()
        assert got.shape == l.shape, f"{what} {name}: shape {tuple(got.shape)} vs {tuple(l.shape)}"
        bad = (got < l) | (got > h) | (got != bf16_rne64(got))  # (NaN fails the last)
        assert not bool(bad.any()), f"{what} {name}: {int(bad.sum())} elements outside their candidates; first at {bad.nonzero()[0].tolist()}"
    return frac


# ================================================================================================ adapter gradients
def grad_case(T, K, N, r, seed, pitch_x=None):
    """-> X [T, K] bf16 (a view of a [T, pitch_x] buffer whose pad columns hold 3e38 when pitch_x is given), DY [T, N] bf16, A, B fp32."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(T, K, generator=g).to(torch.bfloat16)
    DY = (torch.randn(T, N, generator=g) * 0.1).to(torch.bfloat16)
    A = (torch.rand(r, K, generator=g) * 2 - 1) * K ** -0.5
    B = torch.randn(N, r, generator=g) * 0.05
    if pitch_x is not None:
        buf = torch.full((T, pitch_x), 3e38, dtype=torch.bfloat16)
        buf[:, :K] = X
        X = buf[:, :K]
    return X, DY, A, B


def grad_ref(X, DY, A, B, s):
    """R: -> dict(dA [r, K], dB [N, r]) float64."""
    Xd, Dd, Ad, Bd, sd = X.double(), DY.double(), A.double(), B.double(), f32(s).double()
    return dict(dA=sd * ((Dd @ Bd).t() @ Xd), dB=sd * (Dd.t() @ (Xd @ Ad.t())))


def grad_rounded(X, DY, A, B, s, wrong=None):
    """E: the roundings of cm3p_lora_grad in torch fp32 on the CPU.  wrong: an evaluation the bound must refuse."""
    Xf, Df, sv = X.float(), DY.float(), f32(s)
    a, b = A.to(torch.bfloat16).float(), B.to(torch.bfloat16).float()
    if wrong == "s_twice":
        sv = sv * sv
    if wrong == "last_row_dropped":
        Xf, Df = Xf[:-1], Df[:-1]
    u = (Xf @ (a if wrong == "a_for_a_t" else a.t())).to(torch.bfloat16).float()
    v = (Df @ b).to(torch.bfloat16).float()
    if wrong == "u_unrounded_swapped_with_v":
        u, v = Df @ b, Xf @ a.t()
    return dict(dA=(sv * (v.t() @ Xf)).double(), dB=(sv * (Df.t() @ u)).double())
