"""Kernel-level specifications of the audio front end (im2col / col2im / bias + GELU), the fp32 contrastive and classifier
head, the small element kernels, and LayerNorm past its grid, each against a float64 CPU reference of the same operation.

Conventions (as tests/test_kernels_gpu.py): bf16 inputs are rounded once and the same values go to both sides.  Every check is
per element, |got - ref| <= bound, where the bound is written next to it with its derivation; u = 2^-24 is the fp32 unit
roundoff.  A stage's reference is fed the kernel's own inputs to that stage (its bf16 patches, its z, its dz), so each bound
covers one stage.  Each check prints its largest err / bound (`pytest -rP` shows them).
"""
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24  # fp32 unit roundoff
CHUNK = 16384  # rows per float64 reference chunk (keeps the host copies of the 131072-row cases small)

torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def K():
    from cm3p_amd import kernels

    return kernels


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _check(got, ref, bound, what):
    """|got - ref| <= bound element-wise in float64; NaN / inf in `got` fail.  Returns the largest err / bound."""
    got = got.detach().double().cpu()
    ref = ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outside the bound; first at {idx}: got {got[idx].item():.9g} "
                             f"want {ref[idx].item():.9g} bound {bound[idx].item():.3g}")
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: max err/bound {ratio:.3g}")
    return ratio


def _bits_equal(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == torch.bfloat16:
        got, want = got.view(torch.int16), want.view(torch.int16)
    elif got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    bad = got != want
    if bad.any():
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ; first at {idx}")


def _misaligned(t):
    """The same values in a contiguous view that starts one element past a 16-byte boundary (the kernels' scalar paths)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------------------------------------ float64 restatements
def _phi_cdf(v):
    return 0.5 * torch.special.erfc(-v / math.sqrt(2.0))


def _gelu64(v):
    return v * _phi_cdf(v)


def _gelu_grad64(v):
    return _phi_cdf(v) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def _im2col_ref(x, token_major, stride):
    """F.pad + gather restatement: patch row (b, t), column c*3 + kk = input channel c at time t*stride + kk - 1, zero outside."""
    xc = x.permute(0, 2, 1) if token_major else x  # [B, C, T_in]
    B, C, _ = xc.shape
    p = F.pad(xc.float(), (1, 1)).unfold(2, 3, stride)  # [B, C, T_out, 3]
    return p.permute(0, 2, 1, 3).reshape(B * p.shape[2], C * 3)


def _col2im_ref(dp, B, C, T_in, T_out, stride):
    """fp32 sum of the contributions in the kernel's order kk = 0, 1, 2, rounded once to bf16."""
    d4 = dp.float().view(B, T_out, C, 3)
    s = torch.zeros(B, T_in, C)
    t = torch.arange(T_out)
    for kk in range(3):
        ti = t * stride + kk - 1
        ok = (ti >= 0) & (ti < T_in)
        c = torch.zeros(B, T_in, C)
        c[:, ti[ok]] = d4[:, ok, :, kk]
        s = s + c
    return s.to(torch.bfloat16)


def _contraction_c(k):
    """Per-element factor c of |got - ref| <= c * (|A| @ |B|) for an fp32-accumulated contraction over k.  The MFMA GEMMs add
    32-product groups into fp32 accumulators (<= k/32 sequential adds per split, plus the group's own adds and a split-K combine):
    a path of at most k/16 + 64 roundings, below the worst case k (for the k >= 240 used here)."""
    return U * (k / 16 + 64)


# ------------------------------------------------------------------------------------------------ A1 / A2: im2col, col2im
@pytest.mark.parametrize("C", [3, 80, 512])
@pytest.mark.parametrize("T_in", [1, 2, 3, 96, 1599, 1600, 3001])
def test_im2col_is_the_padded_gather_bit_for_bit(K, T_in, C):
    for B in (1, 3):
        g = _gen("im2col", T_in, C, B)
        x32 = torch.randn(B, C, T_in, generator=g) * 3
        a16 = (torch.randn(B, T_in, C, generator=g) * 3).to(torch.bfloat16)
        for stride in (1, 2):
            # channel-major fp32 input: the kernel rounds each value to bf16 (RNE), as .to(torch.bfloat16) does
            p, T_out = K.im2col_k3(x32.to(DEV), False, B, C, T_in, stride)
            assert T_out == (T_in - 1) // stride + 1
            _bits_equal(p, _im2col_ref(x32, False, stride).to(torch.bfloat16), f"im2col cm B{B} s{stride}")
            p, _ = K.im2col_k3(a16.to(DEV), True, B, C, T_in, stride)
            _bits_equal(p, _im2col_ref(a16, True, stride).to(torch.bfloat16), f"im2col tm B{B} s{stride}")


@pytest.mark.parametrize("C", [3, 80, 512])
@pytest.mark.parametrize("T_in", [1, 2, 3, 96, 1599, 1600, 3001])
def test_col2im_is_the_ordered_sum_and_the_adjoint_of_im2col(K, T_in, C):
    for B in (1, 3):
        for stride in (1, 2):
            T_out = (T_in - 1) // stride + 1
            g = _gen("col2im", T_in, C, B, stride)
            dp = torch.randn(B * T_out, C * 3, generator=g).to(torch.bfloat16)
            got = K.col2im_k3(dp.to(DEV), B, C, T_in, T_out, stride)
            _bits_equal(got, _col2im_ref(dp, B, C, T_in, T_out, stride), f"col2im B{B} s{stride}")
            # adjoint: small integers (sums of <= 3 values in [-4, 4] are exact everywhere) against autograd through the gather
            di = torch.randint(-4, 5, (B * T_out, C * 3), generator=g).to(torch.bfloat16)
            x = torch.zeros(B, T_in, C, dtype=torch.float64, requires_grad=True)
            xp = F.pad(x.permute(0, 2, 1), (1, 1)).unfold(2, 3, stride).permute(0, 2, 1, 3).reshape(B * T_out, C * 3)
            xp.backward(di.double())
            got = K.col2im_k3(di.to(DEV), B, C, T_in, T_out, stride)
            _bits_equal(got, x.grad.to(torch.bfloat16), f"col2im adjoint B{B} s{stride}")


# ------------------------------------------------------------------------------------------------ A3: bias + GELU forward
def _gelu_fwd_bound(v, ref):
    """a32: the erfcc fit of Phi is within 3.3e-6 relative as evaluated in fp32 on bf16 inputs (csrc/common.h); on these fp32
    inputs err / (1e-5 |ref| + ...) measured up to 0.93, so 2e-5 |ref| (2x headroom).  The fp32 rounding of z + b moves the input
    by <= u |v|, hence + 2u |v gelu'(v)|; results below ~2e-38 may come out flushed to zero, hence the 1e-37 floor."""
    return 2e-5 * ref.abs() + 2 * U * (v * _gelu_grad64(v)).abs() + 1e-37


# (131077 x 2048 would be 2 GB of float64 per host tensor: at 131077 rows C = 768 is the MLM head's shape)
@pytest.mark.parametrize("R,C", [(R, C) for R in (1, 3, 513) for C in (4, 512, 768, 2048)] + [(131077, C) for C in (4, 512, 768)])
def test_bias_gelu_forward_against_float64(K, R, C):
    g = _gen("bgf", R, C)
    z = torch.randn(R, C, generator=g) * 3
    b = torch.randn(C, generator=g)
    a16, a32 = K.bias_gelu_fwd(z.to(DEV), b.to(DEV), True, True)
    a16, a32 = a16.cpu(), a32.cpu()
    _bits_equal(a16, a32.to(torch.bfloat16), "a16 == bf16(a32)")
    for r0 in range(0, R, CHUNK):
        v = z[r0:r0 + CHUNK].double() + b.double()
        ref = _gelu64(v)
        bnd = _gelu_fwd_bound(v, ref)
        _check(a32[r0:r0 + CHUNK], ref, bnd, f"a32 rows {r0}+")
        # a16: one bf16 rounding of a32 (relative 2^-8, the unit roundoff of an 8-bit significand): 2^-8 |ref| + (1 + 2^-8) bnd
        _check(a16[r0:r0 + CHUNK], ref, 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * bnd, f"a16 rows {r0}+")


# ------------------------------------------------------------------------------------------------ A4: bias + GELU backward
def _colsum_depth(R, nblk):
    """Longest chain of fp32 additions from an element to its column sum: ceil(R / nblk) rows per block, then the final kernel's
    four waves of ceil(nblk / 4) partials each (split over four accumulators) and three adds of the fixed-order combine."""
    return math.ceil(R / nblk) + math.ceil(nblk / 4) + 4


BWD_CASES = ([(R, 512, dt, False) for R in (1, 511, 512, 513, 1023, 1024, 1025, 3200, 131075) for dt in ("bf16", "f32")]
             + [(R, 6, dt, False) for R in (1, 511, 512, 513, 1023, 1024, 1025, 3200, 131075) for dt in ("bf16", "f32")]
             + [(R, C, dt, False) for R in (1, 513, 1025, 3200) for C in (514, 4100) for dt in ("bf16", "f32")]
             + [(R, 512, dt, True) for R in (1, 513, 1025, 3200) for dt in ("bf16", "f32")]
             + [(131075, 768, dt, False) for dt in ("bf16", "f32")])


@pytest.mark.parametrize("R,C,da_dtype,misaligned", BWD_CASES)
def test_bias_gelu_backward_against_float64(K, R, C, da_dtype, misaligned):
    """C % 4 == 0 and C <= 4096 with aligned pointers take the vec kernel (four columns, two rows in flight); C in {6, 514, 4100}
    or a da view one element off a 16-byte boundary take the scalar kernel.  R up to 512 is one block per row, beyond that
    grid-stride with the pair loop and its tail; the column sums reach colsum2 with 1..512 partials."""
    g = _gen("bgb", R, C, da_dtype, misaligned)
    z = torch.randn(R, C, generator=g) * 3
    b = torch.randn(C, generator=g)
    da = torch.randn(R, C, generator=g)
    if da_dtype == "bf16":
        da = da.to(torch.bfloat16)
    da_dev = da.to(DEV)
    if misaligned:
        da_dev = _misaligned(da_dev)
    dz, db = K.bias_gelu_bwd(da_dev, z.to(DEV), b.to(DEV))
    dz = dz.cpu()
    for r0 in range(0, R, CHUNK):
        v = z[r0:r0 + CHUNK].double() + b.double()
        g_ = da[r0:r0 + CHUNK].double()
        ref = g_ * _gelu_grad64(v)
        # one bf16 rounding (2^-8 relative) of an fp32 value whose gelu' is absolutely within 1e-5 (Phi within 3.3e-6 relative,
        # x phi(x) within a few ulps) and moved by <= |gelu''| u |v| <= u |v| through the fp32 rounding of z + b:
        # 2^-8 |ref| + (1 + 2^-8) |da| (1e-5 + 2u |v|)
        bnd = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * g_.abs() * (1e-5 + 2 * U * v.abs())
        _check(dz[r0:r0 + CHUNK], ref, bnd, f"dz rows {r0}+")
    # db: float64 column sums of the kernel's own dz; fp32 summation error <= depth * u * sum |dz|
    nblk = K.query("cm3p_bias_gelu_bwd_blocks", R)
    dzd = dz.double()
    _check(db, dzd.sum(0), _colsum_depth(R, nblk) * U * dzd.abs().sum(0), "db")


# ------------------------------------------------------------------------------------------------ A5: _ConvGeluFn stages
@pytest.mark.parametrize("B,T", [(2, 1600), (3, 1001)])
def test_conv_gelu_stages_against_float64(K, B, T):
    """conv1 (80 mels -> 512, stride 1, channel-major fp32 in, bf16 out) and conv2 (512 -> 512, stride 2, token-major bf16 in,
    fp32 out) of the audio front end, each stage against float64 fed the kernel's own input to it: z from the kernel's patches,
    a from its z, dW from its dz, dp from its dz, dx = col2im of its dp."""
    from cm3p_amd.audio import _ConvGeluFn

    g = _gen("convstages", B, T)
    Co = 512
    for Ci, stride, token_major, out_f32 in ((80, 1, False, False), (512, 2, True, True)):
        if token_major:
            x = (torch.randn(B, T, Ci, generator=g)).to(torch.bfloat16).to(DEV).requires_grad_(True)
        else:
            x = torch.randn(B, Ci, T, generator=g).to(DEV)
        W = (torch.randn(Co, Ci, 3, generator=g) / math.sqrt(3 * Ci)).to(DEV).requires_grad_(True)
        bias = (torch.randn(Co, generator=g) * 0.1).to(DEV).requires_grad_(True)
        y = _ConvGeluFn.apply(x, W, bias, stride, token_major, out_f32)
        T_out = (T - 1) // stride + 1
        assert y.shape == (B, T_out, Co) and y.dtype == (torch.float32 if out_f32 else torch.bfloat16)
        patches, Wb, z, b32 = (t.detach() for t in y.grad_fn.pack[:4])
        _bits_equal(patches, _im2col_ref(x.detach().cpu(), token_major, stride).to(torch.bfloat16), f"patches {Ci}")
        Pd, Wd = patches.double().cpu(), Wb.double().cpu()
        kc = Ci * 3
        _check(z, Pd @ Wd.t(), _contraction_c(kc) * (Pd.abs() @ Wd.abs().t()), f"z {Ci} (K={kc})")
        v = z.double().cpu() + b32.double().cpu()
        ref = _gelu64(v)
        bnd = _gelu_fwd_bound(v, ref)
        if not out_f32:  # one bf16 rounding more (2^-8 relative)
            bnd = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * bnd
        _check(y.reshape(-1, Co), ref, bnd, f"a {Ci}")

        da = torch.randn(B, T_out, Co, generator=g).to(y.dtype).to(DEV)
        y.backward(da)
        # the backward's dz, recomputed by the same deterministic call (its db must come out bit-identical)
        dz, db = K.bias_gelu_bwd(da.reshape(-1, Co), z, b32)
        _bits_equal(bias.grad, db, f"db {Ci} (same call, same bits)")
        dzd = dz.double().cpu()
        kw = B * T_out
        _check(W.grad.reshape(Co, kc), dzd.t() @ Pd, _contraction_c(kw) * (dzd.abs().t() @ Pd.abs()), f"dW {Ci} (K={kw})")
        if token_major:
            dp = K.linear_dgrad(dz, Wb)
            ref = dzd @ Wd
            # contraction over Co, then one bf16 rounding of the result (2^-8 relative)
            _check(dp, ref, 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * _contraction_c(Co) * (dzd.abs() @ Wd.abs()), f"dp {Ci} (K={Co})")
            _bits_equal(x.grad, _col2im_ref(dp.cpu(), B, Ci, T, T_out, stride), f"dx {Ci}")


# ------------------------------------------------------------------------------------------------ A7: refusals
def test_conv_front_end_refuses_what_it_cannot_do(K):
    from cm3p_amd._lib import Cm3pHipError, call, ptr, stream
    from cm3p_amd.audio import _ConvGeluFn

    B, C, T = 1, 8, 10
    a = torch.zeros(B, T, C, dtype=torch.bfloat16, device=DEV)
    p = torch.zeros(B * T, C * 3, dtype=torch.bfloat16, device=DEV)
    call("cm3p_im2col_k3", ptr(a), 1, ptr(p), B, C, T, T, 1, stream())  # (the valid call, for contrast)
    with pytest.raises(Cm3pHipError):
        call("cm3p_im2col_k3", ptr(a), 1, ptr(p), B, C, T, (T - 1) // 3 + 1, 3, stream())  # stride 3
    with pytest.raises(Cm3pHipError):
        call("cm3p_im2col_k3", ptr(a), 1, ptr(p), B, C, T, T - 1, 1, stream())  # T_out != (T_in - 1) / stride + 1
    W = torch.zeros(8, C + 1, 3, device=DEV)
    with pytest.raises(ValueError):
        _ConvGeluFn.apply(a, W, torch.zeros(8, device=DEV), 1, True, True)
    x = torch.randn(B, C, T, device=DEV, requires_grad=True)
    y = _ConvGeluFn.apply(x, torch.randn(8, C, 3, device=DEV), torch.zeros(8, device=DEV), 1, False, True)
    with pytest.raises(NotImplementedError):
        y.sum().backward()


# ------------------------------------------------------------------------------------------------ B1: fp32 GEMM
def _gemm_f32_case(K, M, N, Kd, form, g, alpha=1.0, accumulate=False, ldc=None):
    from cm3p_amd._lib import call, ptr, stream

    a = torch.randn(M, Kd, generator=g)
    b = torch.randn(N, Kd, generator=g)
    # (the device copies are held by name while the kernel runs: a temporary's memory would be handed to the next one)
    # storage of each operand: N = row-major [rows, K] (strides (K, 1)); T = stored transposed [K, rows] (strides (1, rows))
    a_st, a_s = (a.t().contiguous(), (1, M)) if form[0] == "T" else (a, (Kd, 1))
    b_st, b_s = (b.t().contiguous(), (1, N)) if form[1] == "T" else (b, (Kd, 1))
    ldc = N if ldc is None else ldc
    c0 = torch.randn(M, ldc, generator=g)
    c = c0.to(DEV)
    a_dev, b_dev = a_st.to(DEV), b_st.to(DEV)
    call("cm3p_gemm_f32", ptr(a_dev), ptr(b_dev), ptr(c), M, N, Kd, a_s[0], a_s[1], b_s[0], b_s[1], ldc, alpha,
         int(accumulate), stream())
    c = c.cpu()
    ad, bd = a.double(), b.double()
    ref = alpha * (ad @ bd.t()) + (c0[:, :N].double() if accumulate else 0)
    # sequential fma chain over K: a path of K roundings in the worst case; random-sign operands stay far below it, and
    # 2 sqrt(K) + 2 (<= K for K >= 17, = K at K = 1) covers the chain's error with room.  Then one rounding each for alpha * acc
    # and for the accumulate add: 2u |ref| (+ 2u |C0|).
    ck = U * min(Kd, 2 * math.sqrt(Kd) + 2)
    bnd = abs(alpha) * ck * (ad.abs() @ bd.abs().t()) + 2 * U * ref.abs() + (2 * U * c0[:, :N].double().abs() if accumulate else 0)
    _check(c[:, :N], ref, bnd + 1e-38, f"gemm_f32 {form} {M}x{N}x{Kd} alpha={alpha} acc={accumulate}")
    if ldc > N:
        _bits_equal(c[:, N:], c0[:, N:], "gemm_f32 ldc gap untouched")


@pytest.mark.parametrize("form", ["NT", "TN", "NN", "TT"])
def test_gemm_f32_all_stride_forms(K, form):
    """The four forms the head uses: NT projections / logits, TN (TT) weight and logit gradients, NN input gradients
    (modeling_cm3p.py: _ProjectFn, _LogitsFn).  Operand form letters name A then B^T's storage."""
    sizes = (1, 17, 33, 257)
    g = _gen("gemmf32", form)
    for M in sizes:
        for N in sizes:
            for Kd in sizes:
                _gemm_f32_case(K, M, N, Kd, form, g)
    for M, N, Kd in ((32, 512, 768), (256, 256, 512)):
        _gemm_f32_case(K, M, N, Kd, form, g)
        _gemm_f32_case(K, M, N, Kd, form, g, alpha=-0.75, accumulate=True)
        _gemm_f32_case(K, M, N, Kd, form, g, alpha=1.5, accumulate=False, ldc=N + 13)
        _gemm_f32_case(K, M, N, Kd, form, g, alpha=0.5, accumulate=True, ldc=N + 4)


# ------------------------------------------------------------------------------------------------ B2: cross entropy of cm3p_loss
def _captured_specs(L, classes=None):
    """The spec list cm3p_loss_hip builds for L (captured by swapping the autograd node for a recorder)."""
    from cm3p_amd import modeling_cm3p as M

    got = {}

    class _Rec:
        @staticmethod
        def apply(specs, *logits):
            got["specs"] = specs
            return torch.zeros((), device=L.device)

    orig = M._CrossEntropySumFn
    M._CrossEntropySumFn = _Rec
    try:
        M.cm3p_loss_hip(L, classes)
    finally:
        M._CrossEntropySumFn = orig
    return got["specs"]


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2051])
def test_cross_entropy_with_the_specs_of_the_contrastive_loss(K, n, dims):
    from cm3p_amd import modeling_cm3p as M

    g = _gen("ce", n, dims)
    V = 3
    if dims == 2:
        L = torch.randn(n, n, generator=g) * 3
        classes = None
    else:
        L = torch.randn(n, V, n, generator=g) * 3
        classes = torch.randint(0, 3, (n, V), generator=g)
        classes[torch.arange(n), torch.randint(0, V, (n,), generator=g)] = 0  # every row has a true variation
    Ld = L.to(DEV)
    specs = _captured_specs(Ld, None if classes is None else classes.to(DEV))
    flat = L.reshape(-1).double()
    total_ref = 0.0
    for (ti, rows, cols, rs, cs, roff, target, coef) in specs:
        gs = coef / rows
        d0 = torch.randn(L.shape, generator=g) * gs  # a non-zero gradient buffer that must be accumulated into
        d = d0.to(DEV)
        loss_rows = K.cross_entropy(Ld, rows, cols, rs, cs, target, roff, gs, d)
        base = roff.cpu() if roff is not None else torch.arange(rows) * rs
        idx = base[:, None] + torch.arange(cols)[None, :] * cs  # [rows, cols] positions in L
        x = flat[idx]
        t = target.cpu()
        ls = torch.log_softmax(x, 1)
        ref = -ls[torch.arange(rows), t]
        lse = torch.logsumexp(x, 1)
        # rtol 1e-6 / atol 1e-6 of test_head_kernels, relative to the magnitudes that the final lse - x[t] subtracts
        _check(loss_rows, ref, 1e-6 + 1e-6 * (lse.abs() + x[torch.arange(rows), t].abs()), f"loss rows {rows}x{cols}")
        delta = gs * (ls.exp() - F.one_hot(t, cols).double())
        want = d0.reshape(-1).double().clone()
        want[idx.reshape(-1)] += delta.reshape(-1)
        got = d.cpu().reshape(-1)
        touched = torch.zeros(want.numel(), dtype=torch.bool)
        touched[idx.reshape(-1)] = True
        # test_head_kernels' 1e-7 + 1e-5 |ref| on the added term, plus the one rounding of the accumulate (u |result|)
        _check(got[touched], want[touched], 1e-7 + 1e-5 * delta.reshape(-1).abs() + U * want[touched].abs(), f"dlogits {rows}x{cols}")
        _bits_equal(got[~touched], d0.reshape(-1)[~touched], "dlogits outside the view untouched")
        total_ref += coef * ref.mean().item()
    loss = M.cm3p_loss_hip(Ld.clone().requires_grad_(True), None if classes is None else classes.to(DEV))
    _check(loss.reshape(1), torch.tensor([total_ref]), 1e-6 + 1e-6 * abs(total_ref), "cm3p_loss")


# ------------------------------------------------------------------------------------------------ B3: masked cross entropy
@pytest.mark.parametrize("rows,cols,pitch,frac", [(70, 37, 40, 0.5), (300, 3167, 3168, 0.3), (129, 1000, 1003, 1.0), (5, 1, 4, 0.6),
                                                  (33, 257, 260, 0.0)])
def test_cross_entropy_masked_against_float64(K, rows, cols, pitch, frac):
    """loss = mean over rows labelled in [0, cols) (F.cross_entropy(ignore_index=-100); the kernel ignores other out-of-range
    labels too, where torch raises - the reference gets -100 for them); dlogits = grad_scale / #labelled (softmax - onehot) on
    labelled rows, exactly zero on ignored rows and pad columns."""
    g = _gen("cem", rows, cols)
    x = torch.zeros(rows, pitch)
    x[:, :cols] = torch.randn(rows, cols, generator=g) * 3
    x[:, cols:] = 7.0  # pad columns: never read as logits
    lab = torch.randint(0, cols, (rows,), generator=g)
    keep = torch.rand(rows, generator=g) < frac
    lab = torch.where(keep, lab, torch.full_like(lab, -100))
    if rows > 4 and frac > 0:
        lab[1], lab[3] = cols, -5  # out-of-range labels: ignored
    lab_ref = torch.where((lab >= 0) & (lab < cols), lab, torch.full_like(lab, -100))
    n_valid = int((lab_ref != -100).sum())
    scale = 0.37
    inv = K.inv_valid_count(lab_ref.to(DEV), -100)
    loss_rows, dl = K.cross_entropy_masked(x.to(DEV), cols, lab.to(DEV), -100, scale, inv, True)
    assert dl.shape == (rows, pitch)
    got = K.scale_by(K.sum_f32(loss_rows, 1.0), inv)
    xr = x[:, :cols].double().requires_grad_(True)
    if n_valid:
        want = F.cross_entropy(xr, lab_ref, ignore_index=-100)
        (want * scale).backward()
        # as test_masked_lm_loss_kernels: fp32 summation-order error of the loss
        _check(got, want.detach().reshape(1), 1e-6 + 1e-5 * want.abs().item(), "masked CE loss")
        wantg = torch.zeros(rows, pitch, dtype=torch.float64)
        wantg[:, :cols] = xr.grad
        _check(dl, wantg, 1e-7 + 1e-5 * wantg.abs(), "masked CE dlogits")
    else:
        assert got.item() == 0.0  # (inv = 1 / max(0, 1): no labelled row gives loss 0, where torch returns NaN)
    dlc = dl.cpu()
    ign = lab_ref == -100
    assert torch.equal(loss_rows.cpu()[ign], torch.zeros(int(ign.sum())))
    assert torch.equal(dlc[ign], torch.zeros(int(ign.sum()), pitch))
    assert torch.equal(dlc[:, cols:], torch.zeros(rows, pitch - cols))


# ------------------------------------------------------------------------------------------------ B4: pointwise losses
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 224])
def test_pointwise_loss_against_float64(K, n, kind):
    g = _gen("pw", n, kind)
    x = torch.randn(n, generator=g) * 30
    x[: min(n, 4)] = torch.tensor([100.0, -100.0, 99.5, -0.0])[: min(n, 4)]
    y = torch.rand(n, generator=g) if kind == 1 else torch.randn(n, generator=g) * 30  # soft targets for BCE
    loss, dx = K.pointwise_loss(x.to(DEV), y.to(DEV), kind)
    xd = x.double().requires_grad_(True)
    yd = y.double()
    ref = F.mse_loss(xd, yd) if kind == 0 else F.binary_cross_entropy_with_logits(xd, yd)
    ref.backward()
    if kind == 0:
        terms = (xd.detach() - yd) ** 2
        # per term: (a - t) rounded then squared: 3u |term|; the single-workgroup sum: <= 2 + 8 + 2 adds on any path
        term_err = 3 * U * terms
        # dx = 2 (a - t) * fl(1/n): three roundings
        dx_bnd = 4 * U * xd.grad.abs()
    else:
        a = xd.detach()
        terms = torch.clamp(a, min=0) - a * yd + torch.log1p(torch.exp(-a.abs()))
        # max(a, 0) - a t + log1p(exp(-|a|)): the product and the two adds round at the size of their operands (2u each),
        # log1pf(expf(.)) within 4 ulps
        term_err = 2 * U * (a.clamp(min=0) + (a * yd).abs() + terms.abs()) + 4 * U * torch.log1p(torch.exp(-a.abs()))
        # sigmoid(a) - t: sigmoid within 4 ulps (8u), the subtraction at the size of its operands, then * fl(1/n)
        sig = torch.sigmoid(a)
        dx_bnd = (8 * U * sig + 2 * U * (sig + yd)) / n + 2 * U * xd.grad.abs() + 1e-40
    depth = 12
    loss_bnd = (term_err.sum() + depth * U * terms.abs().sum()) / n + 2 * U * abs(ref.item())
    _check(loss, ref.detach().reshape(1), loss_bnd, f"pointwise loss kind {kind} n {n}")
    _check(dx, xd.grad, dx_bnd, f"pointwise dx kind {kind} n {n}")


# ------------------------------------------------------------------------------------------------ B5 / B6: colsum, add_bias
COLSUM_CASES = ([(R, C, False) for R in (1, 511, 512, 513, 131073) for C in (768, 6)]
                + [(R, 4100, False) for R in (1, 511, 512, 513)] + [(R, 768, True) for R in (1, 513, 131073)])


@pytest.mark.parametrize("rows,cols,misaligned", COLSUM_CASES)
def test_colsum_against_float64(K, rows, cols, misaligned):
    """vec kernel: cols % 4 == 0, cols <= 4096, aligned; scalar otherwise (6, 4100, a view off a 16-byte boundary)."""
    g = _gen("colsum", rows, cols, misaligned)
    x = torch.randn(rows, cols, generator=g)
    xd = x.to(DEV)
    if misaligned:
        xd = _misaligned(xd)
    got = K.colsum_f32(xd)
    nblk = K.query("cm3p_colsum_blocks", rows)
    _check(got, x.double().sum(0), _colsum_depth(rows, nblk) * U * x.double().abs().sum(0), f"colsum {rows}x{cols}")


@pytest.mark.parametrize("rows,cols,misaligned", [(8192, 768, False), (3, 8, False), (200003, 6, False), (1, 5, False),
                                                  (70000, 64, True)])
def test_add_bias_is_the_fp32_add_bit_for_bit(K, rows, cols, misaligned):
    """8192 x 768 (vec) and 200003 x 6 (scalar) launch more than the 4096-workgroup cap and grid-stride."""
    g = _gen("addbias", rows, cols)
    x = torch.randn(rows, cols, generator=g)
    b = torch.randn(cols, generator=g)
    xd = x.to(DEV)
    if misaligned:
        xd = _misaligned(xd)
    K.add_bias_(xd, b.to(DEV))
    _bits_equal(xd, x + b, f"add_bias {rows}x{cols}")


# ------------------------------------------------------------------------------------------------ B7: add_f32, cast
@pytest.mark.parametrize("shape", [(131072, 768), (3, 4), (1, 1028)])
def test_add_f32_is_the_fp32_add_then_rne(K, shape):
    g = _gen("addf32", shape)
    a = torch.randn(shape, generator=g)
    for b in (torch.randn(shape, generator=g), torch.randn(shape, generator=g).to(torch.bfloat16)):
        want = a + b.float()
        y32, y16 = K.add_f32(a.to(DEV), b.to(DEV), want_bf16=True, inplace=False)
        _bits_equal(y32, want, f"add_f32 y32 {b.dtype}")
        _bits_equal(y16, want.to(torch.bfloat16), f"add_f32 y16 {b.dtype}")
        ad = a.to(DEV)
        y32, y16 = K.add_f32(ad, b.to(DEV), want_bf16=False, inplace=True)
        assert y32.data_ptr() == ad.data_ptr() and y16 is None
        _bits_equal(ad, want, f"add_f32 in place {b.dtype}")


def test_add_f32_with_no_elements(K):
    """n = 0 with real pointers is a no-op that succeeds; null pointers are refused even then (an empty torch tensor may hand
    the entry a null address, so the wrapper's behaviour on empty tensors is the allocator's: callers do not pass them)."""
    from cm3p_amd._lib import Cm3pHipError, call, ptr, stream

    a = torch.full((4,), 3.0, device=DEV)
    y = torch.full((4,), 5.0, device=DEV)
    call("cm3p_add_f32", ptr(a), ptr(a), 0, ptr(y), None, 0, stream())
    assert y.cpu().tolist() == [5.0] * 4
    with pytest.raises(Cm3pHipError):
        call("cm3p_add_f32", None, None, 0, ptr(y), None, 0, stream())


@pytest.mark.parametrize("n", [4, 1028, 768 * 1152 + 4])
def test_cast_f32_bf16_is_rne(K, n):
    g = _gen("cast", n)
    x = torch.randn(n, generator=g) * 100
    x[:3] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)])  # ties: to even
    _bits_equal(K.cast_bf16(x.to(DEV)), x.to(torch.bfloat16), "cast_f32_bf16")


# ------------------------------------------------------------------------------------------------ B8: scale_exp, dot, sum
@pytest.mark.parametrize("n", [1, 255, 257, 1000003])
def test_scale_exp_dot_and_sum_against_float64(K, n):
    g = _gen("red", n)
    x = torch.randn(n, generator=g)
    y = torch.randn(n, generator=g)
    s = torch.tensor([2.65926])  # log(1 / 0.07), the reference's initial logit scale
    got = K.scale_exp(x.to(DEV), s.to(DEV))
    ref = x.double() * math.exp(s.double().item())
    # expf within 1 ulp, then the product's rounding: 2 fp32 ulps of the result (an ulp is <= 2^-23 |value|)
    _check(got, ref, 2 * 2.0 ** -23 * ref.abs() + 1e-40, f"scale_exp n {n}")
    got = K.dot_f32(x.to(DEV), y.to(DEV))
    prod = x.double() * y.double()
    # one workgroup: ceil(n / 256) products and adds per thread, then 8 levels of the 256-thread reduction (n = 1: one rounding)
    c = min(n, math.ceil(n / 256) + 9) * U
    _check(got, prod.sum().reshape(1), c * prod.abs().sum(), f"dot_f32 n {n} (c = {c / U:.0f} u)")
    for scale, acc in ((0.5, False), (-3.0, True)):
        out0 = torch.tensor([1.25])
        out = out0.to(DEV)
        K.sum_f32(x.to(DEV), scale, out=out, accumulate=acc)
        ref = scale * x.double().sum() + (out0.double() if acc else 0)
        # 1024 threads, four accumulators over ceil(n / 4096) strides, the tail, 16 reduction levels; then * scale (+ out)
        c = (math.ceil(n / 4096) + 20) * U
        _check(out, ref.reshape(1), c * abs(scale) * x.double().abs().sum() + 2 * U * (ref.abs() + 1.25), f"sum_f32 n {n} acc {acc}")


# ------------------------------------------------------------------------------------------------ C: LayerNorm past the grid
@pytest.mark.parametrize("rows,H", [(131072, 768), (32771, 512), (65537, 256)])
def test_layernorm_with_many_rows_per_wave(K, rows, H):
    """More rows than the backward's 1024 x 4 waves: each wave accumulates its rows' dy * xhat in registers (32 rows a wave at
    131072), then the partial rows are reduced.  The backward's reference is fed the kernel's own mean / rstd."""
    g = _gen("ln", rows, H)
    x = torch.randn(rows, H, generator=g) * 2 + 0.5
    w = 1 + 0.2 * torch.randn(H, generator=g)
    y32, y16, mean, rstd = K.layernorm_fwd(x.to(DEV), w.to(DEV), 1e-5, True, True)
    y32, y16 = y32.cpu(), y16.cpu()
    mean_k, rstd_k = mean.cpu().double(), rstd.cpu().double()
    for r0 in range(0, rows, CHUNK):
        xd = x[r0:r0 + CHUNK].double()
        yref = F.layer_norm(xd, (H,), w.double(), None, 1e-5)
        # the bounds of test_layernorm_fwd_bwd (per row: they do not grow with the row count)
        _check(y32[r0:r0 + CHUNK], yref, 2e-5 + 1e-5 * yref.abs(), f"ln y rows {r0}+")
        _check(y16[r0:r0 + CHUNK], yref, 1e-4 + 8e-3 * yref.abs(), f"ln y16 rows {r0}+")
    for dy_dtype in (torch.float32, torch.bfloat16):
        dy = torch.randn(rows, H, generator=g).to(dy_dtype)
        dres = torch.randn(rows, H, generator=g)
        dx32, _, dw = K.layernorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), mean, rstd, dres.to(DEV), False)
        dx32 = dx32.cpu()
        dw_ref = torch.zeros(H, dtype=torch.float64)
        s_abs = torch.zeros(H, dtype=torch.float64)
        for r0 in range(0, rows, CHUNK):
            xh = (x[r0:r0 + CHUNK].double() - mean_k[r0:r0 + CHUNK, None]) * rstd_k[r0:r0 + CHUNK, None]
            gy = dy[r0:r0 + CHUNK].double()
            gw = gy * w.double()
            dx = (gw - gw.mean(1, keepdim=True) - xh * (gw * xh).mean(1, keepdim=True)) * rstd_k[r0:r0 + CHUNK, None]
            dx = dx + dres[r0:r0 + CHUNK].double()
            _check(dx32[r0:r0 + CHUNK], dx, 5e-5 + 1e-5 * dx.abs(), f"ln dx {dy_dtype} rows {r0}+")  # (test_layernorm_fwd_bwd's)
            p = gy * xh
            dw_ref += p.sum(0)
            s_abs += p.abs().sum(0)
        # dw[c] = sum_r dy xhat, bounded by c u sum_r |dy xhat|.  The worst case along the longest addition path (rows / (4 nblk)
        # in a wave's registers, 2 for the four waves, nblk / 32 per colsum slice, 10 more, 3 for xhat and the product: c = 56
        # to 79 here) is looser than the old 2e-4 sqrt(rows); measured max err / (u sum |dy xhat|) = 0.068 over these six cases,
        # so c = 1/4 (3.7x headroom): 1.3e-3 at 131072 x 768, where a lost row moves a column by ~1
        _check(dw, dw_ref, 0.25 * U * s_abs, f"ln dw {dy_dtype}")


# ------------------------------------------------------------------------------------------------ D: classifier loss
def _classifier(num_labels=5):
    import copy

    from cases import CASES

    from cm3p_amd import CM3PConfig
    from cm3p_amd.modeling_cm3p import CM3PForBeatmapClassification

    bc = copy.deepcopy(CM3PConfig(**CASES["d64_cls_nopad"]["cfg"]).beatmap_config)
    bc.num_labels = num_labels
    bc.problem_type = None
    torch.manual_seed(0)
    return CM3PForBeatmapClassification(bc).to(DEV).train()


@pytest.mark.parametrize("labels", [[1, -100, 4, 0, -100, 2], [-100] * 5 + [3], [2, 0, 1, 4, 3, 3]])
def test_single_label_classifier_ignores_minus_100_rows(labels):
    """CrossEntropyLoss() (ref:cm3p/modeling_cm3p.py:1214-1216): mean over the labelled rows, no gradient into -100 rows."""
    model = _classifier()
    g = _gen("cls", len(labels))
    ids = torch.randint(3, 190, (len(labels), 96), generator=g)
    lab = torch.tensor(labels)
    out = model(input_ids=ids.to(DEV), attention_mask=torch.ones_like(ids).to(DEV), labels=lab.to(DEV))
    out.logits.retain_grad()
    out.loss.backward()
    L = out.logits.detach().double().cpu().requires_grad_(True)
    ref = F.cross_entropy(L, lab)
    ref.backward()
    # fp32 row losses and their sum (test_masked_lm_loss_kernels' bound); the gradient as test_head_kernels'
    _check(out.loss.reshape(1), ref.detach().reshape(1), 1e-6 + 1e-5 * ref.abs().item(), "classifier loss")
    _check(out.logits.grad, L.grad, 1e-7 + 1e-5 * L.grad.abs(), "classifier dlogits")
    assert torch.equal(out.logits.grad.cpu()[lab == -100], torch.zeros(int((lab == -100).sum()), 5))


def test_single_label_classifier_without_a_labelled_row_gives_zero():
    """torch returns NaN for a batch whose labels are all -100; this implementation returns loss 0 and a zero gradient (the same
    choice as the masked-LM loss), so one empty batch cannot poison the weights."""
    model = _classifier()
    ids = torch.randint(3, 190, (3, 64), generator=_gen("cls0"))
    out = model(input_ids=ids.to(DEV), attention_mask=torch.ones_like(ids).to(DEV), labels=torch.full((3,), -100, device=DEV))
    out.logits.retain_grad()
    out.loss.backward()
    assert out.loss.item() == 0.0
    assert torch.equal(out.logits.grad.cpu(), torch.zeros(3, 5))
