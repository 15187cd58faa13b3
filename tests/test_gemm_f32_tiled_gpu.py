"""The register-tiled route of cm3p_gemm_f32 (CM3P_GEMM_F32_TILED or-ed into `accumulate`), called through the C entry.

1. Route equality: on the same arguments and the same initial C the tiled kernel returns the bits of the 16 x 16 kernel, which
   tests/test_conv_head_kernels_gpu.py specifies against float64.  Both compute, per output, one chain of fmaf in ascending k with k
   zero-padded to a multiple of 16, then one shared store expression - so equality is exact, with no tolerance.
2. The tiled route against float64 directly, at the head's shapes, with the bound of that file restated here.
3. Two tiled calls give the same bits.

Operand forms are named as the issue of this kernel and DESIGN name them, by BLAS letters of C = op(A) op(B): NT = both operands
with their unit stride along k (projections, logits), NN = A along k, B along its rows (input gradients), TN = both along their rows
(weight and logit gradients), TT = A along its rows, B along k.
"""
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24  # fp32 unit roundoff
TILED = 2  # CM3P_GEMM_F32_TILED
FORMS = {"NT": ("k", "k"), "NN": ("k", "r"), "TN": ("r", "r"), "TT": ("r", "k")}  # unit stride of A, of B: along k or along rows


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _bits(t):
    return t.view(torch.int32)


def _stored(x, unit, pad4=False, offset=0):
    """x [rows, K] on the host -> (device buffer, the operand inside it, (row stride, k stride)).  unit 'k': row-major [rows, K];
    unit 'r': stored transposed, [K, rows].  pad4: the leading dimension is the next multiple of 4 past the row length (padding
    inside the buffer); offset: floats between a 16-byte boundary and the first element (the kernels' scalar paths)."""
    src = x if unit == "k" else x.t()
    ld = (src.shape[1] + 4) // 4 * 4 if pad4 else src.shape[1]
    buf = torch.full((offset + src.shape[0] * ld,), float("nan"))  # (padding that is read by mistake poisons the result)
    buf[offset:].view(src.shape[0], ld)[:, :src.shape[1]] = src
    buf = buf.to(DEV)
    return buf, buf[offset:], ((ld, 1) if unit == "k" else (1, ld))


def _call(a_op, a_s, b_op, b_s, c, M, N, Kd, ldc, alpha, flags):
    from cm3p_amd._lib import _DevPtr, call, stream

    def p(t):  # (a view into a buffer: _lib.ptr wants whole contiguous tensors, the entry point only an address)
        q = _DevPtr(t.data_ptr())
        q.dev = t.device.index
        return q

    call("cm3p_gemm_f32", p(a_op), p(b_op), p(c), M, N, Kd, a_s[0], a_s[1], b_s[0], b_s[1], ldc, alpha, flags, stream())


def _both_routes(a, b, form, c0, alpha, accumulate, pad4=False, offset=0):
    """-> (C of the 16 x 16 route, C of the tiled route), whole [M, ldc] buffers, from the same inputs and the same initial C."""
    M, Kd = a.shape
    N = b.shape[0]
    a_buf, a_op, a_s = _stored(a, FORMS[form][0], pad4, offset)
    b_buf, b_op, b_s = _stored(b, FORMS[form][1], pad4, offset)
    out = []
    for flags in (int(accumulate), int(accumulate) | TILED):
        c = c0.to(DEV)
        _call(a_op, a_s, b_op, b_s, c, M, N, Kd, c0.shape[1], alpha, flags)
        out.append(c)
    torch.cuda.synchronize()  # (a_buf / b_buf are held by name until both kernels ran)
    del a_buf, b_buf
    return out


def _assert_same(c_ref, c_tiled, c0, N, what):
    assert torch.equal(c_tiled, c_ref), f"{what}: routes differ"
    assert torch.equal(_bits(c_tiled), _bits(c_ref)), f"{what}: routes differ in the sign of a zero or the payload of a NaN"
    assert torch.isfinite(c_tiled[:, :N]).all(), f"{what}: padding was read"
    if c0.shape[1] > N:
        assert torch.equal(_bits(c_tiled[:, N:].cpu()), _bits(c0[:, N:])), f"{what}: ldc gap touched"


SIZES_MN = (1, 63, 64, 65, 129)
SIZES_K = (1, 15, 16, 17, 33, 512)
EPILOGUES = ((1.0, False, 0), (-0.75, True, 0), (1.5, False, 13), (0.5, True, 4))  # alpha, accumulate, ldc - N
EPILOGUE_SHAPES = ((65, 129, 33), (129, 63, 17), (1, 65, 512), (64, 64, 16), (63, 1, 15))
# From 2^20 outputs on the entry point takes its large tiles, chosen by M: 32 x 128 (M <= 32), 64 x 64 (M <= 64), 128 x 64.  One shape
# each, just past 2^20 outputs, with edges in M, N and k; below 2^20 (all of the grid above) it runs 16 x 16 outputs with k by 64.
LARGE_TILE_SHAPES = ((32, 32800, 17), (63, 16700, 33), (1025, 1025, 33), (129, 8192, 64))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_tiled_route_equals_the_16x16_route(form):
    """Every M, N in {1, 63, 64, 65, 129} (one row; one short of, exactly, and one past a 64-tile; past the 128-row tile - the three
    tile instances are chosen by M <= 32, <= 64, else) and K in {1, 15, 16, 17, 33, 512} (around the k tile of 16; 512 = the head's k,
    where a 16-byte load is aligned; 512 and 33 also cross the k tile of 64 of the few-outputs instance).  Then the four (alpha, accumulate, ldc) forms of the float64 test at a subset."""
    g = _gen("tiled-eq", form)
    for M in SIZES_MN:
        for N in SIZES_MN:
            for Kd in SIZES_K:
                a, b, c0 = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g), torch.randn(M, N, generator=g)
                c_ref, c_t = _both_routes(a, b, form, c0, 1.0, False)
                _assert_same(c_ref, c_t, c0, N, f"{form} {M}x{N}x{Kd}")
    for M, N, Kd in EPILOGUE_SHAPES + LARGE_TILE_SHAPES:
        assert (M * N >= 1 << 20) == ((M, N, Kd) in LARGE_TILE_SHAPES)
        for alpha, accumulate, gap in EPILOGUES:
            a, b, c0 = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g), torch.randn(M, N + gap, generator=g)
            c_ref, c_t = _both_routes(a, b, form, c0, alpha, accumulate)
            _assert_same(c_ref, c_t, c0, N, f"{form} {M}x{N}x{Kd} alpha={alpha} acc={accumulate} ldc=N+{gap}")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_tiled_route_equals_the_16x16_route_on_padded_and_misaligned_operands(form):
    """Leading dimensions that are a multiple of 4 around row counts and k that are not (16-byte loads with a tail of guarded scalar
    loads; the padding holds NaN), and operands that start 4 bytes past a 16-byte boundary (scalar loads throughout)."""
    g = _gen("tiled-pad", form)
    for M, N, Kd in ((65, 129, 33), (30, 130, 18), (129, 66, 50), (130, 8100, 18), (30, 35000, 18), (62, 17000, 50)):  # (the last three: large tiles)
        for pad4, offset in ((False, 1), (True, 0)):
            for alpha, accumulate, gap in EPILOGUES:
                a, b, c0 = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g), torch.randn(M, N + gap, generator=g)
                c_ref, c_t = _both_routes(a, b, form, c0, alpha, accumulate, pad4, offset)
                _assert_same(c_ref, c_t, c0, N, f"{form} {M}x{N}x{Kd} pad4={pad4} offset {offset} alpha={alpha} acc={accumulate}")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_a_product_that_underflows_to_minus_zero(form):
    """K = 1, a = -1e-30, b = 1e-30: the product underflows to -0, and the fifteen zero operands that pad the k tile turn the
    accumulator into +0 (fmaf(0, 0, -0) = +0).  The tiled kernel pads where the 16 x 16 kernel pads: same bits, sign included."""
    for M, N in ((1, 1), (65, 129), (1025, 1025)):
        a, b = torch.full((M, 1), -1e-30), torch.full((N, 1), 1e-30)
        for alpha, accumulate in ((1.0, False), (-1.0, False), (1.0, True)):
            c0 = torch.zeros(M, N) if not accumulate else -torch.zeros(M, N)
            c_ref, c_t = _both_routes(a, b, form, c0, alpha, accumulate)
            _assert_same(c_ref, c_t, c0, N, f"{form} -0 {M}x{N} alpha={alpha} acc={accumulate}")
            print(f"{form} {M}x{N} alpha={alpha} acc={accumulate}: bits {int(_bits(c_t)[0, 0]):#010x}")


def _against_float64(M, N, Kd, form, g, alpha=1.0, accumulate=False, gap=0):
    a, b, c0 = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g), torch.randn(M, N + gap, generator=g)
    a_buf, a_op, a_s = _stored(a, FORMS[form][0])
    b_buf, b_op, b_s = _stored(b, FORMS[form][1])
    c = c0.to(DEV)
    _call(a_op, a_s, b_op, b_s, c, M, N, Kd, N + gap, alpha, int(accumulate) | TILED)
    c = c.cpu()
    ad, bd = a.double(), b.double()
    ref = alpha * (ad @ bd.t()) + (c0[:, :N].double() if accumulate else 0)
    # (the bound of tests/test_conv_head_kernels_gpu.py::_gemm_f32_case, restated)  A sequential fma chain over K is a path of K
    # roundings in the worst case; random-sign operands stay far below it, and 2 sqrt(K) + 2 (<= K for K >= 17, = K at K = 1) covers
    # the chain's error with room.  Then one rounding each for alpha * acc and for the accumulate add: 2u |ref| (+ 2u |C0|).
    ck = U * min(Kd, 2 * math.sqrt(Kd) + 2)
    bnd = abs(alpha) * ck * (ad.abs() @ bd.abs().t()) + 2 * U * ref.abs() + (2 * U * c0[:, :N].double().abs() if accumulate else 0) + 1e-38
    err = (c[:, :N].double() - ref).abs()
    ratio = (err / bnd).max().item()
    print(f"tiled {form} {M}x{N}x{Kd} alpha={alpha} acc={accumulate}: max err/bound {ratio:.3g}")
    assert torch.isfinite(c[:, :N]).all() and ratio <= 1.0, f"tiled {form} {M}x{N}x{Kd} alpha={alpha} acc={accumulate}: err/bound {ratio:.3g}"
    if gap:
        assert torch.equal(_bits(c[:, N:]), _bits(c0[:, N:])), "ldc gap touched"


def test_tiled_route_against_float64():
    """The two head shapes of the float64 test in all four forms and epilogues, and a variation-sized logits problem scaled down,
    (b V, N b, P) = (512, 64, 512) NT, with its gradients: draw B (512 x 512, k = 64, NN) and draw^T A (64 x 512, k = 512, TN).
    All of these have fewer than 2^20 outputs (the 16 x 16-output instance); two shapes past it follow for the large tiles."""
    g = _gen("tiled-f64")
    for form in sorted(FORMS):
        for M, N, Kd in ((32, 512, 768), (256, 256, 512)):
            for alpha, accumulate, gap in EPILOGUES:
                _against_float64(M, N, Kd, form, g, alpha, accumulate, gap)
    _against_float64(512, 64, 512, "NT", g)
    _against_float64(512, 512, 64, "NN", g)
    _against_float64(64, 512, 512, "TN", g)
    for form in sorted(FORMS):  # 2^20 outputs: the large tiles
        _against_float64(2048, 512, 256, form, g)
        _against_float64(32, 32768, 96, form, g, -0.75, True, 4)


def test_tiled_route_repeats_its_bits():
    g = _gen("tiled-rep")
    for form, (M, N, Kd) in (("NT", (512, 64, 512)), ("NN", (129, 65, 33)), ("TN", (64, 512, 512)), ("TT", (32, 200, 100)),
                              ("NT", (2048, 512, 256)), ("TN", (32, 32800, 17))):
        a, b, c0 = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g), torch.randn(M, N, generator=g)
        a_buf, a_op, a_s = _stored(a, FORMS[form][0])
        b_buf, b_op, b_s = _stored(b, FORMS[form][1])
        out = []
        for _ in range(2):
            c = c0.to(DEV)
            _call(a_op, a_s, b_op, b_s, c, M, N, Kd, N, -0.75, 1 | TILED)
            out.append(c)
        assert torch.equal(_bits(out[0]), _bits(out[1])), f"{form} {M}x{N}x{Kd}"
