"""Kernel-level specifications of the three bf16 GEMM kernels - gemm_bf16_kernel (128 x 128, csrc/gemm.hip), gemm256_kernel
(csrc/gemm256.hip) and gemm8p_kernel ("the ring", csrc/gemm8p.hip) - against float64 at every instance and seam.

Conventions (as tests/test_row_kernels_gpu.py; check / bits_equal come through row_kernel_refs): the data generators, references,
bounds and the case table live in tests/gemm_refs.py, where tests/test_gemm_refs_host.py shows without a GPU that a torch fp32
restatement of the kernels' arithmetic passes every check used here and that wrong evaluations fail.  The operands are exact data
m 2^e at full bf16 significand width: the fp32 accumulator is exact, so everything that is a single IEEE operation after it is
asserted BIT FOR BIT against the float64 matmul; the RoPE, GeGLU and random-data checks are per element |got - ref| <= bound and
print their largest err / bound (`pytest -rP`).  Every case states the kernel and REBAL flag it is meant for (the table's hand-stated
entry) and asserts before it runs that cm3p_amd.kernels._gemm_tag agrees.  That tag is spelled from cm3p_gemm_route, the answer of
the one routing function (csrc/gemm.hip cm3p_gemm_route_of) that the entry point itself evaluates and then launches from: the
hand table is compared with the rule the dispatcher executes, under the CM3P_GEMM_IMPL of the call.  (The launch itself is still
not observed: what is asserted is the route, and the launchers have no decision left to make after it.)
Every big-path case of cm3p_gemm_bf16 and cm3p_qkv_gemm_rope runs three times: by default (the ring), under CM3P_GEMM_IMPL=256
(gemm256_kernel) and under CM3P_GEMM_IMPL=128 (the 128 x 128 kernel); cm3p_gemm_geglu exists on the ring only and the cases of
test_small_kernel_natively take the 128 x 128 kernel whatever the switch.  Every output lies inside a larger buffer
pre-filled with a NaN bit pattern, 64 rows before and 256 rows past the matrix (and the columns past N where ldc > N): the pattern
must survive around the matrix and must be gone inside it.

What the suite did not execute before, and the test that does now:

  1  the ring at one k-tile (K = 64, `sdone` at once) and at 1..5 k-tiles,   test_forward_every_epilogue_at_one_to_five_k_tiles
     plain and REBAL instances alternating
  2  3 to 4 work items per workgroup at 1..5 k-tiles (gemm8p_set_grid(64))   the same test and every edge / layout test below
  3  split-K on the big kernels: equal even splits, a shorter even last      test_wgrad_split_k_with_a_short_last_split,
     split, an odd last split (plain instance, mixed nk); linear_wgrad       test_linear_wgrad_reaches_the_big_kernel_by_the_librarys_own_split
     reaching the ring by cm3p_gemm_wgrad_splits
  4  remainders of 8, 72, 136, 248 rows / columns, under k-contiguous and    test_forward_edge_tiles, test_k_strided_operands_with_ragged_tiles,
     k-strided operands; the (0, 1) layout on all three kernels              test_small_kernel_natively
  5  stores past the matrix (guards around every output); ldc = N + 8,       every test; test_pitched_operands_and_output
     lda = K + 8, ldb = K + 16 through cm3p_gemm_bf16 directly
  6  data at full significand width, residual / bias adds bit for bit;       every test; test_random_data_within_the_derived_bound
     one random-data check per kernel and layout at a derived bound
  7  the RoPE epilogue per kernel (which side of the bf16 rounding), S < 256, test_rope_epilogue_against_its_kernels_specification
     a sequence end inside a tile, per_batch, a ragged last row tile, q_scale
  8  gemm256_kernel: every case above under CM3P_GEMM_IMPL=256, and by       all of the above; test_forward_edge_tiles[...edge_mod4...]
     default at M % 8 = N % 8 = 4
  -  the GeGLU epilogue against float64 and the two-kernel chain             test_geglu_epilogue_against_float64_and_the_two_kernel_chain

Notes on the shapes: the big path needs ceil(M / 256) ceil(N / 256) splits >= 200, hence tall-thin shapes at short K.  The (0, 1)
layout runs at K = 192 and at K = 128 (its REBAL instance); the edge cases also run under gemm8p_set_grid(64); N = 264 and 520 take
M = 25600 and 17152 to keep 200 tiles; the
M % 8 = N % 8 = 4 case cannot take CM3P_EPI_BF16_RESID (the entry point asks for N % 8 = 0).  That case exposed a defect of
gemm256_kernel's bf16 store (16 bytes at a row's last four columns), fixed in csrc/gemm256.hip.  The float64 reference is a CPU
matmul of at most 13 GFLOP everywhere but in test_linear_wgrad_reaches_the_big_kernel_by_the_librarys_own_split.  That shape is
the smallest that cm3p_gemm_wgrad_splits sends to the big kernels just above T = 8192 - it allows T / 2048 = 4 splits, so 50 tiles
are needed - and its reference is 39 GFLOP, the one case here above 10 GFLOP by a wide margin; it takes the device's torch.float64
matmul: on exact data every correct float64 matmul returns the same integers.
The REBAL cases of test_wgrad_split_k_with_a_short_last_split (items of 4 and 2 k-tiles under k-strided operands) sit where the
ring's early B-lo read had the least time between the LDS-DMA and the read; csrc/gemm8p.hip now retires that half-tile with a
counted wait of its own (phase 3, vmcnt(10)).
The (32768, 776, 264) case of tests/test_kernels_gpu.py::test_gemm256_wgrad_layout keeps its name and shape: it does reach the ring
(cm3p_gemm_wgrad_splits answers 49 through its 128 x 128 branch, cm3p_gemm_bf16 makes that 43 splits, and 8 tiles x 43 pass the
threshold); that test now asserts so.  The RoPE and GeGLU checks print a largest err / bound close to 1: over millions of
elements a correctly rounded bf16 result comes arbitrarily close to half an ulp, which is the bound's leading term.
"""
import functools
import os

import pytest
import torch

import gemm_refs as G
import row_kernel_refs as R
from row_kernel_refs import bits_equal, check, gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
IMPLS = [None, "256", "128"]
FRONT, BACK = 64, 256  # guard rows before and past the matrix
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}  # NaN patterns
CHUNK = 8192  # rows per float64 reference chunk of the bounded checks


@pytest.fixture(scope="module")
def K():
    """The kernels module; the CPU references of this module run on 16 threads at most (restored afterwards)."""
    from cm3p_amd import kernels

    assert kernels.SOFTMAX_Q_SCALE == G.SOFTMAX_Q_SCALE
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield kernels
    torch.set_num_threads(threads)


def _set_impl(monkeypatch, impl):
    """CM3P_GEMM_IMPL is read by the library on every call."""
    if impl is None:
        monkeypatch.delenv("CM3P_GEMM_IMPL", raising=False)
    else:
        monkeypatch.setenv("CM3P_GEMM_IMPL", impl)


class Guarded:
    """An [M, N] output of pitch ldc inside a sentinel-filled buffer."""

    def __init__(self, M, N, dtype, ldc=None):
        self.M, self.N, self.ldc = M, N, N if ldc is None else ldc
        self.ity, self.sent = SENTINEL[dtype]
        self.buf = torch.empty((FRONT + M + BACK, self.ldc), dtype=dtype, device=DEV)
        self.buf.view(self.ity).fill_(self.sent)

    @property
    def out(self):
        """What the kernel is handed: the contiguous [M, N] rows (ldc = N), else the flat buffer from the matrix's first element on."""
        if self.ldc == self.N:
            return self.buf[FRONT:FRONT + self.M]
        return self.buf.view(-1)[FRONT * self.ldc:]

    def result(self):
        return self.buf[FRONT:FRONT + self.M, :self.N]

    def assert_intact(self, what):
        b = self.buf.view(self.ity)
        hit = [int((r != self.sent).sum()) for r in (b[:FRONT], b[FRONT + self.M:], b[FRONT:FRONT + self.M, self.N:])]
        assert hit == [0, 0, 0], f"{what}: stores outside the {self.M} x {self.N} matrix: {hit[0]} elements in the rows before it, " \
                                 f"{hit[1]} in the rows past it, {hit[2]} in the columns past N"


def _bits(got, want, what):
    """Bit equality on the device; the host comparison only words the failure."""
    got, want = got.contiguous(), want.to(DEV)
    ity = SENTINEL[got.dtype][0]
    if got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.view(ity), want.view(ity)):
        print(f"{what}: bits equal ({got.numel()} elements)")
        return
    bits_equal(got, want, what)


def _grids(case, impl):
    """Workgroup counts to run at: the default, and for the ring 64 workgroups (3 to 4 work items each at 200 to 204 items)."""
    return (0, 64) if case.tag(0, impl).startswith(G.RING) else (0,)


def _assert_tag(K, case, epi, impl, what):
    """The hand table against the library's own route for this call (K._gemm_tag formats cm3p_gemm_route's answer)."""
    tag = K._gemm_tag(case.M, case.N, case.K, case.a_kc, case.b_kc, epi, case.split_k)
    assert tag == case.tag(epi, impl), f"{what}: lands on {tag}, the case table says {case.tag(epi, impl)}"


# ================================================================================================ plain epilogues on exact data
@functools.lru_cache(maxsize=2)
def _plain(case):
    """Operands, residuals and the expected bits of every plain epilogue of one case, on the device (shared by its three kernels)."""
    g = gen("gemm", case.name)
    a, b = G.exact_operand(case.M, case.K, g), G.exact_operand(case.N, case.K, g)
    acc = G.acc64(a, b)
    r32, r16, bias = G.residuals(case.M, case.N, acc, g)
    refs = {e: t.to(DEV) for e, t in G.epilogue_refs(acc, r32, r16, bias).items()}
    return dict(a=G.stored(a, case.a_kc).to(torch.bfloat16).to(DEV), b=G.stored(b, case.b_kc).to(torch.bfloat16).to(DEV),
                resid={G.EPI_F32_RESID: r32.to(DEV), G.EPI_F32_BIAS: bias.to(DEV), G.EPI_BF16_RESID: r16.to(DEV)}, refs=refs)


def _run_plain(K, case, impl, epilogues=None):
    d = _plain(case)
    grids = _grids(case, impl)
    try:
        for grid in grids:
            K.gemm8p_set_grid(grid)
            assert K.gemm8p_get_grid() == grid
            for epi in (epilogues or case.epilogues()):
                dtype = torch.bfloat16 if epi in (G.EPI_BF16, G.EPI_BF16_RESID) else torch.float32
                for alias in ((False, True) if epi == G.EPI_BF16_RESID else (False,)):
                    what = f"{case.name} impl {impl} grid {grid} epilogue {epi}{' in place' if alias else ''}"
                    _assert_tag(K, case, epi, impl, what)
                    gd = Guarded(case.M, case.N, dtype)
                    resid = d["resid"].get(epi)
                    if alias:  # C aliases R
                        gd.out.copy_(resid)
                        resid = gd.out
                    K.gemm(d["a"], d["b"], case.M, case.N, case.K, case.a_kc, case.b_kc, epi, resid=resid, out=gd.out, split_k=case.split_k)
                    _bits(gd.result(), d["refs"][epi], what)
                    gd.assert_intact(what)
    finally:
        K.gemm8p_set_grid(0)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", G.FORWARD, ids=lambda c: c.name)
def test_forward_every_epilogue_at_one_to_five_k_tiles(K, monkeypatch, case, impl):
    """M = 51200, N = 256: 200 work items.  At the default grid every workgroup has one item and the ring's stream passes its end
    inside the prologue (K = 64) or the first k-tiles; under gemm8p_set_grid(64) a workgroup walks 3 to 4 items and the stream crosses
    an item boundary every 1 to 5 k-tiles, the ring parity flipping between items at odd counts.  All five plain epilogues,
    CM3P_EPI_BF16_RESID with C apart from R and in place."""
    _set_impl(monkeypatch, impl)
    _run_plain(K, case, impl)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", G.EDGES, ids=lambda c: c.name)
def test_forward_edge_tiles(K, monkeypatch, case, impl):
    """Row remainders 8, 64, 136, 248, column remainders 8, 72, 248 and 8 past one and two full tiles, both ragged, and
    M % 8 = N % 8 = 4 (gemm256_kernel by default: its last 8-column chunk of a row holds 4 columns), at one and three k-tiles."""
    _set_impl(monkeypatch, impl)
    _run_plain(K, case, impl)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", G.DGRAD + G.KS_A, ids=lambda c: c.name)
def test_k_strided_operands_with_ragged_tiles(K, monkeypatch, case, impl):
    """dgrad (1, 0): B stored [K][N] with 8 and 72 columns in its last tile (Operand<false>::setup clamps each lane at extent - 8);
    (0, 1): A stored [K][M] with 72 rows in its last tile.  Every epilogue the layout takes."""
    _set_impl(monkeypatch, impl)
    _run_plain(K, case, impl)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", G.WGRAD, ids=lambda c: c.name)
def test_wgrad_split_k_with_a_short_last_split(K, monkeypatch, case, impl):
    """wgrad (0, 0) on 2 x 3 ragged tiles, 34 k-splits (204 work items): all splits 2 k-tiles; splits of 4 with a last one of 2; splits
    of 2 with a last one of 1 (the plain instance, nk mixed within the launch).  Partials and the ordered reduce are exact on this
    data: the bits of fp32(acc).  K.gemm allocates the workspace for the requested split count, the library recomputes the count."""
    _set_impl(monkeypatch, impl)
    assert G.kchunk_of(case.K, case.split_k)[1] == case.split_k
    _run_plain(K, case, impl)


@pytest.mark.parametrize("impl", IMPLS)
def test_linear_wgrad_reaches_the_big_kernel_by_the_librarys_own_split(K, monkeypatch, impl):
    """K.linear_wgrad of dy [8256, 1032], x [8256, 2312]: cm3p_gemm_wgrad_splits answers 4 (50 tiles x 4 = 200 items of 33 k-tiles, the
    last split 30: the plain instance).  The reference is the device's float64 matmul (see the module docstring)."""
    _set_impl(monkeypatch, impl)
    case = G.LINEAR_WGRAD
    assert K._wgrad_splits(case.M, case.N, case.K) == case.split_k
    _assert_tag(K, case, G.EPI_F32, impl, case.name)
    g = gen("gemm", case.name)
    dy = G.exact_operand(case.M, case.K, g).t().contiguous().to(DEV)  # stored [T, N]
    x = G.exact_operand(case.N, case.K, g).t().contiguous().to(DEV)
    want = (dy.double().t() @ x.double())
    assert float(want.abs().max()) < 2.0 ** 24 * 2.0 ** 6 and torch.equal(want.float().double(), want)
    got = K.linear_wgrad(dy.to(torch.bfloat16), x.to(torch.bfloat16))
    _bits(got, want.float(), f"{case.name} impl {impl}")
    gd = Guarded(case.M, case.N, torch.float32)
    K.gemm(dy.to(torch.bfloat16), x.to(torch.bfloat16), case.M, case.N, case.K, False, False, G.EPI_F32, out=gd.out, split_k=case.split_k)
    _bits(gd.result(), want.float(), f"{case.name} impl {impl} guarded")
    gd.assert_intact(case.name)


@pytest.mark.parametrize("case", G.SMALL_CASES, ids=lambda c: c.name)
def test_small_kernel_natively(K, monkeypatch, case):
    """The 128 x 128 kernel below the 200-tile threshold: the older tests' edge shapes with the new data, N % 8 = 4, the four
    layouts ((0, 1) among them), and split-K whose last split ends inside a k-tile."""
    _set_impl(monkeypatch, None)
    _run_plain(K, case, None)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", G.PITCHED, ids=lambda c: c.name)
def test_pitched_operands_and_output(K, monkeypatch, case, impl):
    """lda = K + 8, ldb = K + 16, ldc = N + 8 through cm3p_gemm_bf16 directly (argument order of K.gemm); the residual has C's pitch.
    The pad columns of A and B hold NaN: reading them shows in the result.  The output's pad columns must keep the sentinel."""
    from cm3p_amd import _lib

    _set_impl(monkeypatch, impl)
    M, N, Kd = case.M, case.N, case.K
    lda, ldb, ldc = Kd + 8, Kd + 16, N + 8
    g = gen("gemm", case.name)
    a, b = G.exact_operand(M, Kd, g), G.exact_operand(N, Kd, g)
    acc = G.acc64(a, b)
    r32, r16, bias = G.residuals(M, N, acc, g)
    refs = G.epilogue_refs(acc, r32, r16, bias)

    def pitched(x, ld, dtype):
        buf = torch.full((x.shape[0], ld), float("nan"), dtype=dtype, device=DEV)
        buf[:, :x.shape[1]] = x.to(dtype).to(DEV)
        return buf

    ad, bd = pitched(a, lda, torch.bfloat16), pitched(b, ldb, torch.bfloat16)
    resid = {G.EPI_F32_RESID: pitched(r32, ldc, torch.float32), G.EPI_F32_BIAS: bias.to(DEV), G.EPI_BF16_RESID: pitched(r16, ldc, torch.bfloat16)}
    try:
        for grid in _grids(case, impl):
            K.gemm8p_set_grid(grid)
            for epi in case.epilogues():
                what = f"{case.name} impl {impl} grid {grid} epilogue {epi}"
                _assert_tag(K, case, epi, impl, what)
                gd = Guarded(M, N, torch.bfloat16 if epi in (G.EPI_BF16, G.EPI_BF16_RESID) else torch.float32, ldc)
                _lib.call("cm3p_gemm_bf16", _lib.ptr(ad), _lib.ptr(bd), _lib.ptr(gd.out), _lib.ptr(resid.get(epi)), M, N, Kd, lda, ldb, ldc,
                          1, 1, epi, 1, None, _lib.stream())
                _bits(gd.result(), refs[epi], what)
                gd.assert_intact(what)
    finally:
        K.gemm8p_set_grid(0)


# ================================================================================================ random data
@functools.lru_cache(maxsize=1)
def _random():
    """One logical A [17160, 768], B [520, 768] of bf16 normal data for every layout and kernel, its float64 product and bound."""
    g = gen("gemm", "random")
    c = G.RANDOM[0]
    a, b = G.random_operand(c.M, c.K, g), G.random_operand(c.N, c.K, g)
    return a, b, G.acc64(a, b), G.random_bound(a, b)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", G.RANDOM, ids=lambda c: c.name)
def test_random_data_within_the_derived_bound(K, monkeypatch, case, impl):
    """bf16 normal data at K = 768, fp32 output, per element within 2 K u sum_k |a_k b_k| (G.random_bound) - one check per kernel
    and layout."""
    _set_impl(monkeypatch, impl)
    a, b, ref, bound = _random()
    _assert_tag(K, case, G.EPI_F32, impl, case.name)
    gd = Guarded(case.M, case.N, torch.float32)
    K.gemm(G.stored(a, case.a_kc).to(torch.bfloat16).to(DEV), G.stored(b, case.b_kc).to(torch.bfloat16).to(DEV), case.M, case.N, case.K,
           case.a_kc, case.b_kc, G.EPI_F32, out=gd.out)
    check(gd.result(), ref, bound, f"{case.name} impl {impl}")
    gd.assert_intact(case.name)


# ================================================================================================ RoPE epilogue
@functools.lru_cache(maxsize=2)
def _rope_operands(S, B):
    case = G.rope_case(S, B)
    g = gen("gemm", case.name)
    x, w = G.exact_operand(case.M, case.K, g), G.exact_operand(case.N, case.K, g)
    return x.to(torch.bfloat16).to(DEV), w.to(torch.bfloat16).to(DEV), G.acc64(x, w)


ROPE_PARAMS = [(S, B, impl) for S, B in G.ROPE_BIG for impl in IMPLS] + [(S, B, None) for S, B in G.ROPE_SMALL]


@pytest.mark.parametrize("per_batch", [False, True])
@pytest.mark.parametrize("S,B,impl", ROPE_PARAMS)
def test_rope_epilogue_against_its_kernels_specification(K, monkeypatch, S, B, impl, per_batch):
    """cm3p_qkv_gemm_rope at nh = 2, K = 64 against G.rope_ref: the 256 x 256 kernels rotate the bf16-ROUNDED projection, the
    128 x 128 kernel the fp32 accumulator (the two are told apart on this data, tests/test_gemm_refs_host.py).  S = 200: the ring's
    modulo branch; S = 300: a sequence end inside tiles and a last row tile of 200 rows; per_batch: a table row per token; q_scale 1
    and SOFTMAX_Q_SCALE, on edge tiles too.  cos / sin are cm3p_rope_table's own output.  The v third is RNE_bf16(acc) exactly."""
    from cm3p_amd import _lib

    _set_impl(monkeypatch, impl)
    case = G.rope_case(S, B)
    T, N, Kd, nh = case.M, case.N, case.K, G.ROPE_NH
    x, w, acc = _rope_operands(S, B)
    assert (2 * N // 3) % 256 == 0
    tag = K._gemm_tag(T, N, Kd, True, True, G.EPI_ROPE, 1, rope_cols=2 * N // 3)  # (the tag expression of K.qkv_linear_rope)
    assert tag == case.tag(G.EPI_ROPE, impl), (tag, case.tag(G.EPI_ROPE, impl))
    small = tag.startswith(G.SMALL)
    pos = G.rope_positions(S, B, per_batch)
    cos, sin = K.rope_table(pos.to(DEV), R.rope_inv_freq(10000.0, 64).to(DEV))
    cos64, sin64 = cos.cpu().double(), sin.cpu().double()
    try:
        for grid in _grids(case, impl):
            K.gemm8p_set_grid(grid)
            for q_scale in (1.0, G.SOFTMAX_Q_SCALE):
                what = f"{case.name} impl {impl} grid {grid} per_batch {per_batch} q_scale {q_scale:.4g}"
                gd = Guarded(T, N, torch.bfloat16)
                _lib.call("cm3p_qkv_gemm_rope", _lib.ptr(x), _lib.ptr(w), _lib.ptr(gd.out), T, N, Kd, _lib.ptr(cos, torch.float32),
                          _lib.ptr(sin, torch.float32), S, int(per_batch), 2 * N // 3, float(q_scale), _lib.stream())
                got = gd.result().cpu()
                gd.assert_intact(what)
                for r0 in range(0, T, CHUNK):
                    s = slice(r0, r0 + CHUNK)
                    # (positions of a chunk: the table rows of tokens r0.. - rope_ref indexes rows from 0, so hand it the tokens' rows)
                    rows = torch.arange(r0, min(T, r0 + CHUNK))
                    prow = rows if per_batch else rows % S
                    ref, bound = G.rope_ref(acc[s], cos64[prow], sin64[prow], S, True, q_scale, nh, small)
                    check(got[s], ref, bound, f"{what} rows {r0}+")
    finally:
        K.gemm8p_set_grid(0)


# ================================================================================================ GeGLU epilogue
@pytest.mark.parametrize("T,I,Kd", G.GEGLU)
def test_geglu_epilogue_against_float64_and_the_two_kernel_chain(K, T, I, Kd, monkeypatch):
    """cm3p_gemm_geglu (the ring only) on exact data scaled so that h sits inside [-6, 6] (G.geglu_exps): h = K.linear_fwd is
    RNE_bf16(acc) bit for bit, the fused result equals K.geglu_fwd(h) bit for bit at the default grid and at 3 to 13 items per
    workgroup, and lies within R.geglu_fwd_ref's bound of the float64 GeGLU of those rows."""
    from cm3p_amd import _lib

    _set_impl(monkeypatch, None)
    assert K.gemm_geglu_supported(T, I, Kd)
    rebal = "true" if (Kd // 64) % 2 == 0 else "false"  # (the instance in K.gemm_geglu's tag)
    assert K._gemm_tag(T, 2 * I, Kd, True, True, G.EPI_GEGLU, 1, kernel=K._GEMM_RING) == f"{G.RING}<true, true, {G.EPI_GEGLU}, {rebal}>"
    g = gen("gemm", "geglu", T, I, Kd)
    ea, eb = G.geglu_exps(Kd)
    x, wi = G.exact_operand(T, Kd, g, exps=ea), G.exact_operand(2 * I, Kd, g, exps=eb)
    xd, wd = x.to(torch.bfloat16).to(DEV), wi.to(torch.bfloat16).to(DEV)
    w_il = wd[K.geglu_interleave_index(I, DEV)].contiguous()
    assert torch.equal(K.geglu_interleave_index(I, DEV).cpu(), G.geglu_interleave_index(I))
    acc = G.acc64(x, wi)
    print(f"geglu {T} {I} {Kd}: {float((acc.abs() <= 6).double().mean()):.4f} of h inside [-6, 6]")
    h = K.linear_fwd(xd, wd)
    _bits(h, acc.float().to(torch.bfloat16), f"geglu {T} {I} {Kd}: h")
    two = K.geglu_fwd(h)
    try:
        for grid in (0, 64):
            K.gemm8p_set_grid(grid)
            gd = Guarded(T, I, torch.bfloat16)
            _lib.call("cm3p_gemm_geglu", _lib.ptr(xd), _lib.ptr(w_il), _lib.ptr(gd.out), T, I, Kd, _lib.stream())
            _bits(gd.result(), two, f"geglu {T} {I} {Kd} grid {grid}: fused == two kernels")
            gd.assert_intact(f"geglu {T} {I} {Kd} grid {grid}")
    finally:
        K.gemm8p_set_grid(0)
    got = two.cpu()
    for r0 in range(0, T, CHUNK):
        s = slice(r0, r0 + CHUNK)
        ref, bound = G.geglu_ref(acc[s])
        check(got[s], ref, bound, f"geglu {T} {I} {Kd} rows {r0}+")
