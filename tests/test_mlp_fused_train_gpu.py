"""GeGLU of a training step in the store phases of its two neighbouring GEMMs (csrc/gemm8p.hip): CM3P_EPI_BF16_GEGLU_FWD - the Wi
GEMM stores h' (h with interleaved columns) and a = geglu_fwd(h) - and CM3P_EPI_BF16_GEGLU_BWD - the Wo2 input gradient turns its
bf16-rounded dg and h' into the canonical dh and never writes dg.  Both must give the bits of the two-kernel chains
(K.linear_fwd + K.geglu_fwd, K.linear_dgrad + K.geglu_bwd), and a training step that takes the pair (the default where the library's
route names the ring for both calls) must give the loss, the output and every gradient of the step that does not
(CM3P_GEGLU_FUSED=0).

Kernel level.  The shapes are the smallest the ring takes: the row count is found by asking cm3p_gemm_route (no restatement of the
rule).  Cases: full tiles (I = 256: N = 512 forward, 256 backward); a ragged last row tile (T % 256 = 8); a partly empty last
column tile (I = 1152: the backward's N is 4.5 tiles; I = 96: both calls); an odd k-tile count (K = 192, the plain instance) and
even ones (K = 128, REBAL); the default grid and 3 to 13 work items per workgroup (gemm8p_set_grid 64 and 16 at 200 to 207 items).
Outputs lie in sentinel-filled buffers (guard rows before and after).  a and dh are also held to the float64 bounds of
tests/row_kernel_refs.py (geglu_fwd_ref, geglu_bwd_ref), whose inputs are the bf16 h and dg of the two-kernel chain.

Layer level.  One two-layer step of a default-width tower (768 / 1152; layer 0 global, layer 1 band) at the smallest token count
B x S, S <= 512, that the route accepts for both calls (the backward call, N = I, needs the most rows): fp32 stream, gradient
checkpointing, bf16 training stream; and with an MLP dropout plan the profiler tags show the two-kernel path.
"""
import os

import pytest
import torch

import row_kernel_refs as R
from row_kernel_refs import check, gen
from test_gemm_kernels_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
CHUNK = 8192  # rows per float64 reference chunk
RING, REBAL_BIT = 2, 4
# (I, K of the call, T % 256): the docstring's cases
CASES = [(256, 128, 0), (1152, 192, 8), (96, 128, 8), (96, 192, 0)]
GRIDS = (0, 64, 16)


@pytest.fixture(scope="module")
def K():
    from cm3p_amd import kernels

    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield kernels
    kernels.gemm8p_set_grid(0)
    torch.set_num_threads(threads)


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    monkeypatch.delenv("CM3P_GEMM_IMPL", raising=False)
    monkeypatch.delenv("CM3P_GEGLU_FUSED", raising=False)


def _route(N, Kd, epi, T):
    from cm3p_amd import _lib

    return _lib.query("cm3p_gemm_route", T, N, Kd, Kd, Kd, 1, 1, epi, 1, 0, 0)


def _smallest_rows(N, Kd, epi, rem):
    """Smallest T with T % 256 == rem that the library's route sends to the ring for this call."""
    for tiles in range(1, 4096):
        T = tiles * 256 + rem - (256 if rem else 0)
        if T > 0:
            code = _route(N, Kd, epi, T)
            if code >= 0:
                assert code & 3 == RING
                return T, code
    raise AssertionError("no ring shape found")


def _same_bits(got, want, what):
    assert got.dtype == want.dtype == BF and got.shape == want.shape, what
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), what


def _operand(rows, cols, g, scale):
    return (torch.randn(rows, cols, generator=g) * scale).to(BF).to(DEV)


@pytest.mark.parametrize("I,Kd,rem", CASES)
def test_wi_gemm_stores_interleaved_h_and_a_in_one_launch(K, I, Kd, rem):
    from cm3p_amd import _lib

    T, code = _smallest_rows(2 * I, Kd, _lib.EPI_BF16_GEGLU_FWD, rem)
    assert bool(code & REBAL_BIT) == ((Kd // 64) % 2 == 0) and T % 256 == rem
    assert _route(2 * I, Kd, _lib.EPI_BF16_GEGLU_FWD, T - 256) < 0  # (one row tile fewer: refused, never another kernel)
    g = gen("mlp_fused", "fwd", I, Kd, rem)
    x, wi = _operand(T, Kd, g, 1.0), _operand(2 * I, Kd, g, 2.0 / Kd ** 0.5)  # h ~ N(0, 2^2): both tails of Phi
    idx = K.geglu_interleave_index(I, DEV)
    w_il = wi[idx].contiguous()
    h = K.linear_fwd(x, wi)
    a = K.geglu_fwd(h)
    want_h = h[:, idx].contiguous()
    for grid in GRIDS:
        K.gemm8p_set_grid(grid)
        hg, ag = Guarded(T, 2 * I, BF), Guarded(T, I, BF)
        _lib.call("cm3p_gemm_bf16", _lib.ptr(x), _lib.ptr(w_il), _lib.ptr(hg.out), None, T, 2 * I, Kd, Kd, Kd, 2 * I, 1, 1,
                  _lib.EPI_BF16_GEGLU_FWD, 1, _lib.ptr(ag.out), _lib.stream())
        _same_bits(hg.result(), want_h, f"fwd {I} {Kd} {T} grid {grid}: h' == h[:, interleave]")
        _same_bits(ag.result(), a, f"fwd {I} {Kd} {T} grid {grid}: a == geglu_fwd(h)")
        hg.assert_intact(f"fwd h' {I} {Kd} {T} grid {grid}")
        ag.assert_intact(f"fwd a {I} {Kd} {T} grid {grid}")
    K.gemm8p_set_grid(0)
    h2, a2 = K.linear_geglu_fwd(x, w_il)  # the wrapper the encoder calls
    _same_bits(h2, want_h, "linear_geglu_fwd h'")
    _same_bits(a2, a, "linear_geglu_fwd a")
    hc, ac = h.cpu(), a.cpu()
    for r0 in range(0, T, CHUNK):
        ref, bound = R.geglu_fwd_ref(hc[r0:r0 + CHUNK].double())
        check(ac[r0:r0 + CHUNK], ref, bound, f"fwd {I} {Kd} rows {r0}+: a against float64")


@pytest.mark.parametrize("I,Kd,rem", CASES)
def test_wo2_dgrad_does_the_geglu_backward_in_its_store_phase(K, I, Kd, rem):
    from cm3p_amd import _lib

    T, code = _smallest_rows(I, Kd, _lib.EPI_BF16_GEGLU_BWD, rem)
    assert bool(code & REBAL_BIT) == ((Kd // 64) % 2 == 0) and T % 256 == rem
    assert _route(I, Kd, _lib.EPI_BF16_GEGLU_BWD, T - 256) < 0
    g = gen("mlp_fused", "bwd", I, Kd, rem)
    dy, wo2 = _operand(T, Kd, g, 1.0), _operand(Kd, I, g, 1.0 / Kd ** 0.5)  # Wo2 [H, I]; dg ~ N(0, 1)
    h = R.geglu_h(T, I, g).to(DEV)
    idx = K.geglu_interleave_index(I, DEV)
    h_il = h[:, idx].contiguous()
    wo2_t = wo2.t().contiguous()
    dg = K.linear_dgrad(dy, wo2, wo2_t)
    want = K.geglu_bwd(dg, h)
    for grid in GRIDS:
        K.gemm8p_set_grid(grid)
        out = Guarded(T, 2 * I, BF)
        _lib.call("cm3p_gemm_bf16", _lib.ptr(dy), _lib.ptr(wo2_t), _lib.ptr(out.out), _lib.ptr(h_il), T, I, Kd, Kd, Kd, 2 * I, 1, 1,
                  _lib.EPI_BF16_GEGLU_BWD, 1, None, _lib.stream())
        _same_bits(out.result(), want, f"bwd {I} {Kd} {T} grid {grid}: dh == geglu_bwd(linear_dgrad, h)")
        out.assert_intact(f"bwd dh {I} {Kd} {T} grid {grid}")
    K.gemm8p_set_grid(0)
    _same_bits(K.linear_dgrad_geglu_bwd(dy, wo2_t, h_il), want, "linear_dgrad_geglu_bwd")
    dgc, hc, got = dg.cpu(), h.cpu(), want.cpu()
    for r0 in range(0, T, CHUNK):
        s = slice(r0, r0 + CHUNK)
        ref, bound = R.geglu_bwd_ref(dgc[s].double(), hc[s].double())
        check(got[s], ref, bound, f"bwd {I} {Kd} rows {r0}+: dh against float64")


def test_the_weight_cast_writes_wi_in_interleaved_row_order_in_the_same_launch(K):
    """cm3p_cast_f32_bf16_t_multi with a flagged entry: that matrix's bf16 copy has the rows of geglu_interleave_index, its transpose
    and every other matrix are what the unflagged call gives."""
    g = gen("mlp_fused", "cast")
    ws = [torch.randn(r, c, generator=g).to(DEV) for r, c in ((72, 40), (192, 136), (64, 64), (2304, 768))]
    plain = K.cast_bf16_with_transpose_many(ws)
    flagged = K.cast_bf16_with_transpose_many(ws, [False, True, False, True])
    for i, ((y, yt), (fy, fyt)) in enumerate(zip(plain, flagged)):
        _same_bits(fyt, yt, f"matrix {i}: transpose")
        _same_bits(fy, y[K.geglu_interleave_index(y.shape[0] // 2, DEV)] if i in (1, 3) else y, f"matrix {i}: copy")


# ================================================================================================ layer level
def _encoder(**over):
    from cm3p_amd.configuration_cm3p import CM3PBeatmapConfig
    from cm3p_amd.encoder import CM3PEncoder

    torch.manual_seed(7)
    cfg = CM3PBeatmapConfig(num_hidden_layers=2, global_attn_every_n_layers=2, **over)
    assert (cfg.hidden_size, cfg.intermediate_size) == (768, 1152) and cfg.is_global_layer(0) and not cfg.is_global_layer(1)
    enc = CM3PEncoder(cfg).to(DEV).train()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen("mlp_fused", "param", n)) * (0.02 if p.dim() == 2 else 0.1) + (1.0 if "norm" in n else 0.0))
    return enc


def _tokens(K):
    """Smallest B x S (S <= 512) the route accepts for both calls of the default-width MLP."""
    from cm3p_amd import _lib

    T0 = max(_smallest_rows(2304, 768, _lib.EPI_BF16_GEGLU_FWD, 8)[0], _smallest_rows(1152, 768, _lib.EPI_BF16_GEGLU_BWD, 8)[0])
    for T in range(T0, T0 + 4096, 8):
        for S in range(512, 127, -1):
            if T % S == 0 and K.mlp_geglu_fused_supported(T, 1152, 768):
                return T // S, S
    raise AssertionError("no token count found")


def _step(enc, ids, gy, monkeypatch, fused):
    from cm3p_amd import _lib

    if fused:
        monkeypatch.delenv("CM3P_GEGLU_FUSED", raising=False)
    else:
        monkeypatch.setenv("CM3P_GEGLU_FUSED", "0")
    enc.zero_grad(set_to_none=True)
    _lib.profile_begin()
    try:
        y = enc(input_ids=ids)
        loss = (y.float() * gy.view(y.shape)).sum()
        loss.backward()
    finally:
        tags = _lib.profile_end()
    return loss.detach(), y.detach(), {n: p.grad.clone() for n, p in enc.named_parameters()}, tags


FWD_TAG, BWD_TAG = "gemm8p_kernel<true, true, 9,", "gemm8p_kernel<true, true, 10,"  # (_lib.EPI_BF16_GEGLU_FWD / _BWD instances)


def _is_fused_tag(tag):
    return tag.startswith(FWD_TAG) or tag.startswith(BWD_TAG)


@pytest.fixture(scope="module")
def step_inputs(K):
    B, S = _tokens(K)
    g = gen("mlp_fused", "layer")
    ids = torch.randint(5, 3000, (B, S), generator=g).to(DEV)
    gy = torch.randn(B * S, 768, generator=g).to(DEV)
    return ids, gy


@pytest.mark.parametrize("mode", ["fp32_stream", "checkpointing", "bf16_stream"])
def test_training_step_with_the_fused_pair_equals_the_two_kernel_step(K, step_inputs, monkeypatch, mode):
    ids, gy = step_inputs
    enc = _encoder()
    if mode == "checkpointing":
        enc.gradient_checkpointing = True
    if mode == "bf16_stream":
        enc.train_residual_dtype = BF
    l1, y1, g1, tags1 = _step(enc, ids, gy, monkeypatch, fused=True)
    l0, y0, g0, tags0 = _step(enc, ids, gy, monkeypatch, fused=False)
    # which path ran: two layers, each with one forward launch (two with checkpointing: the recompute) and one backward launch
    n_fwd = 4 if mode == "checkpointing" else 2
    assert sorted(n for t, (n, _, _) in tags1.items() if _is_fused_tag(t)) == sorted([n_fwd, 2]), tags1.keys()
    assert "cm3p_geglu_fwd" not in tags1 and "cm3p_geglu_bwd" not in tags1
    assert not any(_is_fused_tag(t) for t in tags0) and tags0["cm3p_geglu_fwd"][0] == n_fwd and tags0["cm3p_geglu_bwd"][0] == 2
    for t, (n, _, work) in tags1.items():
        if _is_fused_tag(t):
            N = 2304 if t.startswith(FWD_TAG) else 1152
            assert work == n * 2.0 * ids.numel() * N * 768, t
    assert y1.dtype == (BF if mode == "bf16_stream" else torch.float32)
    assert torch.equal(l1, l0) and torch.equal(y1, y0)
    assert g1.keys() == g0.keys() and len(g1) == len(list(enc.parameters()))
    for n in g1:
        assert torch.isfinite(g1[n]).all() and g1[n].abs().max() > 0, n
        assert torch.equal(g1[n], g0[n]), n


def test_an_mlp_dropout_plan_keeps_the_two_kernel_path(K, step_inputs, monkeypatch):
    ids, gy = step_inputs
    enc = _encoder(mlp_dropout=0.1)
    torch.manual_seed(11)
    _, _, grads, tags = _step(enc, ids, gy, monkeypatch, fused=True)
    assert not any(_is_fused_tag(t) for t in tags), tags.keys()
    assert all(torch.isfinite(v).all() for v in grads.values())
    assert tags["cm3p_geglu_fwd_dropout"][0] == 2 and tags["cm3p_geglu_bwd_dropout"][0] == 2
