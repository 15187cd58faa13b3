"""Kernel-level specifications of the encoder's HBM-bound row kernels - LayerNorm, embedding + LayerNorm, GeGLU, RoPE, pooling and
the row gather / scatter - each against a float64 CPU reference of the same operation, at every template instance, every dtype
form and past every grid cap.

Conventions (as tests/test_conv_head_kernels_gpu.py, whose _check / _bits_equal / _gen are reused through row_kernel_refs): bf16
inputs are rounded once and the same values go to both sides; every check is per element, |got - ref| <= bound; the references and
the bounds with their derivations live in tests/row_kernel_refs.py, where tests/test_row_kernel_bounds_host.py shows without a GPU
that each bound is attainable (a torch fp32 walk of the kernel's addition path passes) and sharp (a wrong evaluation fails).  Each
check prints its largest err / bound (`pytest -rP`).

What the suite did not execute or look at before, and the test that does now:

  1  LayerNorm NC = 4, partly filled last chunks, H = 4          test_layernorm_forward_every_instance_and_output_form
  2  dx_bf16, bf16 x, bf16-only y, stats off, in-place == not    test_layernorm_forward_..., test_layernorm_backward_every_form
  3  large-mean, constant, zero and outlier rows                 test_layernorm_forward_on_rows_that_break_a_careless_variance,
                                                                 test_layernorm_backward_every_form (special rows included)
  4  embedding dtype instances, bf16-only y, y past the grid     test_embed_ln_forward_is_layernorm_of_the_gathered_rows,
                                                                 test_embed_ln_backward_against_float64_autograd
  5  audio_slots' carry, 16 wave offsets, mid-wave tile end      test_audio_slots_is_the_exclusive_cumsum
  6  GegluWalk's stride, carry and ragged last trip              test_geglu_against_float64, test_gelu_element_kernels_past_the_grid
  7  RoPE tables at large positions, apply past the grid,        test_rope_table_is_cos_sin_of_the_fp32_product,
     the inverse on its own, head_dim 16 / 32                    test_rope_apply_against_the_float64_rotation
  8  pooling H > 1024, S around one chunk, scattered masks       test_pooling_against_float64
  9  row moves past the grid cap, bf16 rows, no rows             test_gather_and_scatter_rows_bit_for_bit

Cases that the issue lists and that duplicate another path: none dropped.  The LayerNorm backward with only a bf16 dx (dx_f32 null)
has no caller and no wrapper form and is not exercised.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import row_kernel_refs as R
from row_kernel_refs import FTZ, LN_EPS, U, bits_equal, check, gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 4096  # rows per float64 reference chunk

torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def K():
    from cm3p_amd import kernels

    return kernels


def _rne(t32):
    return t32.to(torch.bfloat16)


def _cpu(*ts):
    return tuple(None if t is None else t.cpu() for t in ts)


# ================================================================================================ A. LayerNorm
LN_H = [4, 64, 252, 256, 260, 512, 768, 772, 1024, 1028, 1536, 1792, 2044, 2048]


def _ln_forward_forms(K, x, w, what):
    """All output forms of one input (x fp32 or bf16 on the host): f32 + bf16 with stats, f32 only, bf16 only without stats, f32 only
    without stats - the same bits wherever two calls produce the same output - then every output against float64."""
    xd, wd = x.to(DEV), w.to(DEV)
    y32, y16, mean, rstd = _cpu(*K.layernorm_fwd(xd, wd, LN_EPS, True, True))
    a32, a16, mean_a, rstd_a = _cpu(*K.layernorm_fwd(xd, wd, LN_EPS, True, False))
    b32, b16, mean_b, rstd_b = _cpu(*K.layernorm_fwd(xd, wd, LN_EPS, False, True, want_stats=False))
    c32, _, mean_c, _ = _cpu(*K.layernorm_fwd(xd, wd, LN_EPS, True, False, want_stats=False))
    assert a16 is None and b32 is None and mean_b is None and rstd_b is None and mean_c is None
    bits_equal(y16, _rne(y32), f"{what}: y_bf16 == RNE(y_f32) of the same call")
    bits_equal(a32, y32, f"{what}: f32-only y")
    bits_equal(b16, y16, f"{what}: bf16-only y, stats off")
    bits_equal(c32, y32, f"{what}: f32-only y, stats off")
    bits_equal(mean_a, mean, f"{what}: mean")
    bits_equal(rstd_a, rstd, f"{what}: rstd")
    worst = 0.0
    for r0 in range(0, x.shape[0], CHUNK):
        s = slice(r0, r0 + CHUNK)
        ref = R.ln_fwd_ref(x[s].double(), w.double())
        worst = max(worst, check(mean[s], ref["mean"], ref["mean_b"], f"{what} mean rows {r0}+"),
                    check(rstd[s], ref["rstd"], ref["rstd_b"], f"{what} rstd rows {r0}+"),
                    check(y32[s], ref["y"], ref["y_b"], f"{what} y_f32 rows {r0}+"),
                    check(y16[s], ref["y"], R.bf16_bound(ref["y"], ref["y_b"]), f"{what} y_bf16 rows {r0}+"))
    return y32, mean, rstd, worst


@pytest.mark.parametrize("H", LN_H)
def test_layernorm_forward_every_instance_and_output_form(K, H):
    """ceil(H / 256) = 1, 2, 3, 4 and 5..8 on the NC = 8 instance; H = 252, 260, 772, 1028, 1536, 2044 leave the last chunk partly
    filled and H = 4 has one live lane.  8193 rows: more than the forward's 2048 blocks x 4 waves."""
    for rows in (1, 3, 5, 8193):
        g = gen("lnf", H, rows)
        x = torch.randn(rows, H, generator=g) * 2 + 0.5
        w = 1 + 0.2 * torch.randn(H, generator=g)
        for xdt in (torch.float32, torch.bfloat16):
            _ln_forward_forms(K, x.to(xdt), w, f"H {H} rows {rows} x {xdt}")


@pytest.mark.parametrize("H", LN_H)
def test_layernorm_forward_on_rows_that_break_a_careless_variance(K, H):
    """R.LN_SPECIAL_ROWS: the bounds are functions of the row (u max|x| against the spread, ln_fwd_ref), so they stay meaningful here:
    a one-pass variance fails them on the large-mean rows (tests/test_row_kernel_bounds_host.py).  The constant rows come out within
    the bound of zero and finite, rstd at most eps^-1/2 (1 + 8u) and below it only by what the variance bound allows; the power-of-two
    constant and the zero row are exact (every partial sum k 2.0 is an fp32 number): y = 0, mean = the constant."""
    g = gen("lns", H)
    x = R.ln_special_rows(H, g)
    w = 1 + 0.2 * torch.randn(H, generator=g)
    for xdt in (torch.float32, torch.bfloat16):
        y32, mean, rstd, _ = _ln_forward_forms(K, x.to(xdt), w, f"special rows H {H} x {xdt}")
        assert torch.isfinite(y32).all() and torch.isfinite(rstd).all()
        assert rstd.double().max().item() <= R.LN_EPS32 ** -0.5 * (1 + 8 * U)
        for r, const in ((3, 2.0), (4, 0.0)):
            assert torch.equal(y32[r], torch.zeros(H)) and mean[r].item() == const, (r, mean[r].item())
            assert abs(rstd[r].double().item() - R.LN_EPS32 ** -0.5) <= 8 * U * R.LN_EPS32 ** -0.5


LN_BWD_CASES = [(H, rows) for H in (260, 768, 1024, 1792) for rows in (1, 5, 4097, "special")]


@pytest.mark.parametrize("H,rows", LN_BWD_CASES)
def test_layernorm_backward_every_form(K, H, rows):
    """dy fp32 / bf16, with and without dres; dx_bf16 is the RNE rounding of the same call's dx_f32; the in-place form (dx written over
    dres, the default) gives the bits of the out-of-place one; dx and dw against float64 at the kernel's own mean / rstd, and once
    at float64 statistics throughout.  4097 rows: more than the backward's 1024 blocks x 4 waves."""
    g = gen("lnb", H, rows)
    x = R.ln_special_rows(H, g) if rows == "special" else torch.randn(rows, H, generator=g) * 2 + 0.5
    n = x.shape[0]
    w = 1 + 0.2 * torch.randn(H, generator=g)
    xd, wd = x.to(DEV), w.to(DEV)
    _, _, mean, rstd = K.layernorm_fwd(xd, wd, LN_EPS, True, False)
    mean_k, rstd_k = mean.cpu().double(), rstd.cpu().double()
    nblk = K.query("cm3p_layernorm_bwd_blocks", n)
    assert nblk == R.ln_bwd_blocks(n)
    c_dw = R.ln_dw_c(n, nblk)
    fwd64 = R.ln_fwd_ref(x.double(), w.double())
    for dyt in (torch.float32, torch.bfloat16):
        dy = torch.randn(n, H, generator=g).to(dyt)
        for use_dres in (False, True):
            what = f"H {H} rows {rows} dy {dyt} dres {use_dres}"
            dres = torch.randn(n, H, generator=g) if use_dres else None
            dx32, dx16, dw = _cpu(*K.layernorm_bwd(dy.to(DEV), xd, wd, mean, rstd, dres.to(DEV) if use_dres else None, True, inplace=False))
            bits_equal(dx16, _rne(dx32), f"{what}: dx_bf16 == RNE(dx_f32) of the same call")
            if use_dres:
                buf = dres.to(DEV)
                i32, i16, iw = K.layernorm_bwd(dy.to(DEV), xd, wd, mean, rstd, buf, True)  # inplace=True is the default
                assert i32.data_ptr() == buf.data_ptr()
                bits_equal(i32, dx32, f"{what}: in place == out of place")
                bits_equal(i16, dx16, f"{what}: in place dx_bf16")
                bits_equal(iw, dw, f"{what}: in place dw")
            ref = R.ln_bwd_ref(dy.double(), x.double(), w.double(), mean_k, rstd_k, dres.double() if use_dres else None)
            check(dx32, ref["dx"], ref["dx_b"], f"{what} dx")
            check(dx16, ref["dx"], R.bf16_bound(ref["dx"], ref["dx_b"]), f"{what} dx_bf16")
            s_abs = ref["p"].abs().sum(0)
            check(dw, ref["p"].sum(0), c_dw * U * s_abs * R.SECOND + FTZ, f"{what} dw (c = {c_dw})")
            if use_dres and dyt == torch.float32:
                r64 = R.ln_bwd_ref(dy.double(), x.double(), w.double(), fwd64["mean"], fwd64["rstd"], dres.double())
                dx_s, p_s = R.ln_bwd_stats_slack(fwd64, r64, dy.double())
                check(dx32, r64["dx"], r64["dx_b"] + dx_s, f"{what} dx, float64 statistics")
                check(dw, r64["p"].sum(0), c_dw * U * r64["p"].abs().sum(0) * R.SECOND + p_s.sum(0) + FTZ, f"{what} dw, float64 statistics")


# ================================================================================================ B. embedding + LayerNorm
EMB_CASES = [(tb, ob, H) for tb in (False, True) for ob in (False, True) for H in (128, 260, 768, 1024)]
EMB_V, EMB_AUDIO = 300, 299


def _embed_case(tab_bf16, ovr_bf16, H):
    """T is not a multiple of 64, and above the forward's 8192 waves at H = 768; the padding id, ids outside the table on both
    sides, audio runs that start at token 0, end at token T - 1 and straddle the 1024-token tile of cm3p_audio_slots."""
    T = 9253 if H == 768 else 1101
    g = gen("emb", tab_bf16, ovr_bf16, H)
    table = torch.randn(EMB_V, H, generator=g)
    ids = torch.randint(0, EMB_AUDIO, (T,), generator=g)
    ids[torch.rand(T, generator=g) < 0.2] = 17
    ids[0:5] = EMB_AUDIO
    ids[1000:1050] = EMB_AUDIO
    ids[T - 3:] = EMB_AUDIO
    ids[7], ids[8], ids[9], ids[10], ids[T // 2] = -3, EMB_V, EMB_V + 1000, 0, 0
    n_audio = int((ids == EMB_AUDIO).sum())
    audio = torch.randn(n_audio, H, generator=g)
    if tab_bf16:
        table = table.to(torch.bfloat16)
    if ovr_bf16:
        audio = audio.to(torch.bfloat16)
    w = 1 + 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(T, H, generator=g)
    return T, ids, table, audio, w, dy


def _gathered_rows(ids, table, audio):
    """The rows the kernel normalises, as fp32 (bf16 values widen exactly): the table row, zeros for ids outside it, the audio rows
    in order at the placeholders."""
    outside = (ids < 0) | (ids >= EMB_V)
    rows = table.float()[ids.clamp(0, EMB_V - 1)]
    rows[outside] = 0.0
    rows[ids == EMB_AUDIO] = audio.float()
    return rows


@pytest.mark.parametrize("tab_bf16,ovr_bf16,H", EMB_CASES)
def test_embed_ln_forward_is_layernorm_of_the_gathered_rows(K, tab_bf16, ovr_bf16, H):
    """The four table / override dtype instances: y (f32 + bf16, f32 only, bf16 only), mean and rstd carry the bits of
    cm3p_layernorm_fwd on the gathered rows (the same row_stats / store_norm), and those rows are within the LayerNorm bounds of
    float64.  At H = 768 the rows past the grid's first trip are looked at, not only their statistics."""
    T, ids, table, audio, w, _ = _embed_case(tab_bf16, ovr_bf16, H)
    idd, td, ad, wd = ids.to(DEV), table.to(DEV), audio.to(DEV), w.to(DEV)
    slot, count = K.audio_slots(idd, EMB_AUDIO)
    assert int(count.item()) == audio.shape[0]
    rows = _gathered_rows(ids, table, audio)
    l32, l16, lmean, lrstd = K.layernorm_fwd(rows.to(DEV), wd, LN_EPS, True, True)
    y32, y16, mean, rstd = K.embed_ln_fwd(idd, td, wd, LN_EPS, slot, ad, want_bf16=True, want_f32=True)
    for got, want, what in ((y32, l32, "y_f32"), (y16, l16, "y_bf16"), (mean, lmean, "mean"), (rstd, lrstd, "rstd")):
        bits_equal(got, want, f"embed_ln {what} == layernorm of the gathered rows")
    a32, a16, amean, _ = K.embed_ln_fwd(idd, td, wd, LN_EPS, slot, ad, want_bf16=False, want_f32=True)
    b32, b16, _, brstd = K.embed_ln_fwd(idd, td, wd, LN_EPS, slot, ad, want_bf16=True, want_f32=False)
    assert a16 is None and b32 is None
    bits_equal(a32, l32, "f32-only y")
    bits_equal(b16, l16, "bf16-only y")
    bits_equal(amean, lmean, "f32-only mean")
    bits_equal(brstd, lrstd, "bf16-only rstd")
    y32, y16, mean, rstd = _cpu(y32, y16, mean, rstd)
    for r0 in range(0, T, CHUNK):
        s = slice(r0, r0 + CHUNK)
        ref = R.ln_fwd_ref(rows[s].double(), w.double())
        check(mean[s], ref["mean"], ref["mean_b"], f"mean rows {r0}+")
        check(rstd[s], ref["rstd"], ref["rstd_b"], f"rstd rows {r0}+")
        check(y32[s], ref["y"], ref["y_b"], f"y_f32 rows {r0}+")
        check(y16[s], ref["y"], R.bf16_bound(ref["y"], ref["y_b"]), f"y_bf16 rows {r0}+")
    # without audio placeholders (slot and override null): ids that name the placeholder read the table like any other
    n32, _, _, _ = K.embed_ln_fwd(idd, td, wd, LN_EPS)
    plain = table.float()[ids.clamp(0, EMB_V - 1)]
    plain[(ids < 0) | (ids >= EMB_V)] = 0.0
    bits_equal(n32, K.layernorm_fwd(plain.to(DEV), wd, LN_EPS, True, False)[0], "no override")


@pytest.mark.parametrize("impl", ["sorted", "atomic"])
@pytest.mark.parametrize("tab_bf16,ovr_bf16,H", EMB_CASES)
def test_embed_ln_backward_against_float64_autograd(K, monkeypatch, tab_bf16, ovr_bf16, H, impl):
    """Both CM3P_EMBED_BWD forms against float64 autograd through the gather (the reference reads the bf16 values of a bf16 table),
    with the bounds of test_embedding_backward_in_id_order_is_reproducible_and_matches_autograd (atol + rtol |ref|: d_table 2e-4 +
    3e-4, the atomic form 2e-4 + 5e-3, d_audio 1e-4 + 1e-5, dw 2e-3 + 2e-3); the padding row, the placeholder row and ids outside the
    table get no gradient; want_table_grad=False gives the same d_audio and dw."""
    monkeypatch.setenv("CM3P_EMBED_BWD", impl)
    T, ids, table, audio, w, dy = _embed_case(tab_bf16, ovr_bf16, H)
    tr, ar, wr = (t.double().requires_grad_(True) for t in (table, audio, w))
    outside = (ids < 0) | (ids >= EMB_V)
    emb = F.embedding(ids.clamp(0, EMB_V - 1), tr, padding_idx=0).clone()
    emb[outside] = 0.0
    emb[ids == EMB_AUDIO] = ar
    F.layer_norm(emb, (H,), wr, None, R.LN_EPS32).backward(dy.double())

    idd, td, ad, wd, dyd = ids.to(DEV), table.to(DEV), audio.to(DEV), w.to(DEV), dy.to(DEV)
    slot, _ = K.audio_slots(idd, EMB_AUDIO)
    _, _, mean, rstd = K.embed_ln_fwd(idd, td, wd, LN_EPS, slot, ad)
    d_table, d_audio, dw = K.embed_ln_bwd(dyd, idd, td, wd, mean, rstd, 0, slot, ad)
    assert d_table.dtype == torch.float32 and d_audio.dtype == torch.float32
    rt = 3e-4 if impl == "sorted" else 5e-3
    check(d_table, tr.grad, 2e-4 + rt * tr.grad.abs(), f"{impl} d_table")
    assert d_table[0].abs().max().item() == 0.0 and d_table[EMB_AUDIO].abs().max().item() == 0.0
    check(d_audio, ar.grad, 1e-4 + 1e-5 * ar.grad.abs(), f"{impl} d_audio")
    check(dw, wr.grad, 2e-3 + 2e-3 * wr.grad.abs(), f"{impl} dw")
    none, d_audio2, dw2 = K.embed_ln_bwd(dyd, idd, td, wd, mean, rstd, 0, slot, ad, want_table_grad=False)
    assert none is None
    check(d_audio2, ar.grad, 1e-4 + 1e-5 * ar.grad.abs(), "no table grad: d_audio")
    check(dw2, wr.grad, 2e-3 + 2e-3 * wr.grad.abs(), "no table grad: dw")


@pytest.mark.parametrize("density", ["none", "sparse", "all"])
@pytest.mark.parametrize("T", [1, 63, 64, 1023, 1024, 1025, 16 * 1024 + 1, 131072])
def test_audio_slots_is_the_exclusive_cumsum(K, T, density):
    """The single-block scan against cumsum, exactly: less than a wave, a wave, a tile less one, a tile, a tile and one token (the
    carry), sixteen tiles and one, 128 tiles; no placeholder, a tenth of the tokens, every token."""
    g = gen("slots", T, density)
    ids = torch.randint(0, 50, (T,), generator=g)
    audio_id = 50
    if density == "sparse":
        ids[torch.rand(T, generator=g) < 0.1] = audio_id
    elif density == "all":
        ids[:] = audio_id
    flag = ids == audio_id
    slot, count = K.audio_slots(ids.to(DEV), audio_id)
    want = torch.where(flag, torch.cumsum(flag.int(), 0) - 1, -1).to(torch.int32)
    assert slot.dtype == torch.int32 and torch.equal(slot.cpu(), want)
    assert int(count.item()) == int(flag.sum())


# ================================================================================================ C. GeGLU / GELU
SENTINEL = 123.0  # a bf16 number


@pytest.mark.parametrize("T,I", [(1, 8), (333, 192), (5, 1152), (2049, 520), (32768, 1152), (8 * 4096 + 3, 1152), (70000, 256)])
def test_geglu_against_float64(K, T, I):
    """c8 = I / 8 = 1, 24, 32 (below 64), 65 (not dividing 64), 144 (the step's own) - a trip's four items of a lane fall into one
    row or several; T c8 above 2048 x 1024 items at the last three shapes, where every lane takes several trips by the quotient and
    remainder of the grid stride and the last trip is ragged (T c8 is not a multiple of 1024 at 8 x 4096 + 3).  float64
    a Phi(a) b and its two derivatives (erfc); the outputs are one row longer than T and hold a sentinel there afterwards."""
    from cm3p_amd._lib import call, ptr, stream

    g = gen("geglu", T, I)
    h = R.geglu_h(T, I, g)
    dg = torch.randn(T, I, generator=g).to(torch.bfloat16)
    hd, dgd = h.to(DEV), dg.to(DEV)
    out = torch.full((T + 1, I), SENTINEL, dtype=torch.bfloat16, device=DEV)
    call("cm3p_geglu_fwd", ptr(hd), ptr(out), T, I, stream())
    dh = torch.full((T + 1, 2 * I), SENTINEL, dtype=torch.bfloat16, device=DEV)
    call("cm3p_geglu_bwd", ptr(dgd), ptr(hd), ptr(dh), T, I, stream())
    bits_equal(K.geglu_fwd(hd), out[:T], "wrapper == entry point (forward)")
    bits_equal(K.geglu_bwd(dgd, hd), dh[:T], "wrapper == entry point (backward)")
    out, dh = out.cpu(), dh.cpu()
    assert (out[T] == SENTINEL).all() and (dh[T] == SENTINEL).all(), "written past T rows"
    worst_f = worst_b = 0.0
    for r0 in range(0, T, CHUNK):
        s = slice(r0, r0 + CHUNK)
        ref, bnd = R.geglu_fwd_ref(h[s].double())
        worst_f = max(worst_f, check(out[:T][s], ref, bnd, f"geglu fwd rows {r0}+"))
        ref, bnd = R.geglu_bwd_ref(dg[s].double(), h[s].double())
        worst_b = max(worst_b, check(dh[:T][s], ref, bnd, f"geglu bwd rows {r0}+"))
    print(f"geglu T {T} I {I}: worst err/bound fwd {worst_f:.3g} bwd {worst_b:.3g}")


def test_gelu_element_kernels_past_the_grid(K):
    """cm3p_gelu_fwd / _bwd (the same gelu_erf2 / gelu_cdf_pdf2) on more than 2048 x 256 items of 8, against the GeGLU bounds
    with b = 1 and dg = the incoming gradient."""
    n8 = 2048 * 256 + 5
    g = gen("gelu", n8)
    x = (torch.randn(n8 * 8, generator=g) * 3).to(torch.bfloat16)
    dy = torch.randn(n8 * 8, generator=g).to(torch.bfloat16)
    y = K.gelu_fwd(x.to(DEV)).cpu()
    dx = K.gelu_bwd(dy.to(DEV), x.to(DEV)).cpu()
    h = torch.stack([x.double(), torch.ones(n8 * 8, dtype=torch.float64)], 1)  # [n, 2]: a = x, b = 1
    ref, bnd = R.geglu_fwd_ref(h)
    check(y.view(-1, 1), ref, bnd, "gelu fwd")
    ref, bnd = R.geglu_bwd_ref(dy.double().view(-1, 1), h)
    check(dx.view(-1, 1), ref[:, :1], bnd[:, :1], "gelu bwd")


# ================================================================================================ D. RoPE
ROPE_POS = [0, 1, 127, 4095, 8191, 65535, 10 ** 6]


@pytest.mark.parametrize("theta", [10000.0, 160000.0])
@pytest.mark.parametrize("half", [32, 16, 8])
def test_rope_table_is_cos_sin_of_the_fp32_product(K, half, theta):
    """Positions up to 10^6 (angles up to 10^6 radians: the argument reduction of cosf / sinf), shared [1, n] and per-batch [2, n]
    position ids.  The contract is one fp32 product float(pos) * inv_freq; cos / sin of that angle within 2u absolute: one fp32 ulp
    of a value in [1/2, 1] is u to 2u, and the device library's cosf / sinf are specified to 1 ulp."""
    inv_freq = R.rope_inv_freq(theta, 2 * half)
    shared = torch.tensor([ROPE_POS + list(range(900, 1000))])
    per_batch = torch.stack([shared[0], shared[0].flip(0) + 3])
    for pos in (shared, per_batch):
        cos, sin = K.rope_table(pos.to(DEV), inv_freq.to(DEV))
        assert cos.shape == (pos.numel(), half) and cos.dtype == torch.float32
        c64, s64 = R.rope_table_ref(pos, inv_freq)
        check(cos, c64, 2 * U, f"cos half {half} theta {theta} {tuple(pos.shape)}")
        check(sin, s64, 2 * U, f"sin half {half} theta {theta} {tuple(pos.shape)}")


@pytest.mark.parametrize("B,S,nh", [(2, 4096, 12), (1, 3, 1)])
@pytest.mark.parametrize("D", [64, 32, 16])
def test_rope_apply_against_the_float64_rotation(K, D, B, S, nh):
    """cm3p_rope_apply (head_dim 64) and cm3p_rope_apply_generic (16, 32): the forward rotation and, on its own, the inverse, each
    against the float64 rotation of the bf16 input with the kernel's fp32 tables; the v third keeps its bits; shared and per-batch
    tables.  B S nh = 98304: 786432 items of 8 pairs (64) and at least as many single pairs (16, 32), above 2048 x 256."""
    g = gen("rope", D, B, S, nh)
    qkv = torch.randn(B, S, 3, nh, D, generator=g).to(torch.bfloat16)
    inv_freq = R.rope_inv_freq(160000.0, D).to(DEV)
    for per_batch in (False, True):
        pos = torch.stack([torch.arange(S) * (b + 1) + 11 * b for b in range(B)]) if per_batch else torch.arange(S).unsqueeze(0)
        cos, sin = K.rope_table(pos.to(DEV), inv_freq)
        c64, s64 = (t.cpu().double().view(pos.shape[0], S, D // 2) for t in (cos, sin))
        for inverse in (False, True):
            buf = qkv.to(DEV)
            if D == 64:
                K.rope_apply_(buf, cos, sin, B, S, nh, per_batch, inverse=inverse)
            else:
                K.rope_apply_generic_(buf, cos, sin, B, S, nh, D, per_batch, inverse=inverse)
            buf = buf.cpu()
            ref, bnd = R.rope_apply_ref(qkv.double(), c64, s64, inverse)
            check(buf[:, :, :2], ref, bnd, f"rope D {D} per_batch {per_batch} inverse {inverse}")
            bits_equal(buf[:, :, 2], qkv[:, :, 2], "v third untouched")


# ================================================================================================ E. pooling
def _pool_masks(Bn, S, g):
    prefix = (torch.arange(S)[None] < torch.randint(1, S + 1, (Bn, 1), generator=g)).long()
    scattered = (torch.rand(Bn, S, generator=g) < 0.5).long()
    scattered[0, S // 2] = 1
    if Bn > 1:
        scattered[Bn - 1] = 0  # a row with no kept position
    return {"none": None, "prefix": prefix, "scattered": scattered}


@pytest.mark.parametrize("S", [1, 127, 128, 129, 300, 4096])
@pytest.mark.parametrize("H", [4, 128, 768, 1024, 1028, 2048])
def test_pooling_against_float64(K, H, S):
    """H above 1024 takes pool_partial_kernel's second column trip; S below, at and just above one 128-row chunk, three chunks with
    a ragged last one, 32 chunks; fp32 and bf16 rows; cls and mean pooling without a mask, with a prefix mask, with a scattered mask
    and with a row whose mask is all zero (pooled 0, count 0, gradient 0).  cls is exact both ways (a copy; a product with 0 or
    1)."""
    for Bn in (1, 5):
        g = gen("pool", H, S, Bn)
        h32 = torch.randn(Bn, S, H, generator=g) + 0.25
        dp = torch.randn(Bn, H, generator=g)
        masks = _pool_masks(Bn, S, g)
        for h in (h32, h32.to(torch.bfloat16)):
            hd = h.to(DEV)
            for cls in (True, False):
                for kind, mask in masks.items():
                    what = f"pool Bn {Bn} {h.dtype} cls {cls} mask {kind}"
                    md = None if mask is None else mask.to(DEV)
                    pooled, count = K.pool_fwd(hd, md, Bn, S, cls)
                    ref, cnt, bnd = R.pool_ref(h.double(), mask, cls)
                    check(pooled, ref, bnd, what)
                    if not cls:
                        assert torch.equal(count.cpu().double(), cnt), what
                    dh = K.pool_bwd(dp.to(DEV), md, count, Bn, S, cls)
                    ref, bnd = R.pool_bwd_ref(dp.double(), mask, cnt, S, cls)
                    check(dh.view(Bn, S, H), ref, bnd, what + " backward")


# ================================================================================================ F. row gather / scatter
@pytest.mark.parametrize("dtype,H", [(torch.float32, 4), (torch.float32, 768), (torch.bfloat16, 8), (torch.bfloat16, 768)])
@pytest.mark.parametrize("n", [0, 1, 5, 70001])
def test_gather_and_scatter_rows_bit_for_bit(K, n, dtype, H):
    """70001 rows of 768 floats are 13.4 M items of 16 bytes, past the 2048 x 256 grid; bf16 rows move as fp32 rows of half the
    width (the bf16 residual stream of unpadded calls), so H = 8 is one item a row; n = 0 launches nothing.  Indices repeat in the
    gather; the scatter's are distinct, and rows it does not name keep what they held (zeros from the wrapper, a sentinel from the
    entry point)."""
    from cm3p_amd._lib import call, ptr, stream

    g = gen("rows", n, dtype, H)
    total = n + 29
    src = torch.randn(total, H, generator=g).to(dtype)
    idx = torch.randint(0, total, (n,), generator=g)
    got = K.gather_rows(src.to(DEV), idx.to(DEV))
    assert got.dtype == dtype
    bits_equal(got, src[idx], f"gather n {n} H {H} {dtype}")
    perm = torch.randperm(total, generator=g)[:n]
    rows = src[:n].contiguous()
    got = K.scatter_rows(rows.to(DEV), perm.to(DEV), total)
    want = torch.zeros(total, H, dtype=dtype)
    want[perm] = rows
    assert got.dtype == dtype
    bits_equal(got, want, f"scatter n {n} H {H} {dtype}")
    if n:
        r32 = rows.view(torch.float32) if dtype == torch.bfloat16 else rows
        dst = torch.full((total, r32.shape[1]), -7.5, device=DEV)
        rd, pd = r32.to(DEV), perm.to(DEV)
        call("cm3p_scatter_rows_f32", ptr(rd), ptr(pd, torch.int64), ptr(dst), n, r32.shape[1], stream())
        want32 = torch.full((total, r32.shape[1]), -7.5)
        want32[perm] = r32
        bits_equal(dst, want32, "scatter leaves the rows it does not name untouched")
