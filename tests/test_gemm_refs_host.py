"""The generators, references and bounds of tests/test_gemm_kernels_gpu.py, checked without a GPU: the data is exact (an fp32 matmul
equals the float64 one bit for bit), a torch fp32 restatement of the kernels' arithmetic (tests/gemm_refs.py: gemm_f32_path,
rope_f32_path, R.geglu_fwd_f32_path) passes every check the GPU test makes, and the wrong evaluations the kernels could fall into
fail them.  The case table's hand-stated kernels agree with the restated dispatch rule and with the library's own: cm3p_gemm_route,
the host-only answer of the routing function the entry points launch from (csrc/gemm.hip cm3p_gemm_route_of)."""
import pytest
import torch

import gemm_refs as G
import row_kernel_refs as R
from row_kernel_refs import bits_equal, check, gen

HOST_M, HOST_N = 264, 136  # rows / columns of the host-side operands (the properties shown here do not depend on the extents)
KS_USED = sorted({c.K for c in G.ALL_CASES if not c.name.startswith("random")} | {k for _, _, k in G.GEGLU})


def _fails_bits(got, want, what):
    with pytest.raises(AssertionError, match="elements differ"):
        bits_equal(got, want, what)


def _fails(got, ref, bound, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        check(got, ref, bound, what)


def test_case_table_states_the_kernel_the_restated_rule_gives():
    for c in G.ALL_CASES:
        assert G.restated_kernel(c) == (c.kernel, c.rebal), (c, G.restated_kernel(c))
    names = [c.name for c in G.ALL_CASES]
    assert len(set(names)) == len(names)
    # the seams the cases are there for
    assert [c.K // 64 for c in G.FORWARD] == [1, 2, 3, 4, 5] and [c.rebal for c in G.FORWARD] == [False, True, False, True, False]
    assert all(-(-c.M // 256) * -(-c.N // 256) in range(200, 205) for c in G.FORWARD + G.EDGES + G.DGRAD + G.KS_A + G.PITCHED + G.RANDOM)
    for c, (nk, last, rebal) in zip(G.WGRAD, [(2, 2, True), (4, 2, True), (2, 1, False)]):
        kchunk, splits = G.kchunk_of(c.K, c.split_k)
        assert (splits, kchunk // 64, (c.K - (splits - 1) * kchunk) // 64, c.rebal) == (34, nk, last, rebal) and 6 * splits >= 200
    kchunk, splits = G.kchunk_of(G.LINEAR_WGRAD.K, G.LINEAR_WGRAD.split_k)
    assert (splits, kchunk // 64, (G.LINEAR_WGRAD.K - 3 * kchunk) // 64) == (4, 33, 30) and G.LINEAR_WGRAD.K % 2048 != 0
    assert G.kchunk_of(1000, 3) == (384, 3) and (1000 - 2 * 384) % 64 != 0
    assert {c.M % 8 for c in G.EDGES if "mod4" in c.name} == {4} and {c.N % 8 for c in G.EDGES if "mod4" in c.name} == {4}
    for T, I, Kd in G.GEGLU:
        assert Kd % 64 == 0 and I % 32 == 0 and T % 8 == 0 and -(-T // 256) * -(-2 * I // 256) >= 200
    for S, B in G.ROPE_BIG:
        assert G.rope_case(S, B).kernel == G.RING and (S * B) % 8 == 0
    for S, B in G.ROPE_SMALL:
        assert G.rope_case(S, B).kernel == G.SMALL


# ================================================================================================ the library's own route
IMPLS = [None, "256", "128"]
K128, K256, KRING = 0, 1, 2  # cm3p_gemm_route's kernel numbers (include/cm3p_hip.h)
EPI_AXPBY = 4


def _set_impl(monkeypatch, impl):
    if impl is None:
        monkeypatch.delenv("CM3P_GEMM_IMPL", raising=False)
    else:
        monkeypatch.setenv("CM3P_GEMM_IMPL", impl)


def _route(M, N, K, a_kc=True, b_kc=True, epi=G.EPI_F32, split_k=1, lda=None, ldb=None, rope_cols=0, batch=0):
    """One call of cm3p_gemm_route -> (kernel, rebal, splits), or None where the library refuses."""
    from cm3p_amd import _lib

    lda = (K if a_kc else M) if lda is None else lda
    ldb = (K if b_kc else N) if ldb is None else ldb
    code = _lib.query("cm3p_gemm_route", M, N, K, lda, ldb, int(a_kc), int(b_kc), epi, split_k, rope_cols, batch)
    return None if code < 0 else (code & 3, bool(code & 4), code >> 3)


@pytest.mark.parametrize("impl", IMPLS)
def test_the_librarys_route_spells_the_tag_the_case_table_states(monkeypatch, impl):
    """Every case, every epilogue it accepts, under every value of CM3P_GEMM_IMPL: the tag cm3p_amd.kernels spells from
    cm3p_gemm_route is the hand table's, and the split count the library recomputes is kchunk_of's."""
    from cm3p_amd import kernels as K

    _set_impl(monkeypatch, impl)
    for c in G.ALL_CASES:
        for epi in c.epilogues():
            assert K._gemm_tag(c.M, c.N, c.K, c.a_kc, c.b_kc, epi, c.split_k) == c.tag(epi, impl), (c, epi, impl)
        assert _route(c.M, c.N, c.K, c.a_kc, c.b_kc, G.EPI_F32, c.split_k)[2] == G.kchunk_of(c.K, c.split_k)[1], c
    for S, B in G.ROPE_BIG + G.ROPE_SMALL:
        c = G.rope_case(S, B)
        assert (2 * c.N // 3) % 256 == 0
        assert K._gemm_tag(c.M, c.N, c.K, True, True, G.EPI_ROPE, 1, rope_cols=2 * c.N // 3) == c.tag(G.EPI_ROPE, impl), (c, impl)
    for T, I, Kd in G.GEGLU:
        # cm3p_gemm_geglu runs on the ring whenever it is called; under CM3P_GEMM_IMPL=256 the route names gemm256_kernel and the
        # caller keeps the two-kernel path (gemm_geglu_supported), under 128 the fusion stays on
        rebal = (Kd // 64) % 2 == 0
        assert _route(T, 2 * I, Kd, epi=G.EPI_GEGLU) == (K256 if impl == "256" else KRING, rebal, 1)
        assert K.gemm_geglu_supported(T, I, Kd) == (impl != "256")
        assert K._gemm_tag(T, 2 * I, Kd, True, True, G.EPI_GEGLU, 1, kernel=K._GEMM_RING) == f"{G.RING}<true, true, 6, {'true' if rebal else 'false'}>"


def test_routes_no_case_states():
    """The ring's 32-bit lane offsets, the rotary tile-boundary condition, the batched entry's thresholds and layouts, what the
    route refuses: one query each, no data."""
    big = dict(M=51200, N=256, K=64)  # 200 tiles
    assert _route(**big) == (KRING, False, 1)
    # 16 rows of an operand must lie inside a 32-bit byte offset: lda * 16 elements * 2 bytes < 2^32 / 2
    assert _route(**big, lda=2 ** 27 - 8) == (KRING, False, 1) and _route(**big, lda=2 ** 27) == (K256, False, 1)
    assert _route(**big, ldb=2 ** 27 - 8) == (KRING, False, 1) and _route(**big, ldb=2 ** 27) == (K256, False, 1)
    # RoPE: 3 heads rotate 384 columns, which end inside a 256-column tile: the 128 x 128 kernel whatever M; 4 heads end on one
    for M in (256, 51200, 2 ** 22):
        assert _route(M, 576, 64, epi=G.EPI_ROPE, rope_cols=384) == (K128, False, 1)
    assert _route(51200, 768, 64, epi=G.EPI_ROPE, rope_cols=512) == (KRING, False, 1)
    assert _route(2 ** 31, 768, 64, epi=G.EPI_ROPE, rope_cols=512) == (K128, False, 1)  # (32-bit table row arithmetic)
    # batched (epilogue 4): 128 (matrix, tile) items
    bt = dict(K=128, epi=EPI_AXPBY)
    assert _route(256, 256, batch=127, **bt) == (K128, False, 1) and _route(256, 256, batch=128, **bt) == (KRING, True, 1)
    # ... whose tiles are 0.7 full: 256 x 184 = 47104 >= 0.7 x 65536 = 45875.2 > 256 x 176 = 45056
    assert _route(256, 184, batch=128, **bt) == (KRING, True, 1) and _route(256, 176, batch=128, **bt) == (K128, False, 1)
    # ... in the Muon step's three layouts
    for a_kc, b_kc in ((True, True), (True, False), (False, False)):
        assert _route(256, 256, a_kc=a_kc, b_kc=b_kc, batch=128, **bt) == (KRING, True, 1)
    assert _route(256, 256, a_kc=False, b_kc=True, batch=128, **bt) == (K128, False, 1)
    assert _route(256, 256, batch=128, K=96, epi=EPI_AXPBY) == (K128, False, 1) and _route(252, 256, a_kc=False, b_kc=False, batch=200, **bt)[0] == K128
    # refusals: no kernel has the pair, or the arguments are no call of any entry point
    for epi in (G.EPI_ROPE, G.EPI_F32_BIAS, G.EPI_GEGLU):
        for a_kc, b_kc in ((True, False), (False, True), (False, False)):
            assert _route(51200, 256, 64, a_kc, b_kc, epi) is None
    assert _route(**big, epi=EPI_AXPBY) is None and _route(**big, batch=2) is None and _route(**big, epi=8) is None and _route(**big, epi=-1) is None
    assert _route(**big, split_k=0) is None and _route(0, 256, 64) is None and _route(256, 0, 64) is None and _route(256, 256, 0) is None
    # cm3p_gemm_geglu's shape rule (T, 2 I, K): T % 8, I % 32, K % 64, 200 tiles
    assert _route(51200, 256, 64, epi=G.EPI_GEGLU) == (KRING, False, 1)
    for T, N, Kd in ((51204, 256, 64), (51200, 288, 64), (51200, 256, 96), (50944, 256, 64)):
        assert _route(T, N, Kd, epi=G.EPI_GEGLU) is None, (T, N, Kd)


@pytest.mark.parametrize("impl", IMPLS)
def test_switches_on_the_routes_no_case_states(monkeypatch, impl):
    """CM3P_GEMM_IMPL=256 takes the ring away from a batch too (128 x 128 then); 128 leaves the batched and GeGLU entries alone."""
    _set_impl(monkeypatch, impl)
    assert _route(256, 256, 128, epi=EPI_AXPBY, batch=128)[0] == (K128 if impl == "256" else KRING)
    assert _route(51200, 256, 64, lda=2 ** 27)[0] == (K128 if impl == "128" else K256)
    assert _route(51200, 768, 64, epi=G.EPI_ROPE, rope_cols=512)[0] == {None: KRING, "256": K256, "128": K128}[impl]


@pytest.mark.parametrize("impl", IMPLS)
def test_no_route_names_a_ring_or_256_instance_that_does_not_exist(monkeypatch, impl):
    """The launchers answer CM3P_ERR_INTERNAL for a (layout, epilogue) pair their file does not instantiate.  No such pair comes out
    of the route: over every layout and epilogue number, at shapes that reach each kernel, a route either refuses or names a kernel
    that has the pair (the has_instance statements of csrc/gemm.hip, gemm256.hip and gemm8p.hip, restated)."""
    _set_impl(monkeypatch, impl)
    fwd_only = (G.EPI_ROPE, G.EPI_F32_BIAS, G.EPI_GEGLU)

    def exists(kernel, a_kc, b_kc, epi):
        if epi in fwd_only and not (a_kc and b_kc):
            return False
        if epi == G.EPI_GEGLU:
            return kernel == KRING
        if epi == EPI_AXPBY:
            return kernel == K128 or (kernel == KRING and (a_kc or not b_kc))
        return True

    seen = set()
    for M, N, Kd, batch in ((51200, 256, 64, 200), (51204, 252, 64, 200), (264, 136, 96, 2)):
        for a_kc in (True, False):
            for b_kc in (True, False):
                for epi in range(8):
                    r = _route(M, N, Kd, a_kc, b_kc, epi, rope_cols=256 if epi == G.EPI_ROPE else 0, batch=batch if epi == EPI_AXPBY else 0)
                    if r is not None and not (epi == G.EPI_GEGLU and impl == "256"):  # (that route is advice to the caller: see above)
                        assert exists(r[0], a_kc, b_kc, epi), (M, N, Kd, a_kc, b_kc, epi, r)
                        seen.add(r[0])
    assert seen == {None: {K128, K256, KRING}, "256": {K128, K256}, "128": {K128, KRING}}[impl]


@pytest.mark.parametrize("K", KS_USED)
def test_generated_data_is_exact_at_full_significand_width(K):
    """max |m|^2 K < 2^24, the values are bf16 numbers, and an fp32 matmul (whatever order the BLAS adds in) returns the float64
    matmul bit for bit - for the plain generator and the GeGLU-scaled one."""
    for exps_a, exps_b in ((G.EXPS, G.EXPS), G.geglu_exps(K)):
        g = gen("host-exact", K, exps_a)
        a, ma, ea = G.exact_operand(HOST_M, K, g, exps=exps_a, parts=True)
        b, mb, eb = G.exact_operand(HOST_N, K, g, exps=exps_b, parts=True)
        assert int(ma.abs().max()) * int(mb.abs().max()) * K < 2 ** 24 and G.mmax_for(K) ** 2 * K < 2 ** 24
        assert int(ma.abs().max()) == G.mmax_for(K) and bool((ma % 2 != 0).any())  # the full width is in use
        assert torch.equal(a.double(), ma.double() * 2.0 ** ea.double()[:, None])
        assert torch.equal(a.to(torch.bfloat16).float(), a) and torch.equal(b.to(torch.bfloat16).float(), b)
        acc = G.acc64(a, b)
        assert torch.equal(acc, (ma @ mb.t()).double() * 2.0 ** (ea.double()[:, None] + eb.double()[None, :]))  # the int64 matmul
        bits_equal(a @ b.t(), acc.float(), f"K {K}: fp32 matmul")
        assert torch.equal(acc.float().double(), acc)
        assert len(set(ea.tolist())) == len(exps_a) and len(set(eb.tolist())) == len(exps_b)


@pytest.mark.parametrize("K", [64, 192, 256, 320, 1000, 4288])
def test_plain_epilogues_pass_for_the_fp32_path_and_refuse_wrong_evaluations(K):
    g = gen("host-plain", K)
    a, b = G.exact_operand(HOST_M, K, g), G.exact_operand(HOST_N, K, g)
    acc = G.acc64(a, b)
    r32, r16, bias = G.residuals(HOST_M, HOST_N, acc, g)
    refs = G.epilogue_refs(acc, r32, r16, bias)
    resid = {G.EPI_F32_RESID: r32, G.EPI_F32_BIAS: bias, G.EPI_BF16_RESID: r16}
    assert set(refs) == set(G.PLAIN_EPILOGUES)
    for epi in G.PLAIN_EPILOGUES:
        r = resid.get(epi)
        bits_equal(G.gemm_f32_path(a, b, epi, r), refs[epi], f"K {K} epilogue {epi}")
        for wrong in ("drop_chunk", "swap_chunks", "clear_bits"):
            _fails_bits(G.gemm_f32_path(a, b, epi, r, wrong=wrong), refs[epi], f"K {K} epilogue {epi} {wrong}")
    for epi in (G.EPI_BF16, G.EPI_BF16_RESID):  # truncation instead of RNE
        _fails_bits(G.gemm_f32_path(a, b, epi, resid.get(epi), wrong="trunc"), refs[epi], f"K {K} epilogue {epi} truncated")
    _fails_bits(G.gemm_f32_path(a, b, G.EPI_BF16_RESID, r16, wrong="resid_first"), refs[G.EPI_BF16_RESID], "residual added before the rounding")
    kchunk = 128 if K > 128 else 64  # a last split of K - kchunk floor((K - 1) / kchunk) columns that is skipped
    _fails_bits(G.gemm_f32_path(a, b, G.EPI_F32, wrong="skip_last_split", kchunk=kchunk), refs[G.EPI_F32], "short last split skipped")


def test_small_integer_data_does_not_see_damaged_low_bits_and_the_new_data_does():
    """Integers in [-4, 4] have three significand bits: an evaluation that clears the low four of bf16's seven stored bits returns
    the right answer on them.  On m 2^e data it does not."""
    g = gen("host-sharp")
    a, b = G.small_int_operand(HOST_M, 192, g), G.small_int_operand(HOST_N, 192, g)
    bits_equal(G.gemm_f32_path(a, b, G.EPI_F32, wrong="clear_bits"), G.acc64(a, b).float(), "[-4, 4] data, low bits cleared")
    a, b = G.exact_operand(HOST_M, 192, g), G.exact_operand(HOST_N, 192, g)
    _fails_bits(G.gemm_f32_path(a, b, G.EPI_F32, wrong="clear_bits"), G.acc64(a, b).float(), "m 2^e data, low bits cleared")


def test_random_data_bound_holds_for_an_fp32_matmul_and_refuses_a_dropped_chunk():
    g = gen("host-random")
    K = G.RANDOM[0].K
    a, b = G.random_operand(HOST_M, K, g), G.random_operand(HOST_N, K, g)
    ref, bound = G.acc64(a, b), G.random_bound(a, b)
    assert check(a @ b.t(), ref, bound, "fp32 matmul") <= 0.5  # (rounded adds: the any-order half of the bound)
    # one after another in fp32, k ascending: the longest addition path
    s = torch.zeros(HOST_M, HOST_N)
    for k in range(K):
        s = s + a[:, k, None] * b[None, :, k]
    assert check(s, ref, bound, "sequential fp32 sum") <= 0.5
    _fails(G.gemm_f32_path(a, b, G.EPI_F32, wrong="drop_chunk"), ref, bound, "dropped chunk")
    _fails(G.gemm_f32_path(a, b, G.EPI_F32, wrong="clear_bits"), ref, bound, "low bits cleared")


@pytest.mark.parametrize("per_batch", [False, True])
@pytest.mark.parametrize("S", [200, 300])
def test_rope_specifications_pass_their_fp32_paths_and_tell_the_two_kernels_apart(S, per_batch):
    B, nh = 2, G.ROPE_NH
    case = G.rope_case(S, B)
    g = gen("host-rope", S)
    x, w = G.exact_operand(case.M, case.K, g), G.exact_operand(case.N, case.K, g)
    acc = G.acc64(x, w)
    pos = G.rope_positions(S, B, per_batch)
    cos, sin = R.rope_table_ref(pos, R.rope_inv_freq(10000.0, 64))
    cos32, sin32 = cos.float(), sin.float()  # the table as the kernels read it; the references take these very values
    for q_scale in (1.0, G.SOFTMAX_Q_SCALE):
        spec = {small: G.rope_ref(acc, cos32.double(), sin32.double(), S, per_batch, q_scale, nh, small) for small in (False, True)}
        for small in (False, True):
            ref, bound = spec[small]
            what = f"S {S} per_batch {per_batch} q_scale {q_scale:.3g} small {small}"
            for fma in (False, True):
                check(G.rope_f32_path(acc.float(), cos32, sin32, S, per_batch, q_scale, nh, small, fma=fma), ref, bound, f"{what} fma {fma}")
            _fails(G.rope_f32_path(acc.float(), cos32, sin32, S, per_batch, q_scale, nh, small, wrong="wrong_side"), ref, bound, f"{what} wrong side")
            if not per_batch:
                _fails(G.rope_f32_path(acc.float(), cos32, sin32, S, per_batch, q_scale, nh, small, wrong="wrong_modulus"), ref, bound,
                       f"{what} wrong modulus")
            # the v third: exact, and truncation is seen
            _fails(G.trunc_bf16(acc.float()).to(torch.bfloat16), ref, bound, f"{what} truncated")
        # the two specifications are distinguishable: each one's reference lies outside the other's bound somewhere
        (ref_r, bound_r), (ref_s, bound_s) = spec[False], spec[True]
        n_rs = int(((ref_r - ref_s).abs() > bound_s).sum())
        n_sr = int(((ref_r - ref_s).abs() > bound_r).sum())
        print(f"S {S} per_batch {per_batch} q_scale {q_scale:.3g}: {n_rs} elements of the ring reference outside the small kernel's bound, {n_sr} the reverse")
        assert n_rs > 0 and n_sr > 0


@pytest.mark.parametrize("T,I,K", [(264, I, K) for _, I, K in G.GEGLU])
def test_geglu_data_sits_inside_gelus_slope_and_the_bound_refuses_a_swapped_gate(T, I, K):
    g = gen("host-geglu", I, K)
    ea, eb = G.geglu_exps(K)
    x, wi = G.exact_operand(T, K, g, exps=ea), G.exact_operand(2 * I, K, g, exps=eb)
    acc = G.acc64(x, wi)
    inside = float((acc.abs() <= 6).double().mean())
    print(f"K {K}: {inside:.4f} of h inside [-6, 6], std {float(acc.std()):.3g}")
    assert inside >= 0.99 and float(acc.std()) >= 0.5
    ref, bound = G.geglu_ref(acc)
    h = acc.float().to(torch.bfloat16)
    check(R.geglu_fwd_f32_path(h), ref, bound, "geglu fp32 path")
    _fails(R.geglu_fwd_f32_path(h, wrong="swapped"), ref, bound, "gelu(b) a")
    _fails(R.geglu_fwd_f32_path(G.trunc_bf16(acc.float()).to(torch.bfloat16)), ref, bound, "h truncated")
    idx = G.geglu_interleave_index(I)
    assert sorted(idx.tolist()) == list(range(2 * I))
    assert idx[:64].tolist() == list(range(32)) + list(range(I, I + 32))
