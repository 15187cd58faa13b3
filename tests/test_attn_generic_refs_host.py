"""tests/attn_generic_refs.py on the CPU: the closed-form float64 reference agrees with float64 autograd, a torch fp32 emulation of the
small-head attention kernels' arithmetic (csrc/attention_generic.hip) passes every check of tests/test_attn_generic_gpu.py on every case
of the table with and without dropout (the proof that a correct kernel fits the derived bounds; the worst error / bound per quantity is
printed), each wrong evaluation fails a NAMED check, and the table reaches every branch of the kernels' index arithmetic."""
import functools

import pytest
import torch

import attention_refs as AR
import attn_generic_refs as GR
from attn_generic_refs import NH, TABLE, TABLE_A, TABLE_P


@functools.lru_cache(maxsize=None)
def _ref(g):
    return GR.reference(g)


@functools.lru_cache(maxsize=None)
def _ref_drop(g, p):
    return GR.reference(g, GR.bernoulli_keep(g, p), p)


def _fails(g, wrong, p=None):
    """The names of the checks a wrong evaluation fails on one case."""
    if p is None:
        return set(GR.all_checks(g, _ref(g), GR.emulate(g, wrong=wrong))[1])
    return set(GR.all_checks(g, _ref_drop(g, p), GR.emulate(g, GR.bernoulli_keep(g, p), p, wrong=wrong))[1])


def test_reference_agrees_with_float64_autograd():
    for name, p in (("d16-A-S300-w33-pad-plain", None), ("d32-C-S300-w64-holes-plain", 0.5), ("d16-G-S257-w-1-pad-plain", 0.1),
                    ("d32-B-S65-w1-nomask-plain", None)):
        g = GR.BY_NAME[name]
        keep = GR.bernoulli_keep(g, p) if p else None
        ref = GR.reference(g, keep, p or 0.0)
        x = GR.inputs(g)
        q, k, v = (x[n].clone().requires_grad_(True) for n in "qkv")
        vis = AR.visible(g.case)
        dead = ~vis.any(-1, keepdim=True)
        s = ((q @ k.transpose(-1, -2)) * g.scale).masked_fill(~vis, float("-inf")).masked_fill(dead, 0.0)
        pr = torch.softmax(s, dim=-1).masked_fill(dead, 0.0)
        if keep is not None:
            pr = pr * keep.double() / (1.0 - p)
        o = pr @ v
        o.backward(AR.heads(x["do"].double()))
        for nm, want in (("out", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
            assert (ref[nm] - want).abs().max().item() < 1e-12, (name, nm)
        km = AR.key_mask(g.case)
        if km is not None:  # padded and masked keys: exact zeros
            off = (~km)[:, None, :].expand(-1, NH, -1)
            assert not ref["dk"][off].any() and not ref["dv"][off].any()


def test_the_emulation_passes_every_check_on_every_case():
    worst = {}
    for g in TABLE + TABLE_P:
        seen, fails = GR.all_checks(g, _ref(g), GR.emulate(g))
        assert not fails, (g.name, fails)
        for k, v in seen.items():
            worst[f"d{g.D} {k}"] = max(worst.get(f"d{g.D} {k}", 0.0), v)
    print("emulation, worst error / bound over the table: " + "  ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items())))
    assert all(v < 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("p", GR.DROPOUT_PS)
def test_the_emulation_with_dropout_passes_on_every_case(p):
    worst = {}
    for g in TABLE:
        seen, fails = GR.all_checks(g, _ref_drop(g, p), GR.emulate(g, GR.bernoulli_keep(g, p), p))
        assert not fails, (g.name, p, fails)
        for k, v in seen.items():
            worst[f"d{g.D} {k}"] = max(worst.get(f"d{g.D} {k}", 0.0), v)
    print(f"emulation with dropout {p}, worst error / bound: " + "  ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items())))
    assert all(v < 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("wrong", GR.VISIBILITY_WRONG[:4])
def test_a_window_edge_off_by_one_fails_the_count_at_every_window_of_table_a(wrong):
    """... at every window where the mask differs, on the count probe (count_lse: lse = ln n_vis) and on a float64 bound of the random
    data; both head sizes."""
    for D in GR.HEAD_DIMS:
        for w in AR.WINDOWS_A:
            probe = GR.BY_NAME[f"d{D}-PA-S300-w{w}-pad-plain"]
            data = GR.BY_NAME[f"d{D}-A-S300-w{w}-pad-plain"]
            differs = not torch.equal(GR.wrong_visibility(probe.case, wrong), AR.visible(probe.case))
            assert differs == (w < (299 if wrong.endswith("wide") else 300)), (wrong, w)  # (S - 1 and S are the whole axis)
            if differs:
                assert "count_lse" in _fails(probe, wrong), (wrong, D, w)
                assert _fails(data, wrong) & {"out", "lse", "dq", "dk", "dv", "dead_rows"}, (wrong, D, w)


# wrong evaluation -> (a case that must refuse it, dropout p or None, the check that must fail)
NAMED = {
    "low_edge_narrow": ("d16-PA-S300-w64-pad-plain", None, "count_lse"),
    "low_edge_wide": ("d16-PA-S300-w63-pad-plain", None, "count_lse"),
    "high_edge_narrow": ("d32-PA-S300-w64-pad-plain", None, "count_lse"),
    "high_edge_wide": ("d32-PA-S300-w65-pad-plain", None, "count_lse"),
    "tail_keys": ("d16-PA-S300-w33-pad-plain", None, "count_lse"),
    "mask_ignored": ("d16-C-S300-w33-holes-plain", None, "padded_keys"),
    "dead_uniform": ("d16-C-S300-w33-holes-plain", None, "dead_rows"),
    "dk_no_scale": ("d32-A-S300-w1-pad-plain", None, "dk"),
    "p_bf16": ("d16-A-S300-w1-pad-plain", None, "out"),
    "l_dropped": ("d16-A-S300-w64-pad-plain", 0.1, "lse"),
    "keep_transposed": ("d16-A-S300-w64-pad-plain", 0.1, "out"),
    "ds_no_z": ("d32-A-S300-w64-pad-plain", 0.1, "dq"),
    "dv_no_z": ("d32-A-S300-w64-pad-plain", 0.1, "dv"),
}


@pytest.mark.parametrize("wrong", GR.WRONG)
def test_each_wrong_evaluation_fails_a_named_check(wrong):
    name, p, check = NAMED[wrong]
    failed = _fails(GR.BY_NAME[name], wrong, p)
    print(f"{wrong} on {name}: fails {sorted(failed)}")
    assert check in failed, (wrong, name, sorted(failed))


def test_wrong_evaluations_fail_at_both_head_sizes_and_dropout_rates():
    for D in GR.HEAD_DIMS:
        for wrong in ("tail_keys", "mask_ignored", "dead_uniform", "dk_no_scale", "p_bf16"):
            caught = [g.name for g in TABLE + TABLE_P if g.D == D and g.case.table in "AC" and _fails(g, wrong)]
            assert caught, (D, wrong)
        for p in GR.DROPOUT_PS:
            g = GR.BY_NAME[f"d{D}-A-S300-w65-pad-plain"]
            for wrong, check in (("l_dropped", "lse"), ("keep_transposed", "out"), ("ds_no_z", "dq"), ("ds_no_z", "dk"), ("dv_no_z", "dv")):
                assert check in _fails(g, wrong, p), (D, p, wrong)


def test_p_rounded_to_bf16_is_refused_where_the_two_u_bound_would_take_it():
    """The head-64 path rounds P to bf16 for the matrix cores and its bound is 2 u (P o Z)|V|; these kernels keep P in fp32 and are held to
    1 u: the emulation with P rounded fails `out` here, and would pass with tests/attention_refs.py's leading term."""
    g = GR.BY_NAME["d16-A-S300-w1-pad-plain"]
    ref, got = _ref(g), GR.emulate(g, wrong="p_bf16")
    err = (got["out"].double() - ref["out"]).abs()
    assert bool((err > ref["bound"]["out"]).any())
    assert bool((err <= 2.0 * ref["bound"]["out"]).all())


def test_the_table_reaches_every_branch_of_the_index_arithmetic():
    for D in GR.HEAD_DIMS:
        seen = set().union(*(GR.coverage(g) for g in TABLE if g.D == D and g.case.window >= 0))
        assert not GR.COVERAGE_REQUIRED - seen, (D, sorted(GR.COVERAGE_REQUIRED - seen))
        off_tile = set().union(*(GR.coverage(g) for g in TABLE if g.D == D and g.case.window >= 0 and g.case.window % 64))
        assert not GR.COVERAGE_REQUIRED - off_tile, (D, "only at windows on a tile multiple", sorted(GR.COVERAGE_REQUIRED - off_tile))
    # the global cases sweep every tile and take no per-key skip
    assert GR.coverage(GR.BY_NAME["d16-G-S257-w-1-pad-plain"]) >= {"tail_tile_with_keys_past_S", "key_block_without_a_valid_key"}


def test_table_shapes():
    assert len(TABLE_A) == 38 and len(GR.TABLE_B) == 18 and len(GR.TABLE_C) == 8 and len(GR.TABLE_G) == 6 and len(GR.TABLE_64) == 4
    assert len(TABLE_P) == 38 and {g.case.window for g in TABLE_P} == set(AR.WINDOWS_A)
    assert {g.case.table for g in GR.TABLE_64} == set("ABCG") and all(g.D == 64 for g in GR.TABLE_64)
    assert all(g.B * g.S <= 4 * 449 and not g.case.pre for g in TABLE + TABLE_P)
    assert len(GR.TABLE_DROP) == 2 * (len(GR.DROPOUT_WINDOWS_A) + 4 + 3)
    assert GR.inputs(GR.TABLE_64[0])["qkv"] is AR.inputs(GR.TABLE_64[0].case)["qkv_dev"]  # head 64: the data the MFMA kernels are held to
    probe = GR.inputs(TABLE_P[0])
    assert not probe["q"].any() and not probe["k"].any() and bool((probe["v"].abs() == 1).all())
    assert len({tuple(probe["v"][0, 0, s].tolist()) for s in range(300)}) == 300  # 10 bits at D = 16: every key has its own sign pattern
