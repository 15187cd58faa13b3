"""tests/dropout_refs.py and the dropout part of tests/attention_refs.py on the CPU: the correct fp32 emulations of the element kernels
and of head-64 attention with dropout fit every bound tests/test_dropout_kernels_gpu.py applies, on every case of the tables (the
proof that a correct kernel fits; the worst error / bound per quantity is printed), every wrong emulation fails a check on a NAMED
case, the tables contain the rows the checks need (live rows with every visible key dropped, a partly masked last tile the shifted
key group shows on), and the four element entry points refuse every broken precondition before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

import attention_refs as AR
import dropout_refs as DR
from attention_refs import DROPOUT_PS, TABLE_DROP
from test_dropout_host import scale_ref, threshold_ref


# ================================================================================================ element kernels
def test_the_layouts_are_the_ones_the_kernels_must_survive():
    names = {lay.name: lay for lay in DR.PACKED}
    assert names["packed-mixed"].cu == (0, 1, 2, 9, 73, 138, 338, 339)
    assert names["packed-empty_middle"].cu == (0, 5, 5, 9)
    assert names["packed-ones300"].n_seqs == 300 and names["packed-one"].n_seqs == 1
    enc = names["packed-encoder"]
    assert enc.rows % 64 == 0 and 0 < enc.lens[-1] < 64  # the trailing pseudo-sequence of alignment rows
    # the restated binary search: a zero-length sequence owns no row, positions restart at every first row
    b, s = DR.rows_to_seq(names["packed-empty_middle"])
    assert b.tolist() == [0] * 5 + [2] * 4 and s.tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3]
    b, s = DR.rows_to_seq(names["packed-mixed"])
    assert b[[0, 1, 2, 8, 9, 72, 73, 137, 138, 337, 338]].tolist() == [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    assert s[[0, 1, 2, 8, 9, 72, 73, 137, 138, 337, 338]].tolist() == [0, 0, 0, 6, 0, 63, 0, 64, 0, 199, 0]
    # packed rows are the padded twin's rows of the same tokens
    twin, idx = DR.padded_twin(names["packed-mixed"])
    assert (twin.B, twin.S) == (7, 200) and idx[[2, 8, 338]].tolist() == [400, 406, 1200]
    a = DR.keep_rows(names["packed-mixed"], 136, 3, 3, 6554, DR.SEED)
    assert torch.equal(a, DR.keep_rows(twin, 136, 3, 3, 6554, DR.SEED)[idx])
    assert {(c.layout.rows, c.I) for c in DR.GEGLU_CASES} >= {(400, 8), (400, 136), (4104, 1024)}
    assert DR.SEED_TOP_BIT >> 63 == 1 and threshold_ref(0.5) == 32768


def test_the_references_reduce_to_the_plain_geglu_ones_without_dropout():
    h, dg = DR.geglu_data(400, 136)
    keep = torch.ones(400, 136, dtype=torch.bool)
    ref, bound = DR.geglu_fwd_dropout_ref(h.double(), keep, 0)
    ref0, bound0 = DR.RR.geglu_fwd_ref(h.double())
    assert torch.equal(ref, ref0) and bool((bound >= bound0).all()) and bool((bound <= 2.0 * bound0 + 1e-30).all())
    ref, bound = DR.geglu_bwd_dropout_ref(dg.double(), h.double(), keep, 0)
    ref0, bound0 = DR.RR.geglu_bwd_ref(dg.double(), h.double())
    assert torch.equal(ref, ref0) and bool((bound >= bound0).all()) and bool((bound <= 2.0 * bound0 + 1e-30).all())
    assert DR.z64(32768) == 2.0 and DR.z64(65536) == 0.0 and abs(DR.z64(6554) - scale_ref(6554)) <= DR.U * DR.z64(6554)


def test_the_geglu_emulations_fit_every_bound_on_every_case():
    worst = {}
    for case in DR.GEGLU_CASES:
        h, dg = DR.geglu_data(case.layout.rows, case.I)
        fwd = DR.geglu_fwd_dropout_f32_path(h, case.layout, DR.LAYER, case.thr, DR.SEED)
        bwd = DR.geglu_bwd_dropout_f32_path(dg, h, case.layout, DR.LAYER, case.thr, DR.SEED)
        seen, fails = DR.check_geglu(case, fwd, bwd)
        assert not fails, (case.name, fails)
        keep = DR.geglu_reference(case)["keep"]
        assert 0 < int(keep.sum()) < keep.numel()
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("element emulations, worst error / bound over the table: " + "  ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items())))
    assert worst["geglu_fwd"] < 1.0 and worst["geglu_bwd"] < 1.0


def test_the_dropout_f32_contract_is_two_roundings_of_the_float64_value():
    """dropout_f32_path is the contract in bits; against float64 it is off by the rounding of the scale, the product and the sum."""
    for lay, thr in ((DR.PADDED_SMALL, 6554), (DR.PACKED[0], 32768)):
        x, resid = DR.f32_data(lay.rows, 136)
        keep = DR.keep_rows(lay, 136, DR.LAYER, DR.SITE_ATTN_OUT, thr, DR.SEED)
        y32, y16 = DR.dropout_f32_path(x, resid, lay, DR.LAYER, DR.SITE_ATTN_OUT, thr, DR.SEED)
        xz = torch.where(keep, x.double() * DR.z64(thr), torch.zeros(1, dtype=torch.float64))
        want = xz + resid.double()
        assert bool(((y32.double() - want).abs() <= DR.U * (2.0 * xz.abs() + want.abs()) * (1 + 1e-3)).all())
        assert torch.equal(y32[~keep], resid[~keep]) and torch.equal(y16, y32.to(torch.bfloat16))
        y32, _ = DR.dropout_f32_path(x, None, lay, DR.LAYER, DR.SITE_EMBED, 65536, DR.SEED)
        assert not y32.any()


# the case each wrong element emulation is caught on (forward, backward or both), and a case that cannot see it
ELEMENT_CAUGHT_ON = {
    "mask_shifted_group": ("padded-2x200-I8-p0.1", None),                      # one group per row: group 1 for group 0
    "position_absolute": ("padded-2x200-I136-p0.1", "packed-one-I136-p0.1"),   # a single packed sequence: row = position
    "seq_off_by_one": ("packed-mixed-I136-p0.1", "padded-2x200-I136-p0.1"),    # padded rows take no binary search
    "halves_swapped": ("padded-2x200-I8-p0.5", None),
    "scale_missing": ("packed-encoder-I136-p0.1", None),
    "bwd_rounds_dz": ("padded-2x200-I136-p0.1", None),
}


def _element_fails(case, wrong):
    h, dg = DR.geglu_data(case.layout.rows, case.I)
    fwd = DR.geglu_fwd_dropout_f32_path(h, case.layout, DR.LAYER, case.thr, DR.SEED, wrong)
    bwd = DR.geglu_bwd_dropout_f32_path(dg, h, case.layout, DR.LAYER, case.thr, DR.SEED, wrong)
    return DR.check_geglu(case, fwd, bwd)[1]


@pytest.mark.parametrize("wrong", DR.ELEMENT_WRONG)
def test_wrong_element_emulations_fail_on_a_named_case(wrong):
    seen_on, blind = ELEMENT_CAUGHT_ON[wrong]
    case = DR.GEGLU_BY_NAME[seen_on]
    fails = _element_fails(case, wrong)
    print(f"{wrong}: caught on {seen_on}: {fails}")
    assert fails
    if wrong == "bwd_rounds_dz":  # a backward mistake: the forward of the same emulation still fits
        assert all(f.startswith("geglu_bwd") for f in fails)
    else:
        assert any(f.startswith("geglu_fwd") for f in fails) and any(f.startswith("geglu_bwd") for f in fails)
    if blind is not None:  # why the table needs the other case
        assert not _element_fails(DR.GEGLU_BY_NAME[blind], wrong)
    if wrong != "bwd_rounds_dz":  # the bit contract of cm3p_dropout_f32 sees the same mistakes
        x, resid = DR.f32_data(case.layout.rows, case.I)
        args = (x, resid, case.layout, DR.LAYER, DR.SITE_ATTN_OUT, case.thr, DR.SEED)
        good, bad = DR.dropout_f32_path(*args), DR.dropout_f32_path(*args, wrong=wrong)
        assert not torch.equal(good[0], bad[0]) and not torch.equal(good[1], bad[1])


def test_seq_off_by_one_shows_on_every_packed_layout_with_two_sequences():
    for lay in DR.PACKED:
        a = DR.keep_rows(lay, 136, DR.LAYER, 3, 6554, DR.SEED)
        b = DR.keep_rows(lay, 136, DR.LAYER, 3, 6554, DR.SEED, "seq_off_by_one")
        assert torch.equal(a, b) == (lay.n_seqs == 1), lay.name


# ================================================================================================ head-64 attention with dropout
def _attn_checks(case, p, got, keep):
    """Every check the GPU test applies to one dropout forward + backward -> (measured, failures)."""
    pz = threshold_ref(p) / 65536.0
    ref = AR.reference(case, keep, pz)
    seen, fails = AR.check_float64(ref, got)
    s2, f2 = AR.check_conditioned(AR.conditioned(case, got["out"], keep, pz), got)
    fails = fails + f2 + AR.check_exact(case, ref, got)
    gone = AR.all_dropped_rows(case, keep)
    if bool(gone.any()) and (got["out"].float()[gone].abs().max().item() != 0.0 or not bool(torch.isfinite(got["lse"][gone]).all())):
        fails.append("a live row with every visible key dropped: out is not exactly zero or lse is not finite")
    plain = AR.emulate(case)
    if not torch.equal(got["lse"], plain["lse"]):
        fails.append("lse is not the dropout-free one")
    return dict(seen, **s2), fails


def test_table_drop_shape_and_instances():
    assert len(TABLE_DROP) == 12 + 8 + 6 + 6 and len(set(TABLE_DROP)) == 32 and DROPOUT_PS == (0.1, 0.5)
    assert {c.window for c in TABLE_DROP if c.table == "A"} == {0, 1, 63, 64, 65, 300}
    assert {(c.S, c.window) for c in TABLE_DROP if c.table == "B"} == {(64, 31), (257, 127), (449, 449)}
    assert all(Case in TABLE_DROP for Case in AR.TABLE_C + AR.TABLE_G)
    assert {c.pre for c in TABLE_DROP} == {False, True}
    reached = set().union(*(AR.instances(c, drop=True) for c in TABLE_DROP))
    want = ({f"attn_fwd_kernel<1, {p}, {b}>" for p in ("true", "false") for b in ("true", "false")}
            | {f"attn_bwd_dq_kernel<{p}, {m}>" for p in ("true", "false") for m in ("true", "false")}
            | {f"attn_bwd_dkv_kernel<{p}>" for p in ("true", "false")})
    assert reached == want, sorted(want ^ reached)


def test_the_attention_emulation_with_dropout_fits_every_bound_on_every_case():
    worst = {}
    for p in DROPOUT_PS:
        for case in TABLE_DROP:
            keep = DR.attention_keep(case, threshold_ref(p))
            seen, fails = _attn_checks(case, p, AR.emulate(case, keep, threshold_ref(p) / 65536.0), keep)
            assert not fails, (case.name, p, fails)
            for k, v in seen.items():
                worst[(p, k)] = max(worst.get((p, k), 0.0), v)
    print("attention emulation with dropout, worst over TABLE_DROP: " + "  ".join(f"p{p} {k}={v:.3g}" for (p, k), v in sorted(worst.items())))
    for p in DROPOUT_PS:
        for k in ("out", "dq", "dk", "dv", "dq_given_out", "dk_given_out"):
            assert worst[(p, k)] < 1.0, (p, k, worst[(p, k)])


def test_rows_with_every_visible_key_dropped_exist_at_windows_0_and_1():
    thr = threshold_ref(0.5)
    for w in (0, 1):
        for sfx in ("plain", "pre"):
            case = AR.BY_NAME[f"A-S300-w{w}-pad-{sfx}"]
            gone = AR.all_dropped_rows(case, DR.attention_keep(case, thr))
            assert int(gone.sum()) >= 20, (case.name, int(gone.sum()))
            got = AR.emulate(case, DR.attention_keep(case, thr), 0.5)
            assert not got["out"][gone].any() and bool(torch.isfinite(got["lse"][gone]).all())


def test_the_rows_left_out_of_the_gradient_norm_have_a_zero_reference():
    """attention_refs.rel_l2_rows: the relative L2 bound is asserted on every case over the dq rows that see more than one key and the
    dk rows of the keys such rows see; what it leaves out is identically zero in float64 (to its own rounding) and stays under the
    componentwise bound, which no element is exempt from."""
    some, none = 0, 0
    for case in TABLE_DROP:
        keep = DR.attention_keep(case, threshold_ref(0.1))
        ref = AR.reference(case, keep, threshold_ref(0.1) / 65536.0)
        rows = ref["l2_rows"]
        assert AR.reference(case)["l2_rows"] is None  # without dropout the norm is over the whole tensor, as before
        left_out = int((~rows["dq"]).sum()) + int((~rows["dk"]).sum())
        some, none = some + (left_out > 0), none + (left_out == 0)
        for nm in ("dq", "dk"):
            assert not bool((ref[nm][~rows[nm]].abs() > 1e-12).any()), (case.name, nm)
            assert bool((ref["bound"][nm][~rows[nm]] > 0).all())
        assert torch.equal(rows["dq"], ref["nvis"] != 1)
    assert some >= 12 and none >= 8, (some, none)
    case = AR.BY_NAME["A-S300-w300-pad-plain"]  # sequence 2 (one valid key): every dq row and key 0's dk are left out, nothing else
    rows = AR.reference(case, DR.attention_keep(case, threshold_ref(0.1)), 0.1)["l2_rows"]
    assert not rows["dq"][2].any() and rows["dq"][:2].all() and not rows["dk"][2, :, 0].any() and rows["dk"][:2].all()


def test_the_shifted_key_group_changes_a_visible_element_of_a_partly_masked_last_tile():
    hits = []
    for case in TABLE_DROP:
        for p in DROPOUT_PS:
            keep = DR.attention_keep(case, threshold_ref(p))
            t0 = AR.last_tile_start(case.S)
            vis = AR.visible(case).expand(-1, AR.NH, -1, -1)[..., t0:]
            rows = vis.any(-1) & ~vis.all(-1)  # query rows that see a part of the last key tile
            changed = (AR.shift_keep_groups(keep) != keep)[..., t0:] & vis
            assert not (AR.shift_keep_groups(keep) != keep)[..., :max(t0 - 8, 0)].any()
            if bool((changed.any(-1) & rows).any()):
                hits.append((case.name, p))
    print(f"the shifted group shows on a partly masked last tile of {len(hits)} (case, p) pairs")
    assert ("C-S300-w64-holes-plain", 0.1) in hits and ("A-S300-w64-pad-pre", 0.5) in hits


# the (case, p) each wrong attention emulation is caught on
ATTENTION_CAUGHT_ON = {
    "l_dropped": ("A-S300-w64-pad-pre", 0.1),
    "keep_transposed": ("G-S449-w-1-nomask-pre", 0.1),
    "keep_group_shifted": ("C-S300-w64-holes-plain", 0.1),
    "keep_group_shifted_fwd": ("A-S300-w300-pad-pre", 0.1),
    "keep_group_shifted_dq": ("B-S449-w449-nomask-plain", 0.5),
    "keep_group_shifted_dkv": ("G-S257-w-1-pad-pre", 0.1),
    "ds_no_z": ("A-S300-w1-pad-plain", 0.1),
    "dv_no_z": ("B-S64-w31-nomask-pre", 0.1),
    "delta_from_undropped_out": ("A-S300-w0-pad-plain", 0.5),
    "scale_missing_fwd": ("C-S300-w1-holes-pre", 0.1),
}


@pytest.mark.parametrize("wrong", AR.WRONG_DROP)
def test_wrong_attention_emulations_fail_on_a_named_case(wrong):
    name, p = ATTENTION_CAUGHT_ON[wrong]
    case = AR.BY_NAME[name]
    assert case in TABLE_DROP
    keep = DR.attention_keep(case, threshold_ref(p))
    _, fails = _attn_checks(case, p, AR.emulate(case, keep, threshold_ref(p) / 65536.0, wrong=wrong), keep)
    print(f"{wrong}: caught on {name} at p = {p}: {fails}")
    assert fails
    quantity = {"keep_group_shifted_fwd": "out", "keep_group_shifted_dq": "dq", "keep_group_shifted_dkv": "dv", "dv_no_z": "dv",
                "scale_missing_fwd": "out", "ds_no_z": "dq"}.get(wrong)
    if quantity:
        assert any(f.startswith(quantity) for f in fails), fails
    if wrong == "l_dropped":
        assert "lse is not the dropout-free one" in fails


@pytest.mark.parametrize("wrong", ["keep_group_shifted_fwd", "keep_group_shifted_dq", "keep_group_shifted_dkv"])
def test_a_shifted_group_in_one_sweep_fails_at_the_windows_the_model_runs(wrong):
    """windows 64 and -1, both q modes: what the fp32 comparison of tests/test_dropout_gpu.py (2e-2 of the largest gradient) lets through."""
    for name in ("A-S300-w64-pad-plain", "A-S300-w64-pad-pre", "G-S300-w-1-pad-plain", "G-S300-w-1-pad-pre"):
        case = AR.BY_NAME[name]
        keep = DR.attention_keep(case, threshold_ref(0.1))
        assert _attn_checks(case, 0.1, AR.emulate(case, keep, threshold_ref(0.1) / 65536.0, wrong=wrong), keep)[1], (wrong, name)


# ================================================================================================ refusals
ERR_INVALID = -1
_ROWS = " S cu_seqlens n_seqs layer"
ENTRIES = {
    "cm3p_dropout_f32": "x resid y_f32 y_bf16 rows H" + _ROWS + " site thr seed",
    "cm3p_geglu_fwd_dropout": "h g T I" + _ROWS + " thr seed",
    "cm3p_geglu_bwd_dropout": "dg h dh T I" + _ROWS + " thr seed",
    "cm3p_dropout_keep": "keep n2 n1 n0 layer site thr seed",
}
ENTRIES = {name: (params + " stream").split() for name, params in ENTRIES.items()}
_raw = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_raw) + 15) & ~15  # aligned, non-NULL, never dereferenced
POINTERS = ("x", "resid", "y_f32", "y_bf16", "h", "g", "dg", "dh", "keep", "cu_seqlens")
REQUIRED = ("x", "h", "g", "dg", "dh", "keep")  # (resid and cu_seqlens are optional, one of the two outputs is enough)
ALIGNED = ("x", "resid", "y_f32", "y_bf16", "h", "g", "dg", "dh")
# every check passes: 64 packed rows of two sequences, 64 features, p = 0.1 at the MLP site of layer 0
VALID = dict({p: P for p in POINTERS}, rows=64, T=64, H=64, I=64, S=32, n_seqs=2, n2=2, n1=32, n0=64, layer=0, site=3, thr=6554, seed=1234,
             stream=None)


def _breaks(params):
    out = [(f"null_{p}", {p: None}) for p in REQUIRED if p in params]
    out += [(f"misaligned_{p}", {p: P + 8}) for p in ALIGNED if p in params]
    out += [(f"{p}_{v}", {p: v}) for p in ("H", "I") if p in params for v in (0, 12)]
    out += [(f"{p}_0", {p: 0}) for p in ("n2", "n1", "n0") if p in params]
    out += [("thr_-1", {"thr": -1}), ("thr_65537", {"thr": 65537}), ("layer_-1", {"layer": -1}), ("layer_2^29", {"layer": 1 << 29})]
    if "site" in params:
        out += [("site_-1", {"site": -1}), ("site_4", {"site": 4})]
    if "cu_seqlens" in params:  # the row layout: packed rows need sequences, padded rows a length
        out += [("cu_seqlens_with_n_seqs_0", {"n_seqs": 0}), ("no_cu_seqlens_with_S_0", {"cu_seqlens": None, "S": 0})]
    if "y_f32" in params:
        out += [("neither_output", {"y_f32": None, "y_bf16": None})]
    return out


REFUSALS = [(name, label, broken) for name, params in ENTRIES.items() for label, broken in _breaks(params)]


def test_the_argument_lists_are_the_abi_s():
    from cm3p_amd import _lib

    for name, params in ENTRIES.items():
        assert len(params) == len(_lib.SIGNATURES[name]), name
        for p, ctype in zip(params, _lib.SIGNATURES[name]):
            assert (ctype is ctypes.c_void_p) == (p in POINTERS or p == "stream"), (name, p)
    per_entry = {name: {label for n, label, _ in REFUSALS if n == name} for name in ENTRIES}
    assert all({"thr_-1", "thr_65537", "layer_-1", "layer_2^29"} <= labels for labels in per_entry.values())
    assert sum("site_4" in labels for labels in per_entry.values()) == 2
    assert sum("no_cu_seqlens_with_S_0" in labels for labels in per_entry.values()) == 3
    assert {"H_0", "H_12", "neither_output", "misaligned_resid"} <= per_entry["cm3p_dropout_f32"]
    assert {"I_0", "I_12", "null_dg", "misaligned_dh"} <= per_entry["cm3p_geglu_bwd_dropout"]
    for name, label, broken in REFUSALS:
        assert all(p in ENTRIES[name] and VALID[p] != v for p, v in broken.items()), (name, label)
    # padded rows alone are a valid layout: only cu_seqlens = NULL TOGETHER with S = 0 is refused
    assert VALID["S"] > 0 and VALID["n_seqs"] > 0


@pytest.mark.parametrize("name,label,broken", REFUSALS, ids=[f"{n}-{l}" for n, l, _ in REFUSALS])
def test_one_broken_precondition_is_refused(name, label, broken):
    from cm3p_amd import _lib

    args = [broken.get(p, VALID[p]) for p in ENTRIES[name]]
    assert args != [VALID[p] for p in ENTRIES[name]]  # (the unbroken list would reach a launch)
    assert getattr(_lib.load(), name)(*args) == ERR_INVALID


def test_the_layer_bound_is_the_one_the_counter_word_needs():
    """4 layer + site stays a positive int for layer < 2^29 - the last layer every entry takes; the restatement counts with it."""
    assert 4 * ((1 << 29) - 1) + 3 == 2 ** 31 - 1
    a = DR.keep_mask_ref(1, 2, 16, (1 << 29) - 1, 3, 32768, DR.SEED)
    b = DR.keep_mask_ref(1, 2, 16, 0, 3, 32768, DR.SEED)
    assert a.shape == (1, 2, 16) and not np.array_equal(a, b)
