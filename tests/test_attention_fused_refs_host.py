"""tests/attention_fused_refs.py on the CPU: the emulation of cm3p_attn_bwd_fused passes every check of tests/test_attention_fused_gpu.py
on every case of table F at G = 2 and G = 4, with and without the RoPE epilogues, padded and packed (the proof that a correct kernel fits
the derived bounds); every entry of WRONG_FUSED fails one of them on a named case; the table reaches the seams it names; the row-subset
reference is the full one's rows; the G-dependent bound and the sequential slab adds are what the module docstrings state."""
import functools

import pytest
import torch

import attention_fused_refs as AF
import attention_refs as AR
from attention_fused_refs import TABLE_F
from attention_refs import NH


@functools.lru_cache(maxsize=None)
def _ref(case, packed=False):
    return AR.reference(case, x=AF.padded_rows_zeroed(case) if packed else None)


def _checks(case, got, G, rope=None, packed=False):
    """Every check the GPU test applies to one forward + fused backward -> (measured, failures)."""
    ref = _ref(case, packed)
    x = AF.padded_rows_zeroed(case) if packed else None
    cond = AR.conditioned(case, got["out"], x=x)
    plain = ("out", "lse", "dv") if rope else ("out", "lse", "dq", "dk", "dv")
    seen, fails = AR.check_float64(ref, got, fused=True, G=G, quantities=plain)
    fails = fails + AR.check_exact(case, ref, got)
    if rope:
        cos, sin, index = AF.rope_tables(case, rope)
        s2, f2 = AF.check_rotated(AF.rotated(ref, cos, sin, index, G), got)
        s3, f3 = AF.check_rotated(AF.rotated(cond, cos, sin, index, G), got)
        seen.update(s2, **{k + "_given_out": v for k, v in s3.items()})
        fails += f2 + [f + " (given the stored out)" for f in f3]
    else:
        s2, f2 = AR.check_conditioned(cond, got, fused=True, G=G)
        seen.update(s2)
        fails += f2
    return seen, fails


def _runs(case):
    """(G, rope form, packed) of every call the GPU test makes on a case."""
    for G in AF.groups_of(case):
        yield G, None, False
        if case.lens:
            yield G, None, True
        if case.S in AF.ROPE_S:
            yield G, "shared", False
            yield G, "batch", False
            yield G, "packed", True


def test_the_emulation_passes_every_check_on_every_new_case():
    worst = {}
    for case in TABLE_F:
        for G, rope, packed in _runs(case):
            seen, fails = _checks(case, AF.emulate(case, G, rope, packed), G, rope, packed)
            assert not fails, (case.name, G, rope, packed, fails)
            for k, v in seen.items():
                key = f"G{G} {k}"
                worst[key] = max(worst.get(key, 0.0), v)
    print("emulation, worst over table F: " + "  ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items())))
    for G in (2, 4):
        for k in ("out", "dq", "dk", "dv", "dq_given_out", "dk_given_out", "rope_dq", "rope_dk", "rope_dq_given_out", "rope_dk_given_out"):
            assert worst[f"G{G} {k}"] < 1.0, (G, k)


# (wrong evaluation, case, G, rope form, packed): the named case each one fails on
WRONG_ON = (
    ("block_never_added", "F-S768-w-1-nomask-pre", 4, None, False),
    ("block_never_added", "F-S1300-w-1-holes-plain", 4, None, False),
    ("last_partial_slab_dropped", "F-S768-w-1-nomask-plain", 2, None, False),
    ("last_partial_slab_dropped", "F-S1025-w-1-pad-pre", 4, None, True),
    ("block_added_twice", "F-S640-w-1-nomask-pre", 2, None, False),
    ("block_added_twice", "F-S1025-w-1-pad-plain", 4, None, False),
    ("slab_of_the_other_head", "F-S513-w-1-pad-pre", 2, None, False),
    ("slab_of_the_other_head", "F-S1300-w-1-holes-pre", 4, None, False),
    ("rope_forward_instead_of_inverse", "F-S513-w-1-pad-plain", 2, "shared", False),
    ("rope_row_of_batch_0", "F-S1025-w-1-pad-pre", 4, "batch", False),
    ("rope_row_of_batch_0", "F-S513-w-1-pad-plain", 2, "batch", False),
    ("rope_packed_row_restarts_per_sequence", "F-S513-w-1-pad-pre", 2, "packed", True),
    ("rope_packed_row_restarts_per_sequence", "F-S1025-w-1-pad-plain", 4, "packed", True),
)


def test_every_wrong_evaluation_is_named():
    assert {w for w, *_ in WRONG_ON} == set(AF.WRONG_FUSED) and len(AF.WRONG_FUSED) == 7
    runs = {(c.name, *r) for c in TABLE_F for r in _runs(c)}
    assert all((name, G, rope, packed) in runs for _, name, G, rope, packed in WRONG_ON)  # each is a call the GPU test makes


@pytest.mark.parametrize("wrong,name,G,rope,packed", WRONG_ON, ids=[f"{w}-{n}-G{g}" for w, n, g, _, _ in WRONG_ON])
def test_a_wrong_evaluation_fails(wrong, name, G, rope, packed):
    case = AF.BY_NAME[name]
    got = AF.emulate(case, G, rope, packed, wrong=wrong)
    ok = AF.emulate(case, G, rope, packed)
    assert not all(torch.equal(got[nm], ok[nm]) for nm in ("dq", "dk"))
    seen, fails = _checks(case, got, G, rope, packed)
    print(f"{wrong} on {name} G{G}: {fails[:3]}")
    assert fails
    if wrong.startswith("rope_row") or wrong.startswith("rope_packed"):
        # only rows whose table row differs are off: sequence 0 (positions from 0 either way) still passes on its own
        rot = AF.rotated(_ref(case, packed), *AF.rope_tables(case, rope), G)
        first = torch.zeros(case.B, case.S, dtype=torch.bool)
        first[0] = True
        assert not AF.check_rotated(rot, got, live=first)[1]


def test_the_table_reaches_the_seams_it_names():
    assert [c.S for c in TABLE_F[::2]] == [385, 513, 640, 768, 1025, 1300] and all(a.S == b.S and b.pre and not a.pre for a, b in zip(TABLE_F[::2], TABLE_F[1::2]))
    assert [c.B for c in TABLE_F[::2]] == [3, 3, 2, 3, 2, 5]
    sizes = [c.S for c in TABLE_F] + [S for S, _ in AR.CASES_G]
    assert {-(-S // 64) % 6 for S in sizes} == set(range(6))                 # every residue of the ring's unroll
    assert {-(-S // 64) for S in sizes} >= {5, 7, 8, 9, 10, 12, 17, 21}
    store, add = set(), set()
    for case in TABLE_F:
        for G in AF.groups_of(case):
            s, a = AF.launch_grids(case, G)
            store.add(s)
            add.update(a)
            assert len(a) == min(G, AF.key_blocks(case.S)) - 1
    for grids in (store, add):  # xcd_remap: below one workgroup per XCD, and a remainder
        assert any(g < 8 for g in grids) and any(g > 8 and g % 8 for g in grids) and any(g % 8 == 0 for g in grids), grids
    assert AF.slab_groups(513, 2) == [2, 1] and AF.slab_groups(768, 2) == [2, 1] and AF.slab_groups(768, 4) == [3]
    assert AF.slab_groups(1025, 2) == [2, 2, 1] and AF.slab_groups(1025, 4) == [4, 1]
    assert AF.slab_groups(1300, 2) == [2, 2, 2] and AF.slab_groups(1300, 4) == [4, 2]
    assert AF.groups_of(AF.BY_NAME["F-S385-w-1-pad-pre"]) == (2,) and all(AF.groups_of(c) == (2, 4) for c in TABLE_F if c.S > 512)
    groups = [g for c in TABLE_F for G in AF.groups_of(c) for g in AF.slab_groups(c.S, G)]
    assert {1, 2, 3, 4} <= set(groups)                                       # adds at positions 1, 2, 3; partial last groups
    assert max(len(AF.slab_groups(c.S, G)) for c in TABLE_F for G in AF.groups_of(c)) == 3  # the reduce sums three slabs
    assert AF.key_blocks(513) == 3 and 513 - 512 == 1 and 385 - 256 == 129    # a last key block of one key; a second of 129
    # the holes: five patterns, the fifth only the keys of ONE key block
    km = AR.key_mask(AF.BY_NAME["F-S1300-w-1-holes-pre"])
    assert km.shape == (5, 1300) and 0.6 < km[0].float().mean() < 0.8 and not km[1, 0] and not km[1, -1] and km[1].any()
    assert not km[2].any() and int((~km[3]).sum()) == 1 and not km[3, 1260] and torch.equal(torch.nonzero(km[4]).flatten(), torch.arange(512, 768))
    assert all(c.B * c.S <= 5 * 1300 for c in TABLE_F)
    # positions tell rows apart: batch b starts at 7 b, packed sequences too
    case = AF.BY_NAME["F-S513-w-1-pad-pre"]
    cos_b, _, idx_b = AF.rope_tables(case, "batch")
    cos_p, _, idx_p = AF.rope_tables(case, "packed")
    assert cos_b.shape == (3 * 513, 32) and cos_p.shape == (513 + 256 + 65, 32) and cos_b.dtype == torch.float32
    assert torch.equal(cos_b[idx_b[1, 5]], cos_b[idx_b[0, 12]]) and not torch.equal(cos_b[idx_b[1, 5]], cos_b[idx_b[0, 5]])
    assert torch.equal(cos_p[idx_p[2, 3]], cos_b[idx_b[2, 3]]) and int(idx_p[1, 0]) == 513 and int(idx_p[2, 64]) == 513 + 256 + 64


def test_the_row_subset_reference_is_the_full_reference_s_rows():
    for name in ("F-S385-w-1-pad-plain", "F-S513-w-1-pad-pre", "F-S1300-w-1-holes-pre"):
        case = AF.BY_NAME[name]
        S = case.S
        rows = torch.cat([torch.arange(64), torch.arange(64 * (S // 128), 64 * (S // 128) + 64), torch.arange(64 * ((S - 1) // 64), S)])
        full, sub = _ref(case), AR.reference(case, rows=rows)
        assert "dk" not in sub and "dv" not in sub["bound"]
        for nm in ("out", "lse", "dq", "dead", "nvis", "fused_unit"):
            assert torch.equal(sub[nm], full[nm][:, :, rows]), (name, nm)
        for nm in ("out", "dq"):
            assert torch.equal(sub["bound"][nm], full["bound"][nm][:, :, rows]), (name, nm)
        got = AF.emulate(case, 4)
        c_full, c_sub = AR.conditioned(case, got["out"]), AR.conditioned(case, got["out"][:, :, rows], rows=rows)
        assert torch.equal(c_sub["dq"], c_full["dq"][:, :, rows]) and torch.equal(AR.bound_fused_dq(c_sub, 4), AR.bound_fused_dq(c_full, 4)[:, :, rows])
        sub_got = {nm: got[nm][:, :, rows] for nm in ("out", "lse", "dq")}
        assert not AR.check_float64(sub, sub_got, fused=True, G=4, quantities=("out", "lse", "dq"))[1]


def test_the_long_case_s_row_subset_builds_nothing_s_by_s():
    """S = 5900 (24 key blocks: the length rule's G = 4): three query tiles against all keys, 140 rows in all."""
    case = AR.Case("F", AF.LONG_S, -1, None, True, False, False, 1)
    assert case.B == 1 and AF.key_blocks(case.S) == 24
    rows = AF.long_rows()
    assert len(rows) == 64 + 64 + 12 and int(rows[-1]) == AF.LONG_S - 1
    ref = AR.reference(case, rows=rows)
    assert ref["dq"].shape == (1, NH, len(rows), 64) and ref["lse"].shape == (1, NH, len(rows))


def test_the_bound_and_the_slab_sum_depend_on_g_as_counted():
    case = AF.BY_NAME["F-S1025-w-1-pad-pre"]
    ref = _ref(case)
    b2, b4 = AR.bound_fused_dq(ref, 2), AR.bound_fused_dq(ref, 4)
    assert torch.equal(b2, ref["bound_fused_dq"])  # G = 2 is the pair form's bound: it has not loosened
    assert torch.allclose(b2, ref["bound"]["dq"] + 2.0 * AR.U16 * AR.SCALE * _abs_ds_k(case) * AR.SECOND, rtol=1e-12, atol=0.0)
    assert torch.equal(b4, ref["bound"]["dq"] + 4.0 * ref["fused_unit"]) and torch.equal(b2, ref["bound"]["dq"] + 2.0 * ref["fused_unit"])
    assert bool((b4 > b2).all()) and bool((ref["fused_unit"] > 0).all())
    # the adds of a group are sequential bf16 adds from the stored first partial; at G = 2 that is the pair form, bit for bit
    g = torch.Generator().manual_seed(3)
    parts = [AR._bf(torch.randn(1, 2, 8, 64, generator=g)) for _ in range(6)]
    bf = AR._bf
    assert torch.equal(AR.fused_dq_sum(parts, 2), bf(parts[0] + parts[1]) + bf(parts[2] + parts[3]) + bf(parts[4] + parts[5]))
    assert torch.equal(AR.fused_dq_sum(parts[:5], 2), bf(parts[0] + parts[1]) + bf(parts[2] + parts[3]) + parts[4])
    want4 = bf(bf(bf(parts[0] + parts[1]) + parts[2]) + parts[3]) + bf(parts[4] + parts[5])
    assert torch.equal(AR.fused_dq_sum(parts, 4), want4)
    assert not torch.equal(want4, AR.fused_dq_sum(parts, 2))
    for name in ("F-S1300-w-1-holes-pre", "F-S1025-w-1-pad-plain"):
        c = AF.BY_NAME[name]
        e2 = AR.emulate(c, fused=True)
        assert torch.equal(e2["dq"], AR.emulate(c, fused=True, G=2)["dq"])
        e4 = AR.emulate(c, fused=True, G=4)
        assert not torch.equal(e4["dq"], e2["dq"]) and torch.equal(e4["dk"], e2["dk"]) and torch.equal(e4["dv"], e2["dv"])


def _abs_ds_k(case):
    """|dS||K| [B, NH, S, 64] in float64, restated from the reference's quantities."""
    x = AR.inputs(case)
    _, _, _, p = AR.softmax64(case, x)
    do = AR.heads(x["do"].double())
    out = p @ x["v"]
    dS = p * (do @ x["v"].transpose(-1, -2) - (do * out).sum(-1, keepdim=True))
    return dS.abs() @ x["k"].abs()


def test_the_rotation_is_row_kernel_refs_and_the_workspace_formula_is_sized_as_documented():
    from row_kernel_refs import rope_apply_ref

    case = AF.BY_NAME["F-S513-w-1-pad-plain"]
    ref = _ref(case)
    cos, sin, index = AF.rope_tables(case, "batch")
    qkv = torch.stack([ref["dq"].permute(0, 2, 1, 3), ref["dk"].permute(0, 2, 1, 3)], 2)  # [B, S, 2, NH, 64]
    want, _ = rope_apply_ref(qkv, cos.double()[index], sin.double()[index], inverse=True)
    assert torch.equal(AF.rotate_inverse(ref["dq"], cos, sin, index), want[:, :, 0].permute(0, 2, 1, 3))
    assert torch.equal(AF.rotate_inverse(ref["dk"], cos, sin, index), want[:, :, 1].permute(0, 2, 1, 3))
    back = AF.rotate_inverse(AF.rotate_inverse(ref["dq"], cos, sin, index), cos, sin, index, forward=True)
    assert (back - ref["dq"]).abs().max().item() < 1e-6  # (fp32 tables: cos^2 + sin^2 = 1 to fp32)
    assert AF.workspace_bytes(1, 64, 1) == 13 * 512 + 128 * 128 and AF.workspace_bytes(0, 64, 1) == 0
