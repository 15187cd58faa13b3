"""Compile-time checks of the kernels whose correctness depends on the emitted ISA (no GPU needed): the counted-vmcnt LDS-DMA rings
and the inline-asm MFMAs of gemm8p.hip, attention_fwd.hip and attention_bwd_fused.hip.  The checks live in
cm3p_amd/isa_check.py because cm3p_amd/build.py runs the same ones on every rebuild of these objects (a failed check fails the
build); here they run on every test run, plus a negative control that the checker really looks at the ring."""
import os

import pytest

from cm3p_amd import build, isa_check

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def isa():
    cache = {}

    def get(src):
        if src not in cache:
            cache[src] = isa_check.compile_isa(src, build.FLAGS + build.EXTRA_FLAGS.get(src, []))
        return cache[src]

    return get


@pytest.mark.parametrize("src", sorted(isa_check.CHECKS))
def test_isa_pattern(isa, src):
    isa_check.CHECKS[src](isa(src))


def test_gemm8p_checker_rejects_a_drained_ring(isa):
    """Negative control: the same ISA with the counted wait replaced by a drain, or with one more DMA in the loop, must fail."""
    text = isa("gemm8p.hip")
    with pytest.raises(isa_check.IsaCheckError):
        isa_check.check_gemm8p(text.replace("s_waitcnt vmcnt(6)", "s_waitcnt vmcnt(0)"))
    with pytest.raises(isa_check.IsaCheckError):
        isa_check.check_gemm8p(text.replace("s_waitcnt lgkmcnt(8)", "s_waitcnt lgkmcnt(12)"))


def test_fused_checker_rejects_a_spill(isa):
    text = isa("attention_bwd_fused.hip")
    with pytest.raises(isa_check.IsaCheckError):
        isa_check.check_attention_bwd_fused(text.replace(".vgpr_spill_count: 0", ".vgpr_spill_count: 3", 1))


def test_issue_cost_walk_of_the_attention_streams(isa):
    """tools/isa_gapcost.py prices every MFMA gap of a hand-placed stream (v_exp 8, v_cvt_pk_bf16_f32 8 - tools/ubench/mfma_cvt_dep.hip -,
    other VALU 4 ...).  Only what protects the kernels from regressing is asserted (r05 advisor: the earlier version also pinned the
    schedule's documented UNEVENNESS as lower bounds, so that any improvement - or a hipcc bump - would have failed the suite): one priced
    gap per MFMA of the loop body, and the issue cost per MFMA no higher than it is today.  What the walk shows beyond that (the share of
    near-empty and over-full gaps) is a report: `python tools/isa_gapcost.py`."""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_gapcost

    gaps, cyc = isa_gapcost.gap_costs(isa("attention_bwd_fused.hip"), "attn_bwd_fused_kernelILb1ELb0E", 480)
    per = [g for g, _ in gaps]
    assert len(per) == 480 and cyc == 32.0          # gap count == MFMA count of the six-tile ring body
    assert sum(per) / 480 <= 34.0                   # issue work per MFMA
    assert sum(max(32.0, g) for g in per) / 480 <= 43.0  # ... and as placed (a gap cannot be shorter than its MFMA)
    gaps, cyc = isa_gapcost.gap_costs(isa("attention_fwd.hip"), "attn_fwd_g_kernelILi4ELb0E", 256)
    per = [g for g, _ in gaps]
    assert len(per) in (256, 257) and sum(per) / 256 <= 52.0  # (the rotated loop opens with a partial gap)
