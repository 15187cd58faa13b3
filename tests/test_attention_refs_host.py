"""tests/attention_refs.py on the CPU: the float64 reference agrees with the oracle, a torch fp32 emulation of the head-64 attention
kernels' documented arithmetic passes every check of tests/test_attention_d64_gpu.py on every case of the table (the proof that a
correct kernel fits the derived bounds; the worst error / bound per quantity is printed), wrong evaluations fail those same checks, and
the table reaches every branch of the band kernels' index arithmetic."""
import functools
import math

import pytest
import torch

import attention_refs as AR
from attention_refs import NH, SCALE, TABLE, TABLE_A, TABLE_C, TABLE_G, TABLE_P


@functools.lru_cache(maxsize=None)
def _ref(case):
    return AR.reference(case)


def _all_checks(case, got, fused=False, ref=None):
    """Every check the GPU test applies to one forward + backward -> (measured, failures)."""
    ref = ref or _ref(case)
    if case.probe:
        seen, fails = AR.check_probe(case, ref, got)
        return seen, fails + AR.check_exact(case, ref, got)
    seen, fails = AR.check_float64(ref, got, fused=fused)
    s2, f2 = AR.check_conditioned(AR.conditioned(case, got["out"]), got, fused=fused)
    return dict(seen, **s2), fails + f2 + AR.check_exact(case, ref, got)


def test_reference_agrees_with_the_oracle():
    from oracle import cm3p_oracle as O

    for case in (AR.BY_NAME["A-S300-w33-pad-plain"], AR.BY_NAME["A-S300-w0-pad-pre"], AR.BY_NAME["C-S300-w64-holes-plain"],
                 AR.BY_NAME["B-S65-w1-nomask-plain"], AR.BY_NAME["G-S257-w-1-pad-pre"]):
        x, ref = AR.inputs(case), _ref(case)
        km = AR.key_mask(case)
        allowed = O.attention_allowed(km.long() if km is not None else None, case.B, case.S, case.window if case.window >= 0 else None)
        if allowed is None:
            allowed = torch.ones(case.B, 1, case.S, case.S, dtype=torch.bool)
        assert torch.equal(allowed.expand(case.B, 1, case.S, case.S), AR.visible(case)), case.name
        o = O.sdpa(x["q"], x["k"], x["v"], allowed, SCALE, eager=True)  # (its softmax is fp32)
        assert (o - ref["out"]).abs().max().item() < 5e-6, case.name
        dead = ~allowed.any(-1).expand(-1, NH, -1)
        assert torch.equal(dead, ref["dead"]) and not ref["out"][dead].any() and bool((ref["lse"][dead] == float("-inf")).all())


def test_the_emulation_passes_every_check_on_every_case():
    worst = {}
    for case in TABLE + TABLE_P:
        runs = [(AR.emulate(case), False)]
        if case.table == "G" and not case.probe:
            runs.append((AR.emulate(case, fused=True), True))
        for got, fused in runs:
            seen, fails = _all_checks(case, got, fused)
            assert not fails, (case.name, fused, fails)
            for k, v in seen.items():
                key = ("fused " if fused and k.startswith("dq") else "") + ("probe " if case.probe else "") + k
                worst[key] = max(worst.get(key, 0.0), v)
    print("emulation, worst over the table: " + "  ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items())))
    for k in ("out", "dq", "dk", "dv", "fused dq", "dq_given_out", "dk_given_out", "probe out"):
        assert worst[k] < 1.0, (k, worst[k])


def test_the_emulation_with_dropout_passes():
    for w in (1, 33, 96):
        case = AR.BY_NAME[f"A-S300-w{w}-pad-pre"]
        keep = AR.bernoulli_keep(case, 0.1)
        ref = AR.reference(case, keep, 0.1)
        got = AR.emulate(case, keep, 0.1)
        seen, fails = AR.check_float64(ref, got)
        s2, f2 = AR.check_conditioned(AR.conditioned(case, got["out"], keep, 0.1), got)
        assert not fails + f2 + AR.check_exact(case, ref, got), (case.name, fails, f2)
        print(f"dropout {case.name}: " + "  ".join(f"{k}={v:.3g}" for k, v in dict(seen, **s2).items()))


def _caught(case, wrong):
    return bool(_all_checks(case, AR.emulate(case, wrong=wrong))[1])


@pytest.mark.parametrize("wrong", ["widen_right", "narrow_left"])
def test_a_window_edge_off_by_one_fails_at_every_window_of_table_a(wrong):
    """... where the mask differs (at window 299 / 300 a widened window is the same mask; a narrowed one still is at 300)."""
    for w in AR.WINDOWS_A:
        cases = [c for c in TABLE_A + TABLE_P if c.table == "A" and c.window == w]
        differs = not torch.equal(AR.wrong_visibility(cases[0], wrong), AR.visible(cases[0]))
        assert differs == {"widen_right": w < 299, "narrow_left": w < 300}[wrong], w
        if differs:
            assert any(_caught(c, wrong) for c in cases), (wrong, w)
            assert any(_caught(c, wrong) for c in cases if c.probe), (wrong, w, "count probe")


@pytest.mark.parametrize("wrong", ["drop_half_tile", "mask_ignored_last_tile", "ragged_keys", "dead_mean", "delta_split"])
def test_wrong_evaluations_fail(wrong):
    caught = [c.name for c in TABLE + TABLE_P if c.pre is False and _caught(c, wrong)]
    print(f"{wrong}: caught on {len(caught)} cases: {caught[:6]}")
    assert caught
    if wrong == "delta_split":  # only the check against the backward that takes delta from the stored out can see this one
        case = AR.BY_NAME[caught[0]]
        got = AR.emulate(case, wrong=wrong)
        assert not AR.check_float64(_ref(case), got)[1] and AR.check_conditioned(AR.conditioned(case, got["out"]), got)[1]


def test_the_table_reaches_every_branch_of_the_index_arithmetic():
    seen = {"fwd": set(), "dq": set(), "dkv": set()}
    other_window = {"fwd": set(), "dq": set(), "dkv": set()}
    for case in TABLE:
        if case.window < 0:
            continue
        for g, labels in AR.coverage(case).items():
            seen[g] |= labels
            if case.window != 64:
                other_window[g] |= labels
    for g in seen:
        need = AR.COVERAGE_REQUIRED[g] | AR.SWEEPS
        assert not need - seen[g], (g, sorted(need - seen[g]))
        assert not need - other_window[g], (g, "only at window 64", sorted(need - other_window[g]))
    # the eight-tile sweep of (449, 449) wraps the four-slot ring twice
    assert "sweep_more_than_4_tiles" in AR.coverage(AR.BY_NAME["B-S449-w449-nomask-plain"])["dq"]


def test_every_instance_is_reached_at_a_window_other_than_64():
    reached = set().union(*(AR.instances(c) for c in TABLE if c.window != 64))
    assert AR.ALL_INSTANCES <= reached, sorted(AR.ALL_INSTANCES - reached)
    assert "attn_fwd_g_kernel" in reached  # the pipelined forward, through table G


def test_the_count_probe_separates_neighbouring_counts():
    """out: the bound is below half of 1 / n, the change one key more or less makes to sum(+-1) / n, on every live row at the head dims
    whose sign bit (bit d mod 10 of the key index) has a period of at most 128 keys - the bits 7 .. 9 are constant over a 129-key window
    (out = +-1 there whatever the count) and carry no count.  lse: 1e-4 is below half of ln((n + 1) / n) for the largest n."""
    nmax = 0
    dims = (torch.arange(64) % 10) <= 6
    for case in TABLE_P:
        ref = _ref(case)
        nmax = max(nmax, int(ref["nvis"].max()))
        if 0 <= case.window <= AR.PROBE_OUT_MAX_WINDOW:
            live = ~ref["dead"]
            n = ref["nvis"][live].double()[:, None]
            assert int(n.max()) <= 2 * AR.PROBE_OUT_MAX_WINDOW + 1
            assert bool((AR.probe_out_bound(ref)[live][:, dims] < 0.5 / n).all()), case.name
    assert nmax == 300 and AR.PROBE_LSE_TOL < 0.5 * math.log((nmax + 1) / nmax)


def test_table_shapes():
    assert len(TABLE_A) == 38 and len(AR.TABLE_B) == 18 and len(TABLE_C) == 8 and len(TABLE_G) == 6
    assert all(c.B * c.S <= 4 * 449 for c in TABLE + TABLE_P)
    for w in AR.WINDOWS_C + AR.PROBE_WINDOWS:  # table C's sequence 2: one visible key or none
        km = AR._key_mask("C", 300, w, None)
        assert int(km[2].sum()) == (1 if w in AR.C_ONE_KEY_WINDOWS else 0) and not km[1, 0] and int((~km[3]).sum()) == 1
