"""The tiled route of cm3p_gemm_f32 without a GPU: what the entry point refuses before any HIP call, that the C ABI did not move
(the route is a flag in `accumulate`, not a symbol), and which route kernels.gemm_f32 takes for the head's shapes."""
import ctypes
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cm3p_hip.h")
ERR_INVALID = -1
TILED = 2


def _entry():
    from cm3p_amd import _lib

    return _lib.load().cm3p_gemm_f32


def _host_ptr():
    raw = ctypes.create_string_buffer(4096 + 16)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)  # (never dereferenced: the refusal comes first)


@pytest.mark.parametrize("strides", [(2, 3, 8, 1), (8, 1, 2, 3), (2, 2, 2, 2), (0, 8, 8, 1), (8, 1, 16, 2)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_tiled_flag_refuses_an_operand_without_a_unit_stride(strides, accumulate):
    raw, p = _host_ptr()
    a_rs, a_cs, b_rs, b_cs = strides
    assert _entry()(p, p, p, 4, 4, 8, a_rs, a_cs, b_rs, b_cs, 4, 1.0, TILED | accumulate, None) == ERR_INVALID


@pytest.mark.parametrize("accumulate", [4, 5, 6, 7, 8, 1 << 16, -1, -2])
def test_bits_above_the_flag_are_refused(accumulate):
    raw, p = _host_ptr()
    assert _entry()(p, p, p, 4, 4, 8, 8, 1, 8, 1, 4, 1.0, accumulate, None) == ERR_INVALID


def test_the_flag_does_not_loosen_the_other_requirements():
    raw, p = _host_ptr()
    f = _entry()
    assert f(None, p, p, 4, 4, 8, 8, 1, 8, 1, 4, 1.0, TILED, None) == ERR_INVALID
    assert f(p, p, p, 4, 4, 0, 8, 1, 8, 1, 4, 1.0, TILED, None) == ERR_INVALID
    assert f(p, p, p, 4, 4, 8, 8, 1, 8, 1, 3, 1.0, TILED, None) == ERR_INVALID  # ldc < N


def test_header_binding_and_abi_are_unchanged_in_count_and_version():
    from cm3p_amd import _lib

    text = open(HEADER).read()
    assert int(re.search(r"^#define CM3P_GEMM_F32_TILED (\d+)", text, re.M).group(1)) == TILED == _lib.GEMM_F32_TILED
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"^#define CM3P_ABI_VERSION (\d+)", text, re.M).group(1)) == _lib.ABI_VERSION >= 19
    declared = re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text)
    assert len(declared) == len(set(declared)) == len(_lib.SIGNATURES) == 88 and set(declared) == set(_lib.SIGNATURES)
    assert not any("tiled" in n for n in declared)  # (the one entry point added since is cm3p_gemm_route, ABI 20)
    assert len(_lib.SIGNATURES["cm3p_gemm_f32"]) == 14  # no new parameter


def test_isa_check_is_registered_for_the_head():
    from cm3p_amd import isa_check

    assert "head.hip" in isa_check.CHECKS


# (M, N, K, a_strides, b_strides) -> tiled?  The shape list of the gathered-variation head at N = 8 ranks, b = 32, V = 256, P = 512,
# H_meta = 256 (profiles/gemm_f32_tiled.txt has both routes' times for each), the b x b head and its projection, and two problems
# below kernels.GEMM_F32_TILED_MIN_OUTPUTS = 1024 outputs (the local head at b = 32).  The tiled route was faster or equal at every
# measured shape (behind the flag the entry point takes small tiles and k by 64 for few outputs), so the threshold only keeps the
# smallest, launch-bound problems on the 16 x 16 kernel.
ROUTES = [
    ("logits, metadata direction", 8192, 256, 512, (512, 1), (512, 1), True),
    ("logits, beatmap direction", 32, 65536, 512, (512, 1), (512, 1), True),
    ("d metadata rows", 8192, 512, 256, (256, 1), (1, 512), True),
    ("d gathered beatmaps", 256, 512, 8192, (1, 256), (1, 512), True),
    ("d beatmap rows (k = N b V)", 32, 512, 65536, (65536, 1), (1, 512), True),
    ("d gathered metadata", 65536, 512, 32, (1, 65536), (1, 512), True),
    ("projection", 8192, 512, 256, (256, 1), (256, 1), True),
    ("projection, d input", 8192, 256, 512, (512, 1), (1, 256), True),
    ("projection, d weight", 512, 256, 8192, (1, 512), (1, 256), True),
    ("local b x b head", 32, 32, 512, (512, 1), (512, 1), True),
    ("local head, projection of 32 rows", 32, 512, 768, (768, 1), (768, 1), True),
    ("local head, b = 8", 8, 8, 512, (512, 1), (512, 1), False),
    ("classifier head, 16 rows x 10 labels", 16, 10, 512, (512, 1), (512, 1), False),
]


@pytest.fixture
def stubbed(monkeypatch):
    """kernels.gemm_f32 with the device call recorded instead of made."""
    from cm3p_amd import kernels as K

    calls = []
    monkeypatch.setattr(K, "ptr", lambda t, dtype=None: 0)
    monkeypatch.setattr(K, "call", lambda name, *args, tag=None, work=None: calls.append((name, args, tag, work)))
    return K, calls


def _run(K, calls, M, N, Kd, a_s, b_s, **kw):
    calls.clear()
    x = torch.empty(1)
    K.gemm_f32(x, x, M, N, Kd, a_s, b_s, out=x, **kw)
    (name, args, tag, work), = calls
    assert name == "cm3p_gemm_f32" and work == 2.0 * M * N * Kd
    flags = args[12]
    assert tag == K.GEMM_F32_TAGS[bool(flags & TILED)] and flags & ~3 == 0
    return flags


@pytest.mark.parametrize("what,M,N,Kd,a_s,b_s,tiled", ROUTES, ids=[r[0] for r in ROUTES])
def test_default_route_of_the_head_shapes(stubbed, what, M, N, Kd, a_s, b_s, tiled):
    K, calls = stubbed
    assert K.GEMM_F32_TAGS[False] != K.GEMM_F32_TAGS[True]
    assert bool(_run(K, calls, M, N, Kd, a_s, b_s) & TILED) == tiled
    assert _run(K, calls, M, N, Kd, a_s, b_s, accumulate=True) & 1 == 1
    assert _run(K, calls, M, N, Kd, a_s, b_s, accumulate=False) & 1 == 0


def test_the_constants_force_either_route_and_strides_without_a_unit_stay_off_the_tiled_kernel(stubbed, monkeypatch):
    K, calls = stubbed
    monkeypatch.setattr(K, "GEMM_F32_TILED_MIN_OUTPUTS", 0)
    for _, M, N, Kd, a_s, b_s, _ in ROUTES:
        assert _run(K, calls, M, N, Kd, a_s, b_s) & TILED
    assert _run(K, calls, 1, 1, 1, (1, 1), (1, 1)) & TILED
    assert not _run(K, calls, 64, 64, 64, (128, 2), (64, 1)) & TILED  # no unit stride in A: the entry point would refuse the flag
    assert not _run(K, calls, 64, 64, 64, (64, 1), (2, 128)) & TILED
    monkeypatch.setattr(K, "GEMM_F32_TILED_MIN_OUTPUTS", 1 << 62)
    for _, M, N, Kd, a_s, b_s, _ in ROUTES:
        assert not _run(K, calls, M, N, Kd, a_s, b_s) & TILED
