"""Typed Python wrappers over the C ABI: allocate outputs (torch = device memory only), launch, return tensors.

No autograd here and no torch compute ops: everything numerical happens inside libcm3p_hip.so.
"""
from __future__ import annotations

import math
import os
import struct
from typing import Optional

import torch

from . import _lib
from ._lib import ADD_A_BF16, BF16, GEMM_F32_TILED, POOL_PACKED, EPI_BF16, EPI_BF16_GEGLU_BWD, EPI_BF16_GEGLU_FWD, EPI_BF16_RESID, EPI_F32, EPI_F32_RESID, F32, call, dt, ptr, query, stream

Tensor = torch.Tensor

# C-ABI calls whose `work` is algorithmic BYTES (HBM-bound row-wise kernels); every other `work` is matmul FLOPs
_lib.HBM_BOUND_TAGS.update({"cm3p_layernorm_fwd", "cm3p_layernorm_bwd", "cm3p_geglu_fwd", "cm3p_geglu_bwd", "attn_bwd_prep_kernel [global]",
                            "attn_bwd_dq_reduce_kernel [global]", "attn_bwd_prep_kernel [global, varlen]", "attn_bwd_dq_reduce_kernel [global, varlen]"})


def _empty(shape, dtype, like: Tensor) -> Tensor:
    return torch.empty(shape, dtype=dtype, device=like.device)


# ------------------------------------------------------------------------------------------------ norms
def layernorm_fwd(x: Tensor, weight: Tensor, eps: float, want_f32: bool, want_bf16: bool, want_stats: bool = True):
    """x [rows, H] fp32|bf16 -> (y_f32|None, y_bf16|None, mean|None, rstd|None)."""
    rows, H = x.shape
    y32 = _empty((rows, H), torch.float32, x) if want_f32 else None
    y16 = _empty((rows, H), torch.bfloat16, x) if want_bf16 else None
    mean = _empty((rows,), torch.float32, x) if want_stats else None
    rstd = _empty((rows,), torch.float32, x) if want_stats else None
    call("cm3p_layernorm_fwd", ptr(x), dt(x), ptr(weight, torch.float32), ptr(y32), ptr(y16), ptr(mean, torch.float32), ptr(rstd, torch.float32), rows, H, eps, stream(),
         work=float(rows) * H * (x.element_size() + (4 if want_f32 else 0) + (2 if want_bf16 else 0)))
    return y32, y16, mean, rstd


def layernorm_bwd(dy: Tensor, x: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor],
                  want_bf16: bool, inplace: bool = True, bf16_only: bool = False):
    """-> (dx_f32 = dres + LN'(dy), dx_bf16|None, dw[H]).  With `inplace` dx_f32 overwrites dres.  x and dres: fp32 or bf16 rows.
    bf16_only (the bf16 residual stream of a training step): -> (None, bf16(dres + LN'(dy)), dw) - the sum is formed in fp32 and
    rounded once, where a bf16 torch model rounds LN'(dy) and the sum separately; with `inplace` it overwrites a bf16 dres."""
    rows, H = x.shape
    if bf16_only:
        dx32 = None
        dx16 = dres if (inplace and dres is not None and dres.dtype == torch.bfloat16) else _empty((rows, H), torch.bfloat16, x)
    else:
        dx32 = dres if (inplace and dres is not None and dres.dtype == torch.float32) else _empty((rows, H), torch.float32, x)
        dx16 = _empty((rows, H), torch.bfloat16, x) if want_bf16 else None
    nblk = query("cm3p_layernorm_bwd_blocks", rows)
    part = _empty((nblk, H), torch.float32, x)
    dw = _empty((H,), torch.float32, x)
    call("cm3p_layernorm_bwd", ptr(dy), dt(dy), ptr(x), dt(x), ptr(weight, torch.float32), ptr(mean, torch.float32), ptr(rstd, torch.float32), ptr(dres),
         dt(dres) if dres is not None else F32, ptr(dx32), ptr(dx16), ptr(part), ptr(dw), rows, H, stream(),
         work=float(rows) * H * (dy.element_size() + x.element_size() + (dres.element_size() if dres is not None else 0)
                                 + (4 if dx32 is not None else 0) + (2 if dx16 is not None else 0)))
    return dx32, dx16, dw


def embed_ln_fwd(ids: Tensor, table: Tensor, weight: Tensor, eps: float, slot: Optional[Tensor] = None,
                 override: Optional[Tensor] = None, want_bf16: bool = False, want_f32: bool = True):
    """-> (y_f32|None, y_bf16|None, mean, rstd); at least one of want_f32 / want_bf16 (bf16 alone: the bf16 residual stream)."""
    T = ids.numel()
    H = table.shape[1]
    if not (want_f32 or want_bf16):
        raise ValueError("embed_ln_fwd: no output requested")
    y32 = _empty((T, H), torch.float32, table) if want_f32 else None
    y16 = _empty((T, H), torch.bfloat16, table) if want_bf16 else None
    mean = _empty((T,), torch.float32, table)
    rstd = _empty((T,), torch.float32, table)
    call("cm3p_embed_ln_fwd", ptr(ids, torch.int64), ptr(table), dt(table), ptr(slot, torch.int32), ptr(override), dt(override) if override is not None else F32,
         ptr(weight, torch.float32), ptr(y32), ptr(y16), ptr(mean, torch.float32), ptr(rstd, torch.float32), T, H, eps, table.shape[0], stream())
    return y32, y16, mean, rstd


def embed_ln_bwd(dy: Tensor, ids: Tensor, table: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor, padding_idx: int,
                 slot: Optional[Tensor] = None, override: Optional[Tensor] = None, want_table_grad: bool = True):
    """dy [T, H] fp32 or bf16 (the gradient that leaves a bf16 residual stream) -> (d_table|None, d_override|None, dw), all fp32."""
    T = ids.numel()
    V, H = table.shape
    if want_table_grad and T > 0 and os.environ.get("CM3P_EMBED_BWD", "sorted") != "atomic":
        return _embed_ln_bwd_sorted(dy, ids, table, weight, mean, rstd, padding_idx, slot, override)
    d_table = torch.zeros((V, H), dtype=torch.float32, device=table.device) if want_table_grad else None
    # zeros, not empty: in unpadded execution placeholder tokens at masked positions are dropped from the packed rows, their
    # rows are never written by the kernel, and zero is their true gradient
    d_ovr = torch.zeros(override.shape, dtype=torch.float32, device=table.device) if override is not None else None
    nblk = query("cm3p_layernorm_bwd_blocks", T)
    part = _empty((nblk, H), torch.float32, table)
    dw = _empty((H,), torch.float32, table)
    call("cm3p_embed_ln_bwd", ptr(dy), dt(dy), ptr(ids, torch.int64), ptr(table), dt(table), ptr(slot, torch.int32), ptr(override),
         dt(override) if override is not None else F32, ptr(weight, torch.float32), ptr(mean, torch.float32), ptr(rstd, torch.float32), ptr(d_table), ptr(d_ovr), ptr(part), ptr(dw),
         T, H, padding_idx, V, stream())
    return d_table, d_ovr, dw


def _embed_ln_bwd_sorted(dy, ids, table, weight, mean, rstd, padding_idx, slot, override):
    """The embedding backward without atomics (cm3p_embed_ln_bwd_sorted): tokens are visited in id order, every sum has a fixed
    order (reproducible bit for bit, which the atomic kernel is not) and tokens that share an id do not serialise on one row.
    The sort and the run numbering are a counting sort in six small launches (cm3p_token_order; no host read)."""
    T = ids.numel()
    V, H = table.shape
    dev = table.device
    chunk = query("cm3p_embed_ln_bwd_sorted_chunk")
    flat = ids.reshape(-1).to(torch.int64).contiguous()
    order, run_of = token_order(flat, V, chunk)
    R = min(T, V + 3 + T // chunk)
    run_rows = _empty((R, H), torch.float32, table)
    run_ids = torch.empty((R,), dtype=torch.int64, device=dev)
    d_table = _empty((V, H), torch.float32, table)
    d_ovr = torch.zeros(override.shape, dtype=torch.float32, device=dev) if override is not None else None
    nblk = (-(-T // chunk) + 3) // 4
    part = _empty((nblk, H), torch.float32, table)
    dw = _empty((H,), torch.float32, table)
    call("cm3p_embed_ln_bwd_sorted", ptr(dy), dt(dy), ptr(flat, torch.int64), ptr(order, torch.int64), ptr(run_of, torch.int32), ptr(table), dt(table),
         ptr(slot, torch.int32), ptr(override), dt(override) if override is not None else F32, ptr(weight, torch.float32),
         ptr(mean, torch.float32), ptr(rstd, torch.float32), ptr(d_table), ptr(d_ovr), ptr(run_rows), ptr(run_ids, torch.int64),
         ptr(part), ptr(dw), T, H, padding_idx, V, stream())
    return d_table, d_ovr, dw


def token_order(flat_ids: Tensor, V: int, chunk: int):
    """-> (order [T] int64: token indices by ascending clamp(id, -1, V), ties in token order; run_of [T] int32: run number of every
    sorted position, a new run where the id changes and at every multiple of `chunk`).  cm3p_token_order (a counting sort on the
    device); vocabularies beyond its histogram (V + 2 > 12288) and CM3P_TOKEN_ORDER=torch take the torch.sort / cumsum route that
    defines the result."""
    T = flat_ids.numel()
    dev = flat_ids.device
    n_ws = query("cm3p_token_order_workspace_ints", T, V) if os.environ.get("CM3P_TOKEN_ORDER", "hip") != "torch" else 0
    if n_ws > 0:
        order = torch.empty((T,), dtype=torch.int64, device=dev)
        run_of = torch.empty((T,), dtype=torch.int32, device=dev)
        ws = torch.empty((n_ws,), dtype=torch.int32, device=dev)
        call("cm3p_token_order", ptr(flat_ids, torch.int64), T, V, ptr(order, torch.int64), ptr(run_of, torch.int32), ptr(ws, torch.int32), stream())
        return order, run_of
    key = flat_ids.clamp(-1, V)  # ids outside the table get no gradient: two keys for all of them bound the number of runs
    sk, order = torch.sort(key, stable=True)
    start = torch.ones(T, dtype=torch.bool, device=dev)
    if T > 1:
        start[1:] = sk[1:] != sk[:-1]
    start |= (torch.arange(T, device=dev) % chunk) == 0
    return order, (torch.cumsum(start, 0) - 1).to(torch.int32)


def audio_slots(ids: Tensor, audio_token_id: int):
    T = ids.numel()
    slot = torch.empty((T,), dtype=torch.int32, device=ids.device)
    count = torch.empty((1,), dtype=torch.int32, device=ids.device)
    call("cm3p_audio_slots", ptr(ids, torch.int64), T, audio_token_id, ptr(slot, torch.int32), ptr(count), stream())
    return slot, count


# ------------------------------------------------------------------------------------------------ GEMM
def _wgrad_splits(M: int, N: int, K: int) -> int:
    return query("cm3p_gemm_wgrad_splits", M, N, K)


_GEMM_KERNELS = ("gemm_bf16_kernel", "gemm256_kernel", "gemm8p_kernel")  # the kernel numbers of cm3p_gemm_route
_GEMM_RING, _GEMM_REBAL = 2, 4
EPI_ROPE, EPI_GEGLU = 3, 6  # internal epilogue numbers cm3p_gemm_route accepts (csrc/common.h)


def _gemm_tag(M: int, N: int, K: int, a_kc, b_kc, epilogue, split_k: int, lda: Optional[int] = None, ldb: Optional[int] = None,
              rope_cols: int = 0, kernel: Optional[int] = None) -> str:
    """Profiler tag = the kernel instance the library's own routing rule names (cm3p_gemm_route; csrc/gemm.hip cm3p_gemm_route_of),
    spelled like rocprof.  Asked on every call: CM3P_GEMM_IMPL may change inside a process.  lda / ldb default to the unpadded
    operands'; kernel: the entry point's own kernel where it has only one (cm3p_gemm_geglu)."""
    lda = (K if a_kc else M) if lda is None else lda
    ldb = (K if b_kc else N) if ldb is None else ldb
    code = query("cm3p_gemm_route", M, N, K, lda, ldb, int(bool(a_kc)), int(bool(b_kc)), epilogue, split_k, rope_cols, 0)
    if code < 0:
        raise _lib.Cm3pHipError(f"cm3p_gemm_route: no bf16 GEMM kernel takes M {M} N {N} K {K} a_kc {a_kc} b_kc {b_kc} epilogue {epilogue} split_k {split_k}")
    kernel = code & 3 if kernel is None else kernel
    b2s = lambda v: "true" if v else "false"
    tail = f", {b2s(code & _GEMM_REBAL)}" if kernel == _GEMM_RING else ""
    return f"{_GEMM_KERNELS[kernel]}<{b2s(a_kc)}, {b2s(b_kc)}, {epilogue}{tail}>"


def gemm(a: Tensor, b: Tensor, M: int, N: int, K: int, a_kc: bool, b_kc: bool, epilogue: int,
         resid: Optional[Tensor] = None, out: Optional[Tensor] = None, split_k: int = 1) -> Tensor:
    """C[m,n] = sum_k A(m,k) B(n,k) (+resid).  a/b bf16, row-major 2-D; see include/cm3p_hip.h for the layouts."""
    lda, ldb = a.shape[1], b.shape[1]
    if out is None:
        out = _empty((M, N), torch.bfloat16 if epilogue in (EPI_BF16, EPI_BF16_RESID) else torch.float32, a)
    ws = _empty((split_k, M, N), torch.float32, a) if split_k > 1 else None
    call("cm3p_gemm_bf16", ptr(a), ptr(b), ptr(out), ptr(resid), M, N, K, lda, ldb, N, int(a_kc), int(b_kc), epilogue, split_k,
         ptr(ws), stream(), tag=_gemm_tag(M, N, K, a_kc, b_kc, epilogue, split_k, lda, ldb), work=2.0 * M * N * K)
    return out


def linear_fwd(x: Tensor, w: Tensor, resid: Optional[Tensor] = None) -> Tensor:
    """x [T,K] bf16, w [N,K] bf16 -> x w^T as bf16, or resid + x w^T: fp32 for an fp32 resid, bf16(resid + bf16(x w^T)) for a
    bf16 one (the bf16 residual stream of forward-only calls, CM3P_EPI_BF16_RESID)."""
    T, K = x.shape
    N = w.shape[0]
    if resid is None:
        return gemm(x, w, T, N, K, True, True, EPI_BF16)
    return gemm(x, w, T, N, K, True, True, EPI_BF16_RESID if resid.dtype == torch.bfloat16 else EPI_F32_RESID, resid)


def linear_fwd_f32(x: Tensor, w: Tensor) -> Tensor:
    """x [T,K] bf16, w [N,K] bf16 -> x w^T as fp32 (the attention output projection when out_drop follows it)."""
    T, K = x.shape
    return gemm(x, w, T, w.shape[0], K, True, True, EPI_F32, None)


SOFTMAX_Q_SCALE = 64 ** -0.5 * 1.4426950408889634  # scale * log2(e) for head_dim 64: what q_prescaled attention expects in q


def qkv_linear_rope(x: Tensor, w: Tensor, cos: Tensor, sin: Tensor, S: int, per_batch: bool, q_scale: float = 1.0) -> Tensor:
    """Fused Wqkv projection + RoPE on the q and k thirds: x [T,H] bf16, w [3H,H] bf16 -> qkv [T,3H] bf16 (rotated).
    q_scale multiplies the rotated q third in fp32 before its bf16 rounding (SOFTMAX_Q_SCALE for `prescaled` attention)."""
    T, Kd = x.shape
    N = w.shape[0]
    out = _empty((T, N), torch.bfloat16, x)
    call("cm3p_qkv_gemm_rope", ptr(x), ptr(w), ptr(out), T, N, Kd, ptr(cos, torch.float32), ptr(sin, torch.float32), S, int(per_batch), 2 * N // 3, float(q_scale), stream(),
         tag=_gemm_tag(T, N, Kd, True, True, EPI_ROPE, 1, rope_cols=2 * N // 3), work=2.0 * T * N * Kd)
    return out


def linear_dgrad(dy: Tensor, w: Tensor, w_t: Optional[Tensor] = None) -> Tensor:
    """dy [T,N] bf16, w [N,K] bf16 -> dx [T,K] bf16 = dy w.  With w_t = w^T [K,N] (cast_bf16_with_transpose) the contraction index
    is contiguous in both operands - the faster form of the 256 x 256 kernel (same products, same accumulation order)."""
    T, N = dy.shape
    K = w.shape[1]
    if w_t is not None:
        return gemm(dy, w_t, T, K, N, True, True, EPI_BF16)
    return gemm(dy, w, T, K, N, True, False, EPI_BF16)


def linear_wgrad(dy: Tensor, x: Tensor) -> Tensor:
    """dy [T,N] bf16, x [T,K] bf16 -> dW [N,K] fp32 = dy^T x (split-K over tokens, deterministic combine)."""
    T, N = dy.shape
    K = x.shape[1]
    return gemm(dy, x, N, K, T, False, False, EPI_F32, split_k=_wgrad_splits(N, K, T))


def row_block_rows(n: int, H: int, I: int) -> int:
    """How many rows a block of n token rows is filled up to (with zero rows) for the GEMMs of a layer's row block: a multiple of 8,
    the GEMMs' constraint - or of 64 where the library's routing rule (cm3p_gemm_route) then gives the block's largest
    token-contraction GEMM, the weight gradient dWi [2 I, H] = dh^T xn2, a 256 x 256 kernel that it does not get otherwise (those
    kernels take the contraction in 64-deep tiles)."""
    n8, n64 = (n + 7) // 8 * 8, (n + 63) // 64 * 64
    if n8 == n64:
        return n8

    def kernel(T):
        code = query("cm3p_gemm_route", 2 * I, H, T, 2 * I, H, 0, 0, EPI_F32, _wgrad_splits(2 * I, H, T), 0, 0)
        return code & 3 if code >= 0 else 0

    return n64 if kernel(n64) > kernel(n8) else n8


def cast_bf16(x: Tensor) -> Tensor:
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    call("cm3p_cast_f32_bf16", ptr(x, torch.float32), ptr(y), x.numel(), stream())
    return y


def cast_bf16_with_transpose(x: Tensor):
    """fp32 [rows, cols] -> (bf16 [rows, cols], bf16 [cols, rows]) in one pass."""
    rows, cols = x.shape
    y = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    yt = torch.empty((cols, rows), dtype=torch.bfloat16, device=x.device)
    call("cm3p_cast_f32_bf16_t", ptr(x, torch.float32), ptr(y), ptr(yt), rows, cols, stream())
    return y, yt


def cast_bf16_with_transpose_many(ws: list, geglu_rows: Optional[list] = None) -> list:
    """[fp32 2-D weights, extents multiples of 8] -> [(bf16 copy, bf16 transpose)] in ONE launch (cm3p_cast_f32_bf16_t_multi): the values
    of cast_bf16_with_transpose per matrix.  One bf16 allocation holds all copies; the address table travels with one small H2D copy.
    geglu_rows: one flag per matrix - a flagged Wi [2I, K] gets its bf16 copy in the row order of geglu_interleave_index (what
    linear_geglu_fwd reads) instead of the canonical one; its transpose is the canonical W^T either way."""
    if not ws:
        return []
    geglu_rows = geglu_rows or [False] * len(ws)
    dev = ws[0].device
    numel = sum(w.numel() for w in ws)
    store = torch.empty((2 * numel,), dtype=torch.bfloat16, device=dev)
    base, out, table, off, blocks = store.data_ptr(), [], [], 0, 0
    for w, il in zip(ws, geglu_rows):
        rows, cols = w.shape
        if il and rows % 64:
            raise ValueError(f"cast_bf16_with_transpose_many: interleaved GeGLU rows need 2I a multiple of 64, got {rows}")
        y = store[off:off + rows * cols].view(rows, cols)
        yt = store[off + rows * cols:off + 2 * rows * cols].view(cols, rows)
        table += [w.data_ptr(), base + 2 * off, base + 2 * (off + rows * cols), -rows if il else rows, cols, blocks]
        out.append((y, yt))
        off += 2 * rows * cols
        blocks += (-(-rows // 64)) * (-(-cols // 64))
    # The table goes through PINNED host memory: torch's caching host allocator keeps a pinned block out of circulation until the copy
    # that reads it has run, so the asynchronous upload cannot race the temporary's release (r04 advisor: from a pageable temporary that
    # is freed on return, HIP is free to pin and copy lazily - the kernel would then dereference garbage addresses).  A blocking copy would
    # be safe too but makes the host wait for the stream, and the host runs two to three steps ahead of the GPU (tools/host_lead.py).
    tab = torch.tensor(table, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    call("cm3p_cast_f32_bf16_t_multi", ptr(tab, torch.int64), len(ws), blocks, stream(), work=8.0 * numel)
    return out


# ------------------------------------------------------------------------------------------------ low-rank adapters (include/cm3p_lora.h)
LORA_RANKS = (8, 16, 32, 64)
_lib.HBM_BOUND_TAGS.update({"cm3p_lora_merge_cast_multi", "cm3p_lora_grad"})


def lora_merge_cast_many(entries: list) -> list:
    """[(W fp32 [N, K], A fp32 [r, K], B fp32 [N, r], s, geglu_rows)] -> [(bf16(W + s B A), its transpose)] in ONE launch
    (cm3p_lora_merge_cast_multi): cast_bf16_with_transpose_many with the adapter folded in before the one rounding (fp32 sum over r).
    geglu_rows: the copy of a Wi gets the row order of geglu_interleave_index; its transpose stays canonical."""
    if not entries:
        return []
    dev = entries[0][0].device
    numel = sum(e[0].numel() for e in entries)
    store = torch.empty((2 * numel,), dtype=torch.bfloat16, device=dev)
    base, out, table, off, blocks = store.data_ptr(), [], [], 0, 0
    for w, a, b, s, il in entries:
        rows, cols = w.shape
        r = a.shape[0]
        if r not in LORA_RANKS or tuple(a.shape) != (r, cols) or tuple(b.shape) != (rows, r):
            raise ValueError(f"lora_merge_cast_many: W {tuple(w.shape)} needs A [r, {cols}] and B [{rows}, r] with r in {LORA_RANKS}; got {tuple(a.shape)}, {tuple(b.shape)}")
        if rows % 8 or cols % 8 or (il and rows % 64):
            raise ValueError(f"lora_merge_cast_many: extents must be multiples of 8 (2I a multiple of 64 for interleaved GeGLU rows), got {rows} x {cols}")
        for t in (w, a, b):
            ptr(t, torch.float32)  # (GPU, contiguous, fp32: the kernel reads raw addresses)
        y = store[off:off + rows * cols].view(rows, cols)
        yt = store[off + rows * cols:off + 2 * rows * cols].view(cols, rows)
        s_bits = int.from_bytes(struct.pack("<f", float(s)), "little")
        table += [w.data_ptr(), a.data_ptr(), b.data_ptr(), s_bits, -rows if il else rows, cols, r, base + 2 * off, base + 2 * (off + rows * cols), blocks]
        out.append((y, yt))
        off += 2 * rows * cols
        blocks += (-(-rows // 64)) * (-(-cols // 64))
    # (pinned host memory: see cast_bf16_with_transpose_many; the entry point validates the host copy before it launches)
    host = torch.tensor(table, dtype=torch.int64).pin_memory()
    tab = host.to(dev, non_blocking=True)
    call("cm3p_lora_merge_cast_multi", host.data_ptr(), ptr(tab, torch.int64), len(entries), stream(),
         work=float(sum(8 * e[0].numel() + 4 * (e[1].numel() + e[2].numel()) for e in entries)))
    return out


def _ptr_rows(t: Tensor):
    """Device address of a 2-D bf16 operand whose rows may be pitched (unit stride inside a row)."""
    if not t.is_cuda or t.dim() != 2 or t.dtype != torch.bfloat16 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise _lib.Cm3pHipError("cm3p_amd kernels: a pitched operand must be a 2-D bf16 GPU tensor with unit stride inside a row")
    p = _lib._DevPtr(t.data_ptr())
    p.dev = t.device.index
    return p


def lora_grad_row_block(T: int) -> int:
    """Tokens per row block of lora_grad's token reduction (host-only query)."""
    return query("cm3p_lora_grad_row_block", T)


def lora_grad(x: Tensor, dy: Tensor, A: Tensor, B: Tensor, s: float):
    """Adapter gradients of one adapted weight (cm3p_lora_grad): x [T, K] bf16, dy [T, N] bf16 (rows may be pitched), A [r, K] fp32,
    B [N, r] fp32 -> (dA [r, K], dB [N, r]) fp32 = (s v^T x, s dy^T u) with u = bf16(x bf16(A)^T), v = bf16(dy bf16(B)); ordered sums."""
    T, K = x.shape
    N, r = B.shape
    if r not in LORA_RANKS or tuple(A.shape) != (r, K) or dy.shape[0] != T or dy.shape[1] != N:
        raise ValueError(f"lora_grad: x {tuple(x.shape)}, dy {tuple(dy.shape)}, A {tuple(A.shape)}, B {tuple(B.shape)}: need A [r, K], B [N, r], r in {LORA_RANKS}")
    nbytes = query("cm3p_lora_grad_workspace_bytes", T, K, N, r)
    if nbytes < 0:
        raise ValueError(f"lora_grad: unsupported shape T {T} K {K} N {N} r {r} (T >= 1; K, N multiples of 8)")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    dA = _empty((r, K), torch.float32, x)
    dB = _empty((N, r), torch.float32, x)
    call("cm3p_lora_grad", _ptr_rows(x), x.stride(0), _ptr_rows(dy), dy.stride(0), ptr(A, torch.float32), ptr(B, torch.float32), float(s),
         ptr(dA), ptr(dB), T, K, N, r, ptr(ws), nbytes, stream(), work=4.0 * T * (K + N))
    return dA, dB


def add_f32(a: Tensor, b: Tensor, want_bf16: bool = False, inplace: bool = True):
    """fp32 a: -> (a + b as fp32, its bf16 rounding | None).  bf16 a (the bf16 residual stream of a training step): -> (None,
    bf16(a + b)), the sum formed in fp32 and rounded once; b fp32 or bf16 either way."""
    if a.dtype == torch.bfloat16:
        y16 = a if inplace else torch.empty_like(a)
        call("cm3p_add_f32", ptr(a), ptr(b), dt(b) | ADD_A_BF16, None, ptr(y16), a.numel(), stream())
        return None, y16
    y32 = a if inplace else torch.empty_like(a)
    y16 = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device) if want_bf16 else None
    call("cm3p_add_f32", ptr(a), ptr(b), dt(b), ptr(y32), ptr(y16), a.numel(), stream())
    return y32, y16


# ------------------------------------------------------------------------------------------------ RoPE / attention
def rope_table(position_ids: Tensor, inv_freq: Tensor):
    n = position_ids.numel()
    half = inv_freq.numel()
    cos = torch.empty((n, half), dtype=torch.float32, device=inv_freq.device)
    sin = torch.empty((n, half), dtype=torch.float32, device=inv_freq.device)
    call("cm3p_rope_table", ptr(position_ids, torch.int64), n, ptr(inv_freq, torch.float32), half, ptr(cos, torch.float32), ptr(sin, torch.float32), stream())
    return cos, sin


def rope_apply_(qkv: Tensor, cos: Tensor, sin: Tensor, B: int, S: int, nh: int, per_batch: bool, inverse: bool = False):
    call("cm3p_rope_apply", ptr(qkv), ptr(cos, torch.float32), ptr(sin, torch.float32), B, S, nh, S if per_batch else 0, int(inverse), stream())
    return qkv


def gemm8p_set_grid(workgroups: int) -> None:
    """Workgroups per launch of the big-shape GEMM kernel (0: one per CU, the default; > CU count: the surplus starts as CUs come free -
    what bench.py selects next to RCCL).  Process-wide; include/cm3p_hip.h: cm3p_gemm8p_set_grid."""
    rc = _lib.load().cm3p_gemm8p_set_grid(int(workgroups))
    if rc != 0:
        raise ValueError(f"cm3p_gemm8p_set_grid({workgroups}) -> {rc}")


def gemm8p_get_grid() -> int:
    return int(_lib.load().cm3p_gemm8p_get_grid())


def _drop_abi(drop: Optional[tuple]) -> tuple:
    """drop = (thr, seed, layer) or None -> (what the entry point's name gains, the arguments it takes before the stream in the ABI's
    order, how the kernels' template argument list ends as rocprofv3 prints it)."""
    if drop is None:
        return "", (), ">"
    thr, seed, layer = drop
    return "_dropout", (layer, thr, seed), ", DropCfg>"


def _attn_fwd_name(window: int, prescaled: bool, masked: bool, S: int, nh: int, targs_end: str = ">") -> str:
    """The forward kernel a call lands on, as rocprofv3 names it.  The routing is the library's (cm3p_attn_fwd_impl: global layers with
    pre-scaled q run the pipelined kernel of csrc/attention_fwd.hip unless the sequence is too long for its 32-bit row offsets, and
    never with dropout); this function only spells the answer (r05 advisor: it used to re-derive the rule)."""
    if targs_end == ">" and query("cm3p_attn_fwd_impl", S, nh, window, int(prescaled)):
        return "attn_fwd_g_kernel<4, " + ("true>" if masked else "false>")
    return "attn_fwd_kernel<1, %s, " + ("true" if window >= 0 else "false") + targs_end


def attn_fwd(qkv: Tensor, key_mask: Optional[Tensor], B: int, S: int, nh: int, window: int, scale: float, prescaled: bool = False,
             drop: Optional[tuple] = None):
    """prescaled: the q third already carries scale * log2(e) (qkv_linear_rope(..., q_scale=SOFTMAX_Q_SCALE)).
    drop = (thr, seed, layer): attention-probability dropout (the band kernels at every window)."""
    out = torch.empty((B * S, nh * 64), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, nh, S), dtype=torch.float32, device=qkv.device)
    keys = S if window < 0 else min(S, 2 * window + 1)
    sfx, drop_args, targs_end = _drop_abi(drop)
    call("cm3p_attn_fwd" + sfx, ptr(qkv), ptr(out), ptr(lse, torch.float32), ptr(key_mask, torch.uint8), B, S, nh, window, scale, int(prescaled),
         *drop_args, stream(), tag=_attn_tag(_attn_fwd_name(window, prescaled, key_mask is not None, S, nh, targs_end), window, prescaled),
         work=4.0 * B * nh * S * keys * 64)
    return out, lse


# ---- head sizes other than 64 (csrc/attention_generic.hip: plain fp32 kernels for 16 / 32 so that every reference configuration runs;
# 96 / 128 leave through the same entry points for the matrix-core kernels of csrc/attention_hd.hip)
HD_MFMA_SIZES = (96, 128)  # no dropout form, padded batches only


def attn_generic_supported(head_dim: int) -> bool:
    return bool(query("cm3p_attn_generic_supported", int(head_dim)))


def _attn_hd_prof(names: tuple, products: int, B: int, S: int, nh: int, hd: int, window: int) -> dict:
    """tag / work of a head_dim 96 / 128 launch (the 16 / 32 kernels are not on any measured path and carry none).  `work` is the
    algorithmic count of attn_fwd / attn_bwd (`products` matmuls of 2 B nh S keys hd; recomputed scores are not credited)."""
    if hd not in HD_MFMA_SIZES:
        return {}
    keys = S if window < 0 else min(S, 2 * window + 1)
    return dict(tag=_attn_tag(" + ".join(f"{n}<{hd}>" for n in names), window, False), work=2.0 * products * B * nh * S * keys * hd)


def rope_apply_generic_(qkv: Tensor, cos: Tensor, sin: Tensor, B: int, S: int, nh: int, hd: int, per_batch: bool, inverse: bool = False):
    call("cm3p_rope_apply_generic", ptr(qkv, torch.bfloat16), ptr(cos, torch.float32), ptr(sin, torch.float32), B, S, nh, hd, S if per_batch else 0, int(inverse), stream())
    return qkv


def attn_fwd_generic(qkv: Tensor, key_mask: Optional[Tensor], B: int, S: int, nh: int, hd: int, window: int, scale: float,
                     drop: Optional[tuple] = None):
    """drop = (thr, seed, layer): attention-probability dropout (the rule of attn_fwd's)."""
    out = torch.empty((B * S, nh * hd), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, nh, S), dtype=torch.float32, device=qkv.device)
    sfx, drop_args, _ = _drop_abi(drop)
    prof = {} if drop is not None else _attn_hd_prof(("attn_hd_fwd_kernel",), 2, B, S, nh, hd, window)
    call("cm3p_attn_fwd_generic" + sfx, ptr(qkv, torch.bfloat16), ptr(out), ptr(lse, torch.float32), ptr(key_mask, torch.uint8), B, S, nh, hd, window, scale,
         *drop_args, stream(), **prof)
    return out, lse


def attn_bwd_generic(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, key_mask: Optional[Tensor], B: int, S: int, nh: int, hd: int,
                     window: int, scale: float, drop: Optional[tuple] = None) -> Tensor:
    """-> dqkv with the q / k thirds still in the ROTATED frame (rope_apply_generic_(..., inverse=True) finishes them)."""
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    sfx, drop_args, _ = _drop_abi(drop)
    # one call, two kernels; attn_bwd's count: 2 x forward
    prof = {} if drop is not None else _attn_hd_prof(("attn_hd_dq_kernel", "attn_hd_dkv_kernel"), 4, B, S, nh, hd, window)
    call("cm3p_attn_bwd_generic" + sfx, ptr(qkv, torch.bfloat16), ptr(out, torch.bfloat16), ptr(dout, torch.bfloat16), ptr(lse, torch.float32), ptr(delta),
         ptr(dqkv), ptr(key_mask, torch.uint8), B, S, nh, hd, window, scale, *drop_args, stream(), **prof)
    return dqkv


def attn_probs(qkv: Tensor, lse: Tensor, key_mask: Optional[Tensor], B: int, S: int, nh: int, window: int, scale: float, prescaled: bool = False) -> Tensor:
    """output_attentions: the probabilities [B, nh, S, S] fp32 of one layer, from qkv and the lse attn_fwd stored (inspection path)."""
    probs = torch.empty((B, nh, S, S), dtype=torch.float32, device=qkv.device)
    call("cm3p_attn_probs", ptr(qkv), ptr(lse, torch.float32), ptr(key_mask, torch.uint8), ptr(probs), B, S, nh, window, scale, int(prescaled), stream())
    return probs


ATTN_BWD_DQ, ATTN_BWD_DKV = 1, 2  # stages of cm3p_attn_bwd (include/cm3p_hip.h)


def _attn_tag(fmt: str, window: int, prescaled: bool, varlen: bool = False) -> str:
    """Profiler tag = the kernel's name as rocprofv3 prints it (the template argument is the q_prescaled mode) + which layers it
    served: "attn_bwd_fused_kernel<true, false> [global]".  bench.py matches the part before " [" against the rocprof / PMC rows."""
    name = fmt % ("true" if prescaled else "false") if "%s" in fmt else fmt
    return f"{name} [{'global' if window < 0 else 'local'}{', varlen' if varlen else ''}]"


ATTN_BWD_FUSED_PREP, ATTN_BWD_FUSED_MAIN, ATTN_BWD_FUSED_REDUCE = 1, 2, 4  # stages of cm3p_attn_bwd_fused
ATTN_BWD_FUSED_MAIN_EVEN, ATTN_BWD_FUSED_MAIN_ODD = 8, 16  # the storing launch of _MAIN (first key block of every slab group) and all adding ones
ATTN_BWD_FUSED_MAIN_ADD1 = 32  # the adding launches one by one: _ADD1 << (p - 1) = position p of the group
_fused_ws: dict = {}  # (device index, stream) -> byte tensor: the fused backward's workspace, grown on demand, shared by all layers


_other_caches: list = []  # dicts other modules keep device memory in (encoder.py: the forward-only bf16 weight copies)


def release_workspaces() -> None:
    """Drop the cached workspaces of the fused attention backward (1.65 GB at C2, 3.3 GB at C4 per device and stream) and the bf16
    weight copies kept for forward-only calls: call it between jobs of different sequence lengths if the memory matters; the next
    call allocates what it needs."""
    _fused_ws.clear()
    for c in _other_caches:
        c.clear()


def _attn_bwd_fused(qkv, out, dout, lse, key_mask, cu, B, S, total, nh, scale, rope, per_batch, prescaled) -> Tensor:
    dqkv = torch.empty_like(qkv)
    cos, sin = rope if rope is not None else (None, None)
    need = query("cm3p_attn_bwd_fused_workspace_bytes", B, S, nh)
    key = (qkv.device.index, torch.cuda.current_stream(qkv.device).cuda_stream)
    ws = _fused_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _fused_ws[key] = torch.empty(need, dtype=torch.uint8, device=qkv.device)
    varlen = cu is not None
    rows = total if varlen else B * S
    fl = 2.0 * B * nh * S * S * 64  # one S x S x 64 product per (batch, head); SURVEY.md 8(d) credits four to the backward
    nkb = -(-S // 256)  # 256-key blocks; G of them share a dQ slab: the first of each group stores (one launch), the others add (G - 1 launches)
    G = query("cm3p_attn_bwd_fused_slab_group", S)  # (the C side derives it, CM3P_FUSED_SLAB_GROUP included: one parse, one answer)
    n_store = -(-nkb // G)
    slabs = float(need) * 2.0 / G  # (the workspace is sized for groups of 2)
    # one C call per launch, so that every profiler tag is ONE kernel (one rocprof row): the storing launch, then the adding launches
    adds = [(ATTN_BWD_FUSED_MAIN_ADD1 << (p - 1), "attn_bwd_fused_kernel<%s, true>", 4.0 * fl * len(range(p, nkb, G)) / nkb)
            for p in range(1, min(G, nkb))]
    for stage, name, work in (
        (ATTN_BWD_FUSED_PREP, "attn_bwd_prep_kernel", 2.0 * rows * nh * 64 * 2 + 12.0 * rows * nh),
        (ATTN_BWD_FUSED_MAIN_EVEN, "attn_bwd_fused_kernel<%s, false>", 4.0 * fl * n_store / nkb),
        *adds,
        (ATTN_BWD_FUSED_REDUCE, "attn_bwd_dq_reduce_kernel", slabs + rows * nh * 64 * 2.0),
    ):
        call("cm3p_attn_bwd_fused", ptr(qkv), ptr(out), ptr(dout), ptr(lse, torch.float32), ptr(dqkv), ptr(key_mask, torch.uint8),
             ptr(cu, torch.int32), B, S, total if varlen else 0, nh, scale, ptr(cos, torch.float32), ptr(sin, torch.float32),
             S if (per_batch and not varlen) else 0, stage, int(prescaled), ptr(ws), ws.numel(), stream(),
             tag=_attn_tag(name, -1, prescaled, varlen), work=None if varlen else work)  # (packed rows: S is only the longest sequence)
    return dqkv


def attn_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, key_mask: Optional[Tensor], B: int, S: int, nh: int,
             window: int, scale: float, rope: Optional[tuple] = None, per_batch: bool = False, prescaled: bool = False,
             drop: Optional[tuple] = None) -> Tensor:
    """rope = (cos, sin): also applies the inverse rotary rotation to dq / dk (backward of the fused Wqkv+RoPE GEMM).
    Global layers (window < 0) run the five-product kernel of csrc/attention_bwd_fused.hip; sliding-window layers - and, with dropout,
    every layer - the band kernels of csrc/attention.hip, issued as two C calls so that each has its own profiler tag (one rocprof row
    per tag).  `work` is the algorithmic count of SURVEY.md section 8(d) (backward = 2 x forward = four matmuls: dQ is the dq kernel's,
    dP / dV / dK the dkv kernel's); the scores each kernel recomputes are not credited."""
    if drop is None and window < 0:
        return _attn_bwd_fused(qkv, out, dout, lse, key_mask, None, B, S, 0, nh, scale, rope, per_batch, prescaled)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    keys = S if window < 0 else min(S, 2 * window + 1)
    cos, sin = rope if rope is not None else (None, None)
    sfx, drop_args, targs_end = _drop_abi(drop)
    for stage, name, products in ((ATTN_BWD_DQ, "attn_bwd_dq_kernel<%s", 1), (ATTN_BWD_DKV, "attn_bwd_dkv_kernel<%s", 3)):
        call("cm3p_attn_bwd" + sfx, ptr(qkv), ptr(out), ptr(dout), ptr(lse, torch.float32), ptr(delta), ptr(dqkv), ptr(key_mask, torch.uint8), B, S, nh,
             window, scale, ptr(cos, torch.float32), ptr(sin, torch.float32), S if per_batch else 0, stage, int(prescaled), *drop_args, stream(),
             tag=_attn_tag(name + targs_end, window, prescaled), work=None if drop is not None else 2.0 * products * B * nh * S * keys * 64)
    return dqkv


def attn_fwd_varlen(qkv: Tensor, cu: Tensor, B: int, max_s: int, nh: int, window: int, scale: float, prescaled: bool = False,
                    drop: Optional[tuple] = None):
    """Packed sequences: qkv [total, 3, nh, 64], cu int32 [B+1] -> out [total, nh*64], lse [nh, total]."""
    total = qkv.shape[0]
    out = torch.empty((total, nh * 64), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((nh, total), dtype=torch.float32, device=qkv.device)
    sfx, drop_args, targs_end = _drop_abi(drop)
    call("cm3p_attn_fwd" + sfx + "_varlen", ptr(qkv), ptr(out), ptr(lse, torch.float32), ptr(cu, torch.int32), B, max_s, total, nh, window, scale,
         int(prescaled), *drop_args, stream(), tag=_attn_tag(_attn_fwd_name(window, prescaled, False, max_s, nh, targs_end), window, prescaled, True))
    return out, lse


def attn_bwd_varlen(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, cu: Tensor, B: int, max_s: int, nh: int, window: int,
                    scale: float, rope: Optional[tuple] = None, prescaled: bool = False, drop: Optional[tuple] = None) -> Tensor:
    """rope = (cos, sin) per packed token [total, 32]: also applies the inverse rotation to dq / dk."""
    if drop is None and window < 0:
        return _attn_bwd_fused(qkv, out, dout, lse, None, cu, B, max_s, qkv.shape[0], nh, scale, rope, False, prescaled)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    cos, sin = rope if rope is not None else (None, None)
    sfx, drop_args, targs_end = _drop_abi(drop)
    for stage, name in ((ATTN_BWD_DQ, "attn_bwd_dq_kernel<%s"), (ATTN_BWD_DKV, "attn_bwd_dkv_kernel<%s")):
        call("cm3p_attn_bwd" + sfx + "_varlen", ptr(qkv), ptr(out), ptr(dout), ptr(lse, torch.float32), ptr(delta), ptr(dqkv), ptr(cu, torch.int32), B,
             max_s, qkv.shape[0], nh, window, scale, ptr(cos, torch.float32), ptr(sin, torch.float32), stage, int(prescaled), *drop_args, stream(),
             tag=_attn_tag(name + targs_end, window, prescaled, True))
    return dqkv


# ---- single-query attention for the pooled CLS row (include/cm3p_attn_row.h, csrc/attention_row.hip) ---------------------------------
_lib.HBM_BOUND_TAGS.update({"attn_row_fwd_kernel", "attn_row_bwd_kernel"})  # one pass over K and V; the backward also writes all of dqkv


def attn_row_fwd(qkv: Tensor, key_mask: Optional[Tensor], cu: Optional[Tensor], B: int, S: int, nh: int, window: int, scale: float,
                 prescaled: bool = False):
    """Attention of query position 0 of every sequence.  qkv [B * S, 3 * nh * 64] (or the packed rows [total, ...] with their int32
    cu_seqlens, S = max_seqlen, no key mask) -> out [B, nh * 64] bf16, lse [B, nh] fp32."""
    total = qkv.shape[0] if cu is not None else 0
    out = torch.empty((B, nh * 64), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, nh), dtype=torch.float32, device=qkv.device)
    keys = S if window < 0 else min(S, window + 1)
    call("cm3p_attn_row_fwd", ptr(qkv, torch.bfloat16), ptr(out), ptr(lse, torch.float32), ptr(key_mask, torch.uint8), ptr(cu, torch.int32), B, S, total,
         nh, window, scale, int(prescaled), stream(), tag="attn_row_fwd_kernel", work=2.0 * B * nh * keys * 128)
    return out, lse


def attn_row_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, key_mask: Optional[Tensor], cu: Optional[Tensor], B: int, S: int, nh: int,
                 window: int, scale: float, rope: Optional[tuple] = None, per_batch: bool = False, prescaled: bool = False) -> Tensor:
    """-> dqkv in qkv's full layout, every element written: the q third is zero off the query rows.  rope = (cos, sin): also applies the
    inverse rotary rotation to dq / dk (per-token tables in the packed form)."""
    total = qkv.shape[0] if cu is not None else 0
    dqkv = torch.empty_like(qkv)
    cos, sin = rope if rope is not None else (None, None)
    rows = total if cu is not None else B * S
    call("cm3p_attn_row_bwd", ptr(qkv, torch.bfloat16), ptr(out, torch.bfloat16), ptr(dout, torch.bfloat16), ptr(lse, torch.float32), ptr(dqkv),
         ptr(key_mask, torch.uint8), ptr(cu, torch.int32), B, S, total, nh, window, scale, ptr(cos, torch.float32), ptr(sin, torch.float32),
         S if (per_batch and cu is None) else 0, int(prescaled), stream(), tag="attn_row_bwd_kernel", work=5.0 * rows * nh * 128)
    return dqkv


# ---- attention for a list of query rows (include/cm3p_attn_qrows.h, csrc/attention_qrows.hip) ------------------------------------------
def attn_qrows_fwd(qkv: Tensor, qrows: Tensor, qcu: Tensor, qmax: int, key_mask: Optional[Tensor], cu: Optional[Tensor], B: int, S: int, nh: int,
                   window: int, scale: float, prescaled: bool = False):
    """Attention of the listed query rows against all keys.  qkv [B * S, 3 * nh * 64] (or the packed rows [total, ...] with their int32
    cu_seqlens, S = max_seqlen, no key mask); qrows int32 [n] ascending global rows, qcu int32 [B + 1] their split by sequence, qmax the
    largest per-sequence count -> out [n, nh * 64] bf16, lse [nh, n] fp32, compact in list order."""
    n = qrows.numel()
    out = torch.empty((n, nh * 64), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((nh, n), dtype=torch.float32, device=qkv.device)
    if n == 0:
        return out, lse
    keys = S if window < 0 else min(S, 2 * window + 1)
    call("cm3p_attn_qrows_fwd", ptr(qkv, torch.bfloat16), ptr(out), ptr(lse, torch.float32), ptr(key_mask, torch.uint8), ptr(cu, torch.int32),
         ptr(qrows, torch.int32), ptr(qcu, torch.int32), n, qmax, B, S, qkv.shape[0], nh, window, scale, int(prescaled), stream(),
         tag="attn_qrows_fwd_kernel", work=2.0 * 2.0 * n * nh * keys * 64)
    return out, lse


def attn_qrows_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, qrows: Tensor, qcu: Tensor, qmax: int, key_mask: Optional[Tensor],
                   cu: Optional[Tensor], B: int, S: int, nh: int, window: int, scale: float, rope: Optional[tuple] = None, per_batch: bool = False,
                   prescaled: bool = False) -> Tensor:
    """-> dqkv in qkv's full layout, every element written: the q third is zero off the listed rows, dk / dv sum over the listed queries.
    rope = (cos, sin): also applies the inverse rotary rotation to dq / dk (per-token tables in the packed form)."""
    n = qrows.numel()
    dqkv = torch.empty_like(qkv)
    cos, sin = rope if rope is not None else (None, None)
    keys = S if window < 0 else min(S, 2 * window + 1)
    live = n > 0
    call("cm3p_attn_qrows_bwd", ptr(qkv, torch.bfloat16), ptr(out, torch.bfloat16) if live else None, ptr(dout, torch.bfloat16) if live else None,
         ptr(lse, torch.float32) if live else None, ptr(dqkv), ptr(key_mask, torch.uint8), ptr(cu, torch.int32), ptr(qrows, torch.int32) if live else None,
         ptr(qcu, torch.int32), n, qmax, B, S, qkv.shape[0], nh, window, scale, ptr(cos, torch.float32), ptr(sin, torch.float32),
         S if (per_batch and cu is None) else 0, int(prescaled), stream(), tag="attn_qrows_bwd_kernel", work=2.0 * 8.0 * n * nh * keys * 64)
    return dqkv


def _rows_as_f32(src: Tensor) -> Tensor:
    """bf16 rows [n, H] (H even) as fp32 rows [n, H / 2] of the same bits: the row copies below move them unchanged."""
    return src.view(torch.float32) if src.dtype == torch.bfloat16 else src


def gather_rows(src: Tensor, idx: Tensor) -> Tensor:
    """src [R, H] fp32 or bf16, idx int64 [n] -> [n, H] of src's dtype (the row selection of _unpad_cm3p_input)."""
    s32 = _rows_as_f32(src)
    out = torch.empty((idx.numel(), s32.shape[1]), dtype=torch.float32, device=src.device)
    if idx.numel() == 0:  # no row selected (every position masked): an empty tensor has no address to hand to the entry point
        return out.view(src.dtype)
    call("cm3p_gather_rows_f32", ptr(s32), ptr(idx, torch.int64), ptr(out), idx.numel(), s32.shape[1], stream())
    return out.view(src.dtype)


def scatter_rows(src: Tensor, idx: Tensor, rows: int) -> Tensor:
    """src [n, H] fp32 or bf16 -> [rows, H] of src's dtype with row idx[i] = src[i] and zeros elsewhere (_pad_cm3p_output)."""
    s32 = _rows_as_f32(src)
    out = torch.zeros((rows, s32.shape[1]), dtype=torch.float32, device=src.device)
    if idx.numel() == 0:  # nothing to place: all rows stay zero (see gather_rows)
        return out.view(src.dtype)
    call("cm3p_scatter_rows_f32", ptr(s32), ptr(idx, torch.int64), ptr(out), idx.numel(), s32.shape[1], stream())
    return out.view(src.dtype)


# ------------------------------------------------------------------------------------------------ MLP pieces
def geglu_fwd(h: Tensor) -> Tensor:
    T, I2 = h.shape
    g = torch.empty((T, I2 // 2), dtype=torch.bfloat16, device=h.device)
    call("cm3p_geglu_fwd", ptr(h), ptr(g), T, I2 // 2, stream(), work=6.0 * T * (I2 // 2))
    return g


def gemm_geglu_supported(T: int, I: int, Kd: int) -> bool:
    """Whether the Wi projection of this shape runs fused with GeGLU: cm3p_gemm_geglu's shape rule (the ring's big shapes), and the
    library's route names the ring (it does not under CM3P_GEMM_IMPL=256)."""
    code = query("cm3p_gemm_route", T, 2 * I, Kd, Kd, Kd, 1, 1, EPI_GEGLU, 1, 0, 0)
    return code >= 0 and (code & 3) == _GEMM_RING


def geglu_interleave_index(I: int, device) -> Tensor:
    """Row order of the interleaved Wi copy cm3p_gemm_geglu reads: row 64 q + r <- Wi row 32 q + r (r < 32) or I + 32 q + r - 32."""
    n = torch.arange(2 * I, device=device)
    r = n % 64
    j = (n // 64) * 32 + r % 32
    return torch.where(r < 32, j, I + j)


def gemm_geglu(x: Tensor, w_interleaved: Tensor) -> Tensor:
    """x [T,K] bf16, interleaved Wi [2I,K] bf16 -> gelu_erf(x Wi[:I]^T) * (x Wi[I:]^T) as bf16 [T,I] in one kernel (forward-only)."""
    T, Kd = x.shape
    I = w_interleaved.shape[0] // 2
    a = _empty((T, I), torch.bfloat16, x)
    call("cm3p_gemm_geglu", ptr(x), ptr(w_interleaved), ptr(a), T, I, Kd, stream(),
         tag=_gemm_tag(T, 2 * I, Kd, True, True, EPI_GEGLU, 1, kernel=_GEMM_RING), work=2.0 * T * 2 * I * Kd)
    return a


def mlp_geglu_fused_supported(T: int, I: int, H: int) -> bool:
    """Whether a training step's MLP of this shape takes the fused pair linear_geglu_fwd / linear_dgrad_geglu_bwd: the library's route
    (cm3p_gemm_route) names the ring for both calls - the Wi projection [T, H] -> [T, 2I] and the Wo2 input gradient [T, H] -> [T, I]."""
    fwd = query("cm3p_gemm_route", T, 2 * I, H, H, H, 1, 1, EPI_BF16_GEGLU_FWD, 1, 0, 0)
    bwd = query("cm3p_gemm_route", T, I, H, H, H, 1, 1, EPI_BF16_GEGLU_BWD, 1, 0, 0)
    return fwd >= 0 and (fwd & 3) == _GEMM_RING and bwd >= 0 and (bwd & 3) == _GEMM_RING


def linear_geglu_fwd(x: Tensor, w_interleaved: Tensor):
    """x [T,K] bf16, interleaved Wi [2I,K] bf16 (geglu_interleave_index) -> (h' [T,2I], a [T,I]) in one kernel: h' = x Wi^T with
    its columns in the order of the weight rows (linear_fwd's h permuted by geglu_interleave_index) and a = geglu_fwd(h), bit for bit.
    The Wi GEMM of a training step; linear_dgrad_geglu_bwd reads h'."""
    T, Kd = x.shape
    N = w_interleaved.shape[0]
    h = _empty((T, N), torch.bfloat16, x)
    a = _empty((T, N // 2), torch.bfloat16, x)
    call("cm3p_gemm_bf16", ptr(x), ptr(w_interleaved), ptr(h), None, T, N, Kd, Kd, Kd, N, 1, 1, EPI_BF16_GEGLU_FWD, 1, ptr(a), stream(),
         tag=_gemm_tag(T, N, Kd, True, True, EPI_BF16_GEGLU_FWD, 1), work=2.0 * T * N * Kd)
    return h, a


def linear_dgrad_geglu_bwd(dy: Tensor, w_t: Tensor, h_interleaved: Tensor) -> Tensor:
    """dy [T,H] bf16, w_t = Wo2^T [I,H] bf16, h' [T,2I] of linear_geglu_fwd -> dh [T,2I] bf16 in CANONICAL column order =
    geglu_bwd(linear_dgrad(dy, Wo2, w_t), h), bit for bit, in one kernel: the bf16 dg exists only in the GEMM's store phase."""
    T, Kd = dy.shape
    I = w_t.shape[0]
    dh = torch.empty_like(h_interleaved)
    call("cm3p_gemm_bf16", ptr(dy), ptr(w_t), ptr(dh), ptr(h_interleaved), T, I, Kd, Kd, Kd, 2 * I, 1, 1, EPI_BF16_GEGLU_BWD, 1, None, stream(),
         tag=_gemm_tag(T, I, Kd, True, True, EPI_BF16_GEGLU_BWD, 1), work=2.0 * T * I * Kd)
    return dh


def geglu_bwd(dg: Tensor, h: Tensor) -> Tensor:
    dh = torch.empty_like(h)
    call("cm3p_geglu_bwd", ptr(dg), ptr(h), ptr(dh), h.shape[0], h.shape[1] // 2, stream(), work=10.0 * h.shape[0] * (h.shape[1] // 2))
    return dh


# ------------------------------------------------------------------------------------------------ dropout (csrc/dropout_rng.h)
SITE_EMBED, SITE_ATTN_PROBS, SITE_ATTN_OUT, SITE_MLP = 0, 1, 2, 3


def dropout_threshold(p: float) -> int:
    """thr = round(p * 65536) of the RNG contract: an element is kept iff its 16-bit draw is >= thr."""
    return int(math.floor(float(p) * 65536.0 + 0.5))


def dropout_scale(thr: int) -> float:
    """The survivors' factor 65536 / (65536 - thr) as the kernels hold it (fp32); 0 when nothing survives."""
    return 0.0 if thr >= 65536 else float(torch.tensor(65536.0) / torch.tensor(float(65536 - thr)))


def _drop_rows(S: int, cu: Optional[Tensor]):
    """Row layout arguments of the element sites: padded rows of S positions, or the packed batch of cu_seqlens."""
    return (S, None, 0) if cu is None else (S, ptr(cu, torch.int32), cu.numel() - 1)


def dropout_f32(x: Tensor, thr: int, seed: int, layer: int, site: int, S: int, cu: Optional[Tensor] = None, resid: Optional[Tensor] = None,
                bf16_only: bool = False) -> Tensor:
    """[resid +] x o Z on [rows, H] fp32 (also the backward: dy o Z); bf16_only: the bf16 result alone (a GEMM operand)."""
    rows, H = x.shape
    y = torch.empty(x.shape, dtype=torch.bfloat16 if bf16_only else torch.float32, device=x.device)
    call("cm3p_dropout_f32", ptr(x, torch.float32), ptr(resid, torch.float32), None if bf16_only else ptr(y), ptr(y) if bf16_only else None, rows, H,
         *_drop_rows(S, cu), layer, site, thr, seed, stream())
    return y


def geglu_fwd_dropout(h: Tensor, thr: int, seed: int, layer: int, S: int, cu: Optional[Tensor] = None) -> Tensor:
    T, I2 = h.shape
    g = torch.empty((T, I2 // 2), dtype=torch.bfloat16, device=h.device)
    call("cm3p_geglu_fwd_dropout", ptr(h, torch.bfloat16), ptr(g), T, I2 // 2, *_drop_rows(S, cu), layer, thr, seed, stream())
    return g


def geglu_bwd_dropout(dg: Tensor, h: Tensor, thr: int, seed: int, layer: int, S: int, cu: Optional[Tensor] = None) -> Tensor:
    dh = torch.empty_like(h)
    call("cm3p_geglu_bwd_dropout", ptr(dg, torch.bfloat16), ptr(h, torch.bfloat16), ptr(dh), h.shape[0], h.shape[1] // 2, *_drop_rows(S, cu),
         layer, thr, seed, stream())
    return dh


def dropout_keep(n2: int, n1: int, n0: int, layer: int, site: int, thr: int, seed: int, device) -> Tensor:
    """The contract's keep mask (uint8 [n2, n1, n0]) of one (layer, site): element sites (sequences, positions, features)."""
    keep = torch.empty((n2, n1, n0), dtype=torch.uint8, device=device)
    call("cm3p_dropout_keep", ptr(keep), n2, n1, n0, layer, site, thr, seed, stream())
    return keep


def philox4x32_10_host(ctr, key):
    """Philox4x32-10 on the host (no GPU): ctr uint32 [n, 4], key uint32 [n, 2] (numpy) -> uint32 [n, 4]."""
    import numpy as np

    c = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
    k = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
    if c.shape[0] != k.shape[0]:
        raise ValueError("one key per counter")
    out = np.empty_like(c)
    _lib._check(query("cm3p_philox4x32_10_host", c.ctypes.data, k.ctypes.data, out.ctypes.data, c.shape[0]), "cm3p_philox4x32_10_host")
    return out


def gelu_fwd(x: Tensor) -> Tensor:
    y = torch.empty_like(x)
    call("cm3p_gelu_fwd", ptr(x), ptr(y), x.numel(), stream())
    return y


def gelu_bwd(dy: Tensor, x: Tensor) -> Tensor:
    dx = torch.empty_like(x)
    call("cm3p_gelu_bwd", ptr(dy), ptr(x), ptr(dx), x.numel(), stream())
    return dx


# ------------------------------------------------------------------------------------------------ audio front end
def im2col_k3(x: Tensor, token_major: bool, B: int, C: int, T_in: int, stride: int):
    T_out = (T_in - 1) // stride + 1
    p = torch.empty((B * T_out, C * 3), dtype=torch.bfloat16, device=x.device)
    call("cm3p_im2col_k3", ptr(x, torch.bfloat16 if token_major else torch.float32), int(token_major), ptr(p), B, C, T_in, T_out, stride, stream())
    return p, T_out


def col2im_k3(dp: Tensor, B: int, C: int, T_in: int, T_out: int, stride: int) -> Tensor:
    dx = torch.empty((B, T_in, C), dtype=torch.bfloat16, device=dp.device)
    call("cm3p_col2im_k3", ptr(dp), ptr(dx), B, C, T_in, T_out, stride, stream())
    return dx


def bias_gelu_fwd(z: Tensor, bias: Tensor, want_bf16: bool, want_f32: bool):
    R, C = z.shape
    a16 = torch.empty((R, C), dtype=torch.bfloat16, device=z.device) if want_bf16 else None
    a32 = torch.empty((R, C), dtype=torch.float32, device=z.device) if want_f32 else None
    call("cm3p_bias_gelu_fwd", ptr(z), ptr(bias), ptr(a16), ptr(a32), R, C, stream())
    return a16, a32


def bias_gelu_bwd(da: Tensor, z: Tensor, bias: Tensor):
    R, C = z.shape
    dz = torch.empty((R, C), dtype=torch.bfloat16, device=z.device)
    part = torch.empty((query("cm3p_bias_gelu_bwd_blocks", R), C), dtype=torch.float32, device=z.device)
    db = torch.empty((C,), dtype=torch.float32, device=z.device)
    call("cm3p_bias_gelu_bwd", ptr(da), dt(da), ptr(z), ptr(bias), ptr(dz), ptr(part), ptr(db), R, C, stream())
    return dz, db


# ------------------------------------------------------------------------------------------------ pooling
def pool_fwd(h: Tensor, mask: Optional[Tensor], Bn: int, S: int, cls: bool, cu: Optional[Tensor] = None, total: Optional[int] = None):
    """h [Bn, S, H] fp32 or bf16 (fp32 accumulation either way) -> (pooled [Bn, H] fp32, count [Bn] fp32).
    Packed rows: h [total, H], cu int32 [Bn + 1] (sequence b owns rows cu[b] .. cu[b+1]-1), S = max_seqlen, no mask."""
    H = h.shape[-1]
    if cu is not None:  # (the entry point takes cu_seqlens where a padded batch has its mask, flagged in cls)
        _packed_pool_args(h.shape[0], mask, Bn, S, cu, total)
        pooled = torch.empty((Bn, H), dtype=torch.float32, device=h.device)
        count = torch.empty((Bn,), dtype=torch.float32, device=h.device)
        part = None if cls else torch.empty((Bn, query("cm3p_pool_chunks", S), H), dtype=torch.float32, device=h.device)
        call("cm3p_pool_fwd", ptr(h), dt(h), ptr(cu, torch.int32), ptr(pooled), ptr(part), ptr(count), Bn, S, H, int(cls) | POOL_PACKED, stream())
        return pooled, count
    pooled = torch.empty((Bn, H), dtype=torch.float32, device=h.device)
    count = torch.empty((Bn,), dtype=torch.float32, device=h.device)
    part = None if cls else torch.empty((Bn, query("cm3p_pool_chunks", S), H), dtype=torch.float32, device=h.device)
    call("cm3p_pool_fwd", ptr(h), dt(h), ptr(mask, torch.int64), ptr(pooled), ptr(part), ptr(count), Bn, S, H, int(cls), stream())
    return pooled, count


def _packed_pool_args(rows: int, mask, Bn: int, S: int, cu: Tensor, total: Optional[int]) -> int:
    """What can be checked of a packed description without a host read (the forward kernels read the rows cu names, as the varlen
    attention kernels do: _PoolPackedFn checks cu itself; the backward writes rows below total only, whatever cu holds)."""
    total = rows if total is None else int(total)
    if mask is not None:
        raise ValueError("packed rows carry no mask: pass cu alone")
    if cu.numel() != Bn + 1:
        raise ValueError(f"cu has {cu.numel()} entries for {Bn} sequences (Bn + 1 expected)")
    if not 0 < total <= rows:
        raise ValueError(f"total {total} must lie in 1 .. {rows}, the rows of the packed tensor")
    return total


def pool_bwd(dpooled: Tensor, mask: Optional[Tensor], count: Optional[Tensor], Bn: int, S: int, cls: bool, dtype: torch.dtype = torch.float32,
             cu: Optional[Tensor] = None, total: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """-> dh [Bn * S, H] of `dtype` (fp32, or bf16 when the pooled rows were a bf16 residual stream's: one rounding of the fp32 value).
    Packed rows (cu int32 [Bn + 1], total): dh [total, H], every row written once, zeros at and past cu[Bn].  out: write the first
    `total` rows of this [>= total, H] tensor instead of a new one (it fixes the dtype)."""
    H = dpooled.shape[-1]
    if cu is not None:
        if total is None and out is None:
            raise ValueError("packed pooling backward needs total (the rows of dh)")
        dh = out if out is not None else torch.empty((int(total), H), dtype=dtype, device=dpooled.device)
        if dh.dim() != 2 or dh.shape[1] != H or dpooled.shape[0] != Bn:
            raise ValueError(f"dh {tuple(dh.shape)} / dpooled {tuple(dpooled.shape)} do not fit {Bn} sequences of width {H}")
        total = _packed_pool_args(dh.shape[0], mask, Bn, S, cu, total)
        if total >= 2 ** 31:
            raise ValueError("packed pooling backward: the row count must fit an int")
        call("cm3p_pool_bwd", ptr(dpooled, torch.float32), ptr(cu, torch.int32), ptr(count), ptr(dh), dt(dh), Bn, total, H, int(cls) | POOL_PACKED,
             stream())  # (S carries the row count of dh)
        return dh
    dh = torch.empty((Bn * S, H), dtype=dtype, device=dpooled.device)
    call("cm3p_pool_bwd", ptr(dpooled, torch.float32), ptr(mask, torch.int64), ptr(count), ptr(dh), dt(dh), Bn, S, H, int(cls), stream())
    return dh


# ------------------------------------------------------------------------------------------------ fp32 head
# Route of cm3p_gemm_f32 (both give the same bits, so this is a choice of speed alone): the tiled kernels from
# GEMM_F32_TILED_MIN_OUTPUTS outputs (M * N) on, the 16 x 16 kernel below.  Measured on one MI355X (profiles/gemm_f32_tiled.txt) the
# tiled route was faster or equal at every shape of the head, down to the 32 x 32 local head and 8 x 2048 logits, and found no
# crossover: behind the flag the entry point itself takes 16 x 16 outputs per workgroup with k in tiles of 64 for problems of fewer
# than 2^20 outputs (k is never split, so those cannot fill the chip with large tiles) and 32..128 x 64..128 register tiles from
# there on.  1024 outputs is the local head at b = 32; smaller, launch-bound calls (probes at 8 x 8 and 16 x 16 were 5-8 us faster on
# the tiled route too) stay on the kernel they have always run on.
# Tests set the constant to 0 (tiled wherever the operands allow it) or to a huge value (never).
GEMM_F32_TILED_MIN_OUTPUTS = 1024
GEMM_F32_TAGS = {False: "cm3p_gemm_f32 [16x16]", True: "cm3p_gemm_f32 [tiled]"}


def gemm_f32_route(M: int, N: int, a_strides, b_strides) -> bool:
    """True: the tiled kernel.  Decided from the shape and the strides only, never from the data."""
    unit = 1 in tuple(a_strides) and 1 in tuple(b_strides)  # the tiled kernel needs a unit stride in each operand
    return unit and M * N >= GEMM_F32_TILED_MIN_OUTPUTS


def gemm_f32(a: Tensor, b: Tensor, M: int, N: int, K: int, a_strides, b_strides, alpha: float = 1.0,
             out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    tiled = gemm_f32_route(M, N, a_strides, b_strides)
    call("cm3p_gemm_f32", ptr(a), ptr(b), ptr(out), M, N, K, a_strides[0], a_strides[1], b_strides[0], b_strides[1], N, alpha,
         int(bool(accumulate)) | (GEMM_F32_TILED if tiled else 0), stream(), tag=GEMM_F32_TAGS[tiled], work=2.0 * M * N * K)
    return out


def l2norm_fwd(x: Tensor):
    rows, D = x.shape
    y = torch.empty_like(x)
    norm = torch.empty((rows,), dtype=torch.float32, device=x.device)
    call("cm3p_l2norm_fwd", ptr(x), ptr(y), ptr(norm), rows, D, stream())
    return y, norm


def l2norm_bwd(dy: Tensor, y: Tensor, norm: Tensor) -> Tensor:
    dx = torch.empty_like(y)
    call("cm3p_l2norm_bwd", ptr(dy), ptr(y), ptr(norm), ptr(dx), y.shape[0], y.shape[1], stream())
    return dx


def cross_entropy(logits: Tensor, rows: int, cols: int, row_stride: int, col_stride: int, target: Tensor,
                  row_offset: Optional[Tensor], grad_scale: float, dlogits: Optional[Tensor]) -> Tensor:
    loss_rows = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    call("cm3p_cross_entropy", ptr(logits, torch.float32), rows, cols, row_stride, col_stride, ptr(row_offset, torch.int64), ptr(target, torch.int64), grad_scale,
         ptr(loss_rows), ptr(dlogits), stream())
    return loss_rows


def cross_entropy_masked(logits: Tensor, cols: int, target: Tensor, ignore_index: int, grad_scale: float, inv_count: Tensor,
                         want_grad: bool):
    rows, pitch = logits.shape
    loss_rows = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    call("cm3p_cross_entropy_masked", ptr(logits, torch.float32), rows, cols, pitch, ptr(target, torch.int64), ignore_index, grad_scale, ptr(inv_count, torch.float32),
         ptr(loss_rows), ptr(dlogits), stream())
    return loss_rows, dlogits


def ce_masked_stats(logits: Tensor, cols: int, target: Tensor, ignore_index: int):
    """-> (loss_rows, lse_rows), zero for ignored rows."""
    rows, pitch = logits.shape
    loss_rows = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    lse_rows = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    call("cm3p_ce_masked_stats", ptr(logits, torch.float32), rows, cols, pitch, ptr(target, torch.int64), ignore_index, ptr(loss_rows), ptr(lse_rows, torch.float32), stream())
    return loss_rows, lse_rows


def ce_masked_dlogits_bf16(logits: Tensor, cols: int, target: Tensor, ignore_index: int, lse_rows: Tensor, scale_a: Tensor, scale_b: Tensor):
    """-> (dlogits bf16 [rows, pitch], column sums fp32 [pitch]) of scale_a * scale_b * (softmax - onehot) on the labelled rows."""
    rows, pitch = logits.shape
    dl = torch.empty((rows, pitch), dtype=torch.bfloat16, device=logits.device)
    part = torch.empty((query("cm3p_ce_masked_dlogits_blocks", rows), pitch), dtype=torch.float32, device=logits.device)
    colsum = torch.empty((pitch,), dtype=torch.float32, device=logits.device)
    call("cm3p_ce_masked_dlogits_bf16", ptr(logits, torch.float32), rows, cols, pitch, ptr(target, torch.int64), ignore_index, ptr(lse_rows, torch.float32), ptr(scale_a, torch.float32), ptr(scale_b, torch.float32),
         ptr(dl), ptr(part), ptr(colsum), stream())
    return dl, colsum


def mlm_lse(y: Tensor, w: Tensor, bias: Optional[Tensor], cols: int, target: Tensor, ignore_index: int):
    """The decoder GEMM and ce_masked_stats in one, without the logits (include/ext/cm3p_mlm_loss.h): y [T, H] bf16, w [Vp, H] bf16,
    bias [Vp] fp32 or None, cols = V <= Vp -> (loss_rows, lse_rows), zero for ignored rows."""
    T, H = y.shape
    Vp = w.shape[0]
    loss_rows = torch.empty((T,), dtype=torch.float32, device=y.device)
    lse_rows = torch.empty((T,), dtype=torch.float32, device=y.device)
    nbytes = query("cm3p_mlm_lse_workspace_bytes", T, Vp)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=y.device)
    call("cm3p_mlm_lse", ptr(y, torch.bfloat16), ptr(w, torch.bfloat16), ptr(bias, torch.float32) if bias is not None else None, ptr(target, torch.int64), ignore_index,
         T, H, cols, Vp, ptr(loss_rows), ptr(lse_rows), ptr(ws), ws.numel(), stream(), tag="cm3p_mlm_lse", work=2.0 * T * Vp * H)
    return loss_rows, lse_rows


def mlm_dlogits(y: Tensor, w: Tensor, bias: Optional[Tensor], cols: int, target: Tensor, ignore_index: int, lse_rows: Tensor, scale_a: Tensor,
                scale_b: Tensor, colsum: Optional[Tensor] = None, accumulate: bool = False, out: Optional[Tensor] = None):
    """ce_masked_dlogits_bf16 from recomputed logit tiles: -> (dlogits bf16 [T, Vp], column sums fp32 [Vp]).  accumulate: the sums are
    added to `colsum` (the row chunks of one batch); out: a [>= T, Vp] bf16 buffer whose first T rows are written."""
    T, H = y.shape
    Vp = w.shape[0]
    dl = torch.empty((T, Vp), dtype=torch.bfloat16, device=y.device) if out is None else out[:T]
    if colsum is None:
        if accumulate:
            raise ValueError("mlm_dlogits: accumulate needs the colsum to add to")
        colsum = torch.empty((Vp,), dtype=torch.float32, device=y.device)
    nbytes = query("cm3p_mlm_dlogits_workspace_bytes", T, Vp)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=y.device)
    call("cm3p_mlm_dlogits", ptr(y, torch.bfloat16), ptr(w, torch.bfloat16), ptr(bias, torch.float32) if bias is not None else None, ptr(target, torch.int64), ignore_index,
         ptr(lse_rows, torch.float32), ptr(scale_a, torch.float32), ptr(scale_b, torch.float32), T, H, cols, Vp, ptr(dl, torch.bfloat16), ptr(colsum, torch.float32),
         int(accumulate), ptr(ws), ws.numel(), stream(), tag="cm3p_mlm_dlogits", work=2.0 * T * Vp * H)
    return dl, colsum


def mlm_topk(y: Tensor, w: Tensor, bias: Optional[Tensor], cols: int, k: int):
    """The decoder GEMM and a top-k in one, without the logits (include/ext/predict/cm3p_mlm_topk.h): y [T, H] bf16, w [Vp, H] bf16,
    bias [Vp] fp32 or None, cols = V <= Vp, 1 <= k <= 8 -> (idx int32 [T, k], val fp32 [T, k], lse fp32 [T]): every row's k best columns
    below V by (logit descending, column ascending), their logits (index -1 and -inf past V when V < k) and log sum exp of the row."""
    T, H = y.shape
    Vp = w.shape[0]
    if not 1 <= int(k) <= 8:
        raise ValueError(f"mlm_topk: k must lie in 1..8, got {k}")
    k = int(k)
    idx = torch.empty((T, k), dtype=torch.int32, device=y.device)
    val = torch.empty((T, k), dtype=torch.float32, device=y.device)
    lse = torch.empty((T,), dtype=torch.float32, device=y.device)
    if T == 0:  # (nothing to launch; an empty tensor has no address to hand over)
        return idx, val, lse
    nbytes = query("cm3p_mlm_topk_workspace_bytes", T, Vp, k)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=y.device)
    call("cm3p_mlm_topk", ptr(y, torch.bfloat16), ptr(w, torch.bfloat16), ptr(bias, torch.float32) if bias is not None else None, T, H, cols, Vp, k,
         ptr(idx, torch.int32), ptr(val, torch.float32), ptr(lse, torch.float32), ptr(ws), ws.numel(), stream(), tag="cm3p_mlm_topk", work=2.0 * T * Vp * H)
    return idx, val, lse


def inv_valid_count(target: Tensor, ignore_index: int) -> Tensor:
    out = torch.empty((1,), dtype=torch.float32, device=target.device)
    call("cm3p_inv_valid_count", ptr(target, torch.int64), target.numel(), ignore_index, ptr(out), stream())
    return out


def add_bias_(x: Tensor, bias: Tensor) -> Tensor:
    call("cm3p_add_bias_f32", ptr(x), ptr(bias), x.shape[0], x.shape[1], stream())
    return x


def colsum_f32(x: Tensor) -> Tensor:
    rows, cols = x.shape
    part = torch.empty((query("cm3p_colsum_blocks", rows), cols), dtype=torch.float32, device=x.device)
    out = torch.empty((cols,), dtype=torch.float32, device=x.device)
    call("cm3p_colsum_f32", ptr(x), ptr(part), ptr(out), rows, cols, stream())
    return out


def pointwise_loss(x: Tensor, y: Tensor, kind: int):
    """Mean MSE (kind 0) / BCE-with-logits (kind 1) of fp32 x against y -> (loss [1], dloss/dx)."""
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    call("cm3p_pointwise_loss", ptr(x), ptr(y), ptr(out), ptr(dx), x.numel(), kind, stream())
    return out, dx


def first_zero_index(classes: Tensor) -> Tensor:
    B, V = classes.shape
    idx = torch.empty((B,), dtype=torch.int64, device=classes.device)
    call("cm3p_first_zero_index", ptr(classes, torch.int64), B, V, ptr(idx, torch.int64), stream())
    return idx


def scale_exp(x: Tensor, log_scale: Tensor) -> Tensor:
    y = torch.empty_like(x)
    call("cm3p_scale_exp", ptr(x), ptr(log_scale), ptr(y), x.numel(), stream())
    return y


def scale_by(x: Tensor, scale: Tensor) -> Tensor:
    y = torch.empty_like(x)
    call("cm3p_scale_by", ptr(x), ptr(scale), ptr(y), x.numel(), stream())
    return y


def dot_f32(a: Tensor, b: Tensor) -> Tensor:
    out = torch.empty((1,), dtype=torch.float32, device=a.device)
    call("cm3p_dot_f32", ptr(a), ptr(b), ptr(out), a.numel(), stream())
    return out


def sum_f32(x: Tensor, scale: float, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=x.device)
    call("cm3p_sum_f32", ptr(x), ptr(out), x.numel(), scale, int(accumulate), stream())
    return out
