"""The fused global attention backward (csrc/attention_bwd_fused.hip, cm3p_attn_bwd_fused) past one dQ slab: the case table, the inverse
RoPE of its two epilogues in float64 with rotated bounds, the packed form, the slab arithmetic restated and the wrong evaluations of all
of it.  Shared by tests/test_attention_fused_gpu.py (the kernel against them) and tests/test_attention_fused_refs_host.py (the emulation
passes, the wrong evaluations fail, the table reaches the seams it names).  The float64 reference, the bounds and the emulation are
tests/attention_refs.py's (its module docstring counts the roundings, the G-dependent ones included).  No GPU, no cm3p_amd import.

The table (global, window -1, NH = 2, head size 64, both q modes) - the smallest shapes that reach each seam of the kernel:
  S = 385  lens (385, 64, 1)    7 query tiles; a second key block of 129 keys; a one-tile and a one-row sequence
  S = 513  lens (513, 256, 65)  3 key blocks, the last with ONE key (three keyless waves); 2 slabs at G = 2; a sequence ending on a block edge
  S = 640  no mask, B = 2       10 tiles; a half-full last key block
  S = 768  no mask, B = 3       12 tiles; exact blocks; a partial last group at G = 2 and at G = 4
  S = 1025 lens (1025, 769)     17 tiles; 5 key blocks: 2 + 2 + 1 at G = 2, 4 + 1 at G = 4
  S = 1300 holes, B = 5         21 tiles; 6 key blocks: 3 slabs at G = 2, 4 + 2 at G = 4; attention_refs._key_mask's five patterns
With table G's 300 / 449 / 257, ceil(S / 64) takes every residue mod 6 (the ring's unroll) and the 1-D grids of the storing and the
adding launches are both below 8 and above 8 without being multiples of 8 (xcd_remap); launch_grids restates them.

RoPE.  Both epilogues rotate the fp32 sum (dq: the reduce's sum of the slabs; dk: the accumulator), THEN scale and round to bf16:
y[d] = x[d] c + x[d + 32] s, y[d + 32] = x[d + 32] c - x[d] s (rope_rotate4<true>, tables [n_pos, 32] fp32).  The rotation is linear, so
an error e of x becomes at most |c| |e[d]| + |s| |e[d +- 32]|: the un-rotated bound, rotated with |c| and |s|.  That bound also counts
the bf16 STORE, which here comes after the rotation; it is still covered: the store is off by u |y| <= u (|c| |x[d]| + |s| |x[d +- 32]|),
and u |x[d]| <= u scale (|dS||K|)[d] is exactly the store term the un-rotated bound holds for element d (the same with |Q| for dk) - so
rotating that term with |c|, |s| bounds the rounding of the rotated value.  What is new is the rotation's own fp32 arithmetic, two
products and a sum: 3 U (|c| |x[d]| + |s| |x[d +- 32]|) taken with |x| <= |ref| + bound (row_kernel_refs.rope_apply_ref's count).
Table rows: pos0 + row, pos0 = b * pos_batch_stride (padded; the tests start batch b at position 7 b so that rows of different batches
differ) or the packed row cu[b] + row (per-token tables; sequences start at positions 7 b, not 0, so a table indexed by the row inside
the sequence reads other values)."""
import functools

import torch

import attention_refs as AR
from attention_refs import NH, SCALE, Case
from row_kernel_refs import FTZ, SECOND, U, rope_inv_freq, rope_table_ref

CASES_F = ((385, (385, 64, 1), False, 0), (513, (513, 256, 65), False, 0), (640, None, False, 2), (768, None, False, 3),
           (1025, (1025, 769), False, 0), (1300, None, True, 0))
TABLE_F = [Case("F", S, -1, lens, pre, False, holes, nb) for S, lens, holes, nb in CASES_F for pre in (False, True)]
BY_NAME = {c.name: c for c in TABLE_F}
GROUPS = (2, 4)
ROPE_S = (513, 1025)       # the cases the RoPE epilogues run on (both have lens: also packed)
POS_STEP = 7               # batch / sequence b starts at position 7 b
ROPE_THETA = 10000.0
RELOC_S, RELOC_BLOCKS = 1280, 5
LONG_S = 5900              # the length rule picks G = 4 from S = 5889 on
WRONG_FUSED = AR.WRONG_FUSED_SLABS + ("rope_forward_instead_of_inverse", "rope_row_of_batch_0", "rope_packed_row_restarts_per_sequence")


def long_rows(S=LONG_S):
    """The query rows of three tiles: tile 0, one in the middle of the sequence and the ragged last one."""
    mid = 64 * (-(-S // 64) // 2)
    return torch.cat([torch.arange(64), torch.arange(mid, mid + 64), torch.arange(64 * ((S - 1) // 64), S)])


def key_blocks(S):
    return -(-S // 256)


def groups_of(case):
    """G = 4 only where there are three or more key blocks."""
    return tuple(G for G in GROUPS if G == 2 or key_blocks(case.S) >= 3)


def launch_grids(case, G):
    """The 1-D grid sizes of cm3p_attn_bwd_fused's main launches -> (storing, [adding, position 1 .. G - 1])."""
    nkb = key_blocks(case.S)
    return -(-nkb // G) * NH * case.B, [-(-(nkb - p) // G) * NH * case.B for p in range(1, min(G, nkb))]


def slab_groups(S, G):
    """Key blocks per slab, in slab order: 1025 -> [2, 2, 1] at G = 2, [4, 1] at G = 4."""
    nkb = key_blocks(S)
    return [min(G, nkb - j) for j in range(0, nkb, G)]


def workspace_bytes(B, S, nh):
    """cm3p_attn_bwd_fused_workspace_bytes restated: two 64-float statistics rows per 64-row tile and 12 pad tiles, rounded up to 256
    bytes, and the bf16 slabs [B nh][slabs at G = 2][64 tiles + 64 dump rows][64]."""
    if B <= 0 or S <= 0 or nh <= 0:
        return 0
    tiles = -(-S // 64)
    stats = -(-(B * nh * (tiles + 12) * 128 * 4) // 256) * 256
    return stats + B * nh * -(-key_blocks(S) // 2) * (64 * tiles + 64) * 128


# ================================================================================================ packed
def padded_rows_zeroed(case):
    """inputs(case) with dO = 0 on the padded query rows (the packed entry points have none; in the model they never reach the loss)."""
    x, km = AR.inputs(case), AR.key_mask(case)
    return dict(x, do=x["do"] * km[:, :, None, None].to(torch.bfloat16))


def cu_seqlens(case):
    return [0] + [int(v) for v in torch.tensor(case.lens).cumsum(0)]


# ================================================================================================ RoPE
@functools.lru_cache(maxsize=None)
def rope_tables(case, form):
    """fp32 cos / sin tables [n_pos, 32] as cm3p_rope_table writes them (cos / sin of ONE fp32 product pos * inv_freq) and the table row
    of every (b, row) -> (cos, sin, index [B, S] long).  form: "shared" - pos_batch_stride 0, one table of S rows, positions 0 ..;
    "batch" - pos_batch_stride S, [B S, 32], batch b at positions 7 b ..; "packed" - per token [total, 32], sequence b at 7 b .. (index
    cu[b] + row; rows past a sequence's length point at row 0 of the table and are never used)."""
    B, S = case.B, case.S
    inv = rope_inv_freq(ROPE_THETA, 64)
    r = torch.arange(S)
    if form == "shared":
        pos, index = r, r[None].expand(B, -1)
    elif form == "batch":
        pos = (POS_STEP * torch.arange(B)[:, None] + r[None]).reshape(-1)
        index = (S * torch.arange(B)[:, None] + r[None])
    else:
        cu = cu_seqlens(case)
        pos = torch.cat([POS_STEP * b + torch.arange(n) for b, n in enumerate(case.lens)])
        index = torch.stack([torch.where(r < n, cu[b] + r, torch.zeros_like(r)) for b, n in enumerate(case.lens)])
    cos, sin = rope_table_ref(pos, inv)
    return cos.float(), sin.float(), index.contiguous()


def _cs(cos, sin, index, dtype):
    """-> c, s [B, 1, S, 32] of every (b, row)."""
    return cos.to(dtype)[index][:, None], sin.to(dtype)[index][:, None]


def rotate_inverse(x, cos, sin, index, forward=False):
    """x [B, NH, S, 64] (float64 or fp32) -> the inverse rotation over pairs (d, d + 32) in x's precision."""
    c, s = _cs(cos, sin, index, x.dtype)
    a, b = x[..., :32], x[..., 32:]
    if forward:
        return torch.cat([a * c - b * s, b * c + a * s], -1)
    return torch.cat([a * c + b * s, b * c - a * s], -1)


def rotate_bound(ref_x, bound, cos, sin, index):
    """The bound of the rotated quantity (module docstring): |c| bound[d] + |s| bound[d +- 32] + the rotation's fp32 floor."""
    c, s = _cs(cos, sin, index, torch.float64)
    c, s = c.abs(), s.abs()
    ba, bb = bound[..., :32], bound[..., 32:]
    ma, mb = ref_x[..., :32].abs() + ba, ref_x[..., 32:].abs() + bb
    return torch.cat([c * ba + s * bb + 3.0 * U * (c * ma + s * mb) * SECOND + FTZ, c * bb + s * ba + 3.0 * U * (c * mb + s * ma) * SECOND + FTZ], -1)


def rotated(ref, cos, sin, index, G):
    """A reference (or a conditioned one) with dq and dk rotated: -> dict(dq, dk, bound_dq at G key blocks per slab, bound_dk)."""
    bq = AR.bound_fused_dq(ref, G)
    return dict(dq=rotate_inverse(ref["dq"], cos, sin, index), dk=rotate_inverse(ref["dk"], cos, sin, index),
                bound_dq=rotate_bound(ref["dq"], bq, cos, sin, index), bound_dk=rotate_bound(ref["dk"], ref["bound"]["dk"], cos, sin, index))


def check_rotated(rot, got, live=None):
    """dq and dk against the rotated float64 reference within the rotated bounds (live [B, S] bool: these rows only - the packed form
    has no others) -> (measured, failures); the tensor-wide relative L2 bound of attention_refs as well."""
    seen, fails = {}, []
    for nm in ("dq", "dk"):
        g, w, bnd = got[nm].double(), rot[nm], rot[f"bound_{nm}"]
        if live is not None:
            sel = live[:, None, :].expand(-1, NH, -1)
            g, w, bnd = g[sel], w[sel], bnd[sel]
        seen[f"rope_{nm}"], nbad = AR.ratio(g, w, bnd)
        if nbad:
            fails.append(f"rotated {nm}: {nbad} elements outside the bound, worst error / bound = {seen[f'rope_{nm}']:.3f}")
        seen[f"rope_{nm}_rel_l2"] = ((g - w).norm() / w.norm()).item()
        if not seen[f"rope_{nm}_rel_l2"] < AR.GRAD_REL_L2:
            fails.append(f"rotated {nm}: relative L2 error {seen[f'rope_{nm}_rel_l2']:.3e}")
    return seen, fails


# ================================================================================================ emulation
def emulate(case, G=2, rope=None, packed=False, wrong=None):
    """attention_refs.emulate(fused=True) at G key blocks per slab; rope: a form of rope_tables - the epilogues rotate the fp32 sums, scale
    and round; packed: dO is zero on padded rows (the valid rows of the result are what the packed call gives: the kernel test holds the
    two to the same bits).  wrong: one of WRONG_FUSED."""
    x = padded_rows_zeroed(case) if packed else None
    got = AR.emulate(case, fused=True, G=G, wrong=wrong if wrong in AR.WRONG_FUSED_SLABS else None, x=x)
    if rope is None:
        return got
    cos, sin, index = rope_tables(case, rope)
    if wrong == "rope_row_of_batch_0":
        index = index[:1].expand(case.B, -1)
    if wrong == "rope_packed_row_restarts_per_sequence":
        index = torch.arange(case.S)[None].expand(case.B, -1).clamp(max=cos.shape[0] - 1)
    fwd = wrong == "rope_forward_instead_of_inverse"
    got["dq"] = (rotate_inverse(got["dq_acc"], cos, sin, index, fwd) * SCALE).to(torch.bfloat16)
    got["dk"] = (rotate_inverse(got["dk_acc"], cos, sin, index, fwd) * got["dk_mul"]).to(torch.bfloat16)
    return got


# ================================================================================================ key-block relocation
@functools.lru_cache(maxsize=None)
def relocation_data():
    """S = 1280, B = 1: q and dO of every row, and ONE block of 256 K / V rows that run j places at key block j (the other K / V rows are
    other random rows: their keys are masked) -> (q [S, NH, 64], do [S, NH, 64], k_block, v_block [256, NH, 64], k_other, v_other [S, NH, 64])."""
    g = torch.Generator().manual_seed(64128)
    q, do, ko, vo = (torch.randn(RELOC_S, NH, 64, generator=g).to(torch.bfloat16) for _ in range(4))
    kb, vb = (torch.randn(256, NH, 64, generator=g).to(torch.bfloat16) for _ in range(2))
    return q, do, kb, vb, ko, vo


def relocation_qkv(j, pre):
    """-> qkv [1, S, 3, NH, 64] bf16 as the device gets it, key_mask [1, S] bool: only the keys of key block j valid."""
    q, do, kb, vb, ko, vo = relocation_data()
    if pre:
        q = (q.float() * AR.SOFTMAX_Q_SCALE).to(torch.bfloat16)
    k, v = ko.clone(), vo.clone()
    k[256 * j:256 * j + 256], v[256 * j:256 * j + 256] = kb, vb
    km = torch.zeros(1, RELOC_S, dtype=torch.bool)
    km[0, 256 * j:256 * j + 256] = True
    return torch.stack([q, k, v], 1)[None].contiguous(), km
