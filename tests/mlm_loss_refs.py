"""Float64 references and derived error bounds of the logit-free masked-LM loss kernels (csrc/mlm_loss.hip, include/ext/cm3p_mlm_loss.h),
shared by tests/test_mlm_loss_kernels_gpu.py (the kernels against them) and tests/test_mlm_loss_refs_host.py (a torch fp32 restatement
of the kernels' path against them, and wrong evaluations that must fail them).  No GPU and no cm3p_amd import here.

The reference values are those of tests/loss_head_refs.py (ce_stats_ref, ce_dlogits_ref) applied to the float64 logits of the bf16
operands, x = y W^T (+ bias).  The bounds restate that file's counting (u = 2^-24 per rounded fp32 operation, LIBM per expf / logf,
SECOND once, FTZ) for this kernel's path:
  logits   x_k = fl(acc + bias): the products of two bf16 numbers are exact in fp32; their fp32 accumulation over H terms in the MFMA is
           within 2 H u sum_k |y_k W_ck| (tests/gemm_refs.py random_bound: any order, truncating adds allowed); the bias add rounds once
           more, u |x|.  dx[r, c] is that per-element bound; operands whose products are exact zeros and ones (the exact rows) have
           an exact accumulation and keep only the bias add.
  lse      per 128-column tile M_t = max (exact), S_t = sum exp(x - M_t): 15 adds in the lane, 2 over the lanes, 1 over the two waves;
           the combine takes M = max_t M_t and S = sum_t S_t exp(M_t - M): a subtraction, an expf, a product and tiles - 1 adds.  An
           element's exponential is exp(x - M_t) exp(M_t - M): the two exponents add up to d = x - M, so their subtractions cost u |d|
           together and there are two expf.  Then logf and M + . as in ce_stats_ref.  The logits' own error moves lse by at most
           sum_c p_c dx_c exp(2 max dx) (the gradient of lse is a softmax at an intermediate point).
  dlogits  ce_dlogits_ref's e32 for exact logits, plus |s| p expm1(dx) for the logit's error; the bf16 store through bf16_bound.
  colsum   the unrounded values: 3 adds in the lane, 4 over the 16 lanes, 1 over the two waves, row tiles - 1 adds in the combine and one
           more when it accumulates.
"""
import torch

from loss_head_refs import FTZ, IGNORE, LIBM, PAD_VALUE, SECOND, U, bf16_bound, bits_equal, ce_case, ce_dlogits_ref, ce_live, ce_stats_ref, check, gen  # noqa: F401

TILE = 128
# the seams of the 128 x 128 x 64 tile: one row; below, at and past a row tile; two tiles and a part / a handful of columns; below, at and
# past a column tile; a second tile's first half and a bit; the model's vocabulary / one 8-wide k chunk; one k tile; one and a chunk; two and a chunk
SEAM_T = (1, 127, 128, 129, 300)
SEAM_V = (5, 127, 128, 129, 200, 3167)
SEAM_H = (8, 64, 72, 136)
EXACT_KINDS = ("all equal", "one +100 rest -100, target on the +100", "one +100 rest -100, target on a -100", "all about -90", "all about +88",
               "target at column 0", "target at column cols - 1", "target in the last partial tile")


def vp_of(V):
    return (V + 63) // 64 * 64


def tiles(n):
    return -(-n // TILE)


def lse_workspace_bytes(T, Vp):
    """cm3p_mlm_lse_workspace_bytes restated: one (M, S) pair of floats per (128-column tile, row)."""
    return T * tiles(Vp) * 8


def dlogits_workspace_bytes(T, Vp):
    """cm3p_mlm_dlogits_workspace_bytes restated: one float per (128-row tile, column)."""
    return tiles(T) * Vp * 4


def chunk_rows(Vp, budget=256 << 20):
    """_MLMHeadLogitFreeLossFn's rows per chunk restated: the largest multiple of 128 with rows * Vp * 2 <= 256 MiB, at least 128."""
    return max(128, budget // (Vp * 2) // 128 * 128)


# ================================================================================================ data
def _pad(W, bias, V, Vp):
    Wp = torch.full((Vp, W.shape[1]), PAD_VALUE, dtype=torch.float32)
    Wp[:V] = W
    bp = None
    if bias is not None:
        bp = torch.full((Vp,), PAD_VALUE, dtype=torch.float32)
        bp[:V] = bias
    return Wp.to(torch.bfloat16), bp


def mlm_case(T, V, H, g, bias=True, ignored_tile=None):
    """Random operands: y bf16 [T, H] ~ N(0, 1), W bf16 [Vp, H] ~ N(0, 9 / H) (logits with spread 3), bias fp32 [Vp] ~ N(0, 1) or None;
    pad rows of W and pad entries of bias hold PAD_VALUE.  Labels int64 [T]: a third IGNORE; where T allows, row 0 targets column 0,
    row 1 column V - 1, row 2 carries label V, row 3 label -5, row 4 IGNORE, row 5 a target in the last (partial) column tile;
    ignored_tile = k: rows 128 k .. 128 k + 127 all IGNORE.  The y rows of every row that is not live hold NaN."""
    Vp = vp_of(V)
    y = torch.randn(T, H, generator=g)
    W = torch.randn(V, H, generator=g) * 3 / H ** 0.5
    b = torch.randn(V, generator=g) if bias else None
    lab = torch.randint(0, V, (T,), generator=g)
    lab = torch.where(torch.rand(T, generator=g) < 1 / 3, torch.full_like(lab, IGNORE), lab)
    for r, v in enumerate((0, V - 1, V, -5, IGNORE, (V - 1) // TILE * TILE + (V - 1) % TILE // 2)):
        if r < T:
            lab[r] = v
    if T == 1:
        lab[0] = V - 1
    if ignored_tile is not None:
        lab[TILE * ignored_tile:TILE * ignored_tile + TILE] = IGNORE
    y[~ce_live(lab, V)] = float("nan")
    Wp, bp = _pad(W, b, V, Vp)
    return y.to(torch.bfloat16), Wp, bp, lab


def exact_case(V, H, g, bias=False):
    """Rows whose logits are exact: y[r] = e_r (a unit vector) and W[:, r] = the row's bf16-representable logits, one row per
    EXACT_KINDS entry (the row kinds of loss_head_refs.ce_case, and a target in the last partial tile) -> y, W, bias, lab, kinds.
    With a bias the logits are fl(W + bias), one rounding."""
    n = len(EXACT_KINDS)
    assert H >= n and V >= 2
    Vp = vp_of(V)
    x = torch.zeros(n, V)
    lab = torch.zeros(n, dtype=torch.int64)
    for r, k in enumerate(EXACT_KINDS):
        hot = int(torch.randint(0, V, (1,), generator=g))
        lab[r] = hot
        if k == "all equal":
            x[r] = 1.703125
        elif k.startswith("one +100"):
            x[r] = -100.0
            x[r, hot] = 100.0
            lab[r] = hot if k.endswith("the +100") else (hot + 1) % V
        elif k == "all about -90":
            x[r] = -90.0 + 0.5 * torch.randint(-2, 3, (V,), generator=g)
        elif k == "all about +88":
            x[r] = 88.0 + 0.5 * torch.randint(-2, 3, (V,), generator=g)
        else:
            x[r] = (torch.randn(V, generator=g) * 3).to(torch.bfloat16).float()
            lab[r] = {"target at column 0": 0, "target at column cols - 1": V - 1}.get(k, (V - 1) // TILE * TILE)
    assert bool((x.to(torch.bfloat16).float() == x).all())
    y = torch.zeros(n, H)
    y[torch.arange(n), torch.arange(n)] = 1.0
    W = torch.zeros(V, H)
    W[:, :n] = x.t()
    b = torch.randn(V, generator=g) if bias else None
    Wp, bp = _pad(W, b, V, Vp)
    return y.to(torch.bfloat16), Wp, bp, lab, EXACT_KINDS


# ================================================================================================ references
def logits_ref(y, W, bias, V, lab, exact=False):
    """-> (x float64 [T, V], dx): the float64 logits of the bf16 operands and the bound of the kernel's fp32 logit (see the module
    docstring).  Rows that are not live are computed from zeros (their y may hold NaN; nothing of them is compared)."""
    live = ce_live(lab, V)
    yd = torch.where(live[:, None], y.double(), torch.zeros((), dtype=torch.float64))
    Wd = W[:V].double()
    x = yd @ Wd.t()
    dx = torch.zeros_like(x) if exact else 2 * y.shape[1] * U * (yd.abs() @ Wd.abs().t())
    if bias is not None:
        x = x + bias[:V].double()
        dx = dx + U * x.abs()
    return x, dx * SECOND


def lse_sum_depth(V):
    """Adds on the longest path of a row's sum of exponentials: 15 in the lane, 2 over the lanes, 1 over the waves, the product with
    exp(M_t - M), and the tiles one after another."""
    return 15 + 2 + 1 + 1 + tiles(V)


def lse_ref(y, W, bias, V, lab, exact=False):
    """-> dict live, lse, loss (ce_stats_ref's values on the float64 logits, zero on rows that are not live) and lse_b, loss_b."""
    x, dx = logits_ref(y, W, bias, V, lab, exact)
    ref = ce_stats_ref(x, V, lab)
    live = ref["live"]
    mx = x.max(1).values
    d = x - mx[:, None]
    e = torch.exp(d)
    S = e.sum(1)
    logS = torch.log(S)
    lse = mx + logS
    rS = (e * (U * d.abs() + 2 * LIBM)).sum(1) / S + lse_sum_depth(V) * U
    from_x = (e / S[:, None] * dx).sum(1) * torch.exp(2 * dx.max(1).values)
    lse_b = (rS * (1 + rS) + LIBM * logS.abs() + U * lse.abs()) * SECOND + FTZ + from_x
    xt_b = dx.gather(1, lab.clamp(0, V - 1)[:, None])[:, 0]
    loss_b = lse_b + xt_b + U * ref["loss"].abs() * SECOND
    z = torch.zeros_like(lse)
    return dict(live=live, lse=ref["lse"], loss=ref["loss"], lse_b=torch.where(live, lse_b, z), loss_b=torch.where(live, loss_b, z), x=x, dx=dx)


def colsum_depth(T, accumulate=False):
    return 3 + 4 + 1 + tiles(T) + (1 if accumulate else 0)


def dlogits_ref(y, W, bias, V, lab, lse_in, sa, sb, exact=False, colsum0=None):
    """lse_in [T] float64 (the fp32 values the kernel is handed), sa / sb the fp32 scalars as floats, colsum0 float64 [Vp] what colsum
    holds when the call accumulates -> dict g (float64, unrounded, [T, Vp]; zero on rows that are not live and on pad columns), dl_b,
    colsum, colsum_b."""
    T, Vp = y.shape[0], W.shape[0]
    x, dx = logits_ref(y, W, bias, V, lab, exact)
    base = ce_dlogits_ref(x, V, lab, lse_in, sa, sb)
    live = base["live"]
    m = live[:, None].double()
    a = torch.where(live[:, None], x - lse_in[:, None], torch.zeros((), dtype=torch.float64))
    p = torch.exp(a)
    e32 = base["e32"] + abs(sa * sb) * p * torch.expm1(dx) * SECOND * m
    g = torch.zeros(T, Vp, dtype=torch.float64)
    g[:, :V] = base["g"]
    e = torch.zeros(T, Vp, dtype=torch.float64)
    e[:, :V] = e32
    dl_b = torch.zeros(T, Vp, dtype=torch.float64)
    dl_b[:, :V] = bf16_bound(base["g"], e32) * m
    colsum = g.sum(0)
    colsum_b = (e.sum(0) + colsum_depth(T, colsum0 is not None) * U * g.abs().sum(0)) * SECOND
    if colsum0 is not None:
        colsum = colsum + colsum0
        colsum_b = colsum_b + U * colsum.abs() * SECOND
    return dict(g=g, dl_b=dl_b, colsum=colsum, colsum_b=colsum_b, live=live)


# ================================================================================================ the kernels' path in torch fp32
def _x32(y, W, bias, V, lab, pad_as_logits=False):
    live = ce_live(lab, V)
    n = W.shape[0] if pad_as_logits else V
    x = torch.where(live[:, None], y.float(), torch.zeros(())) @ W[:n].float().t()
    return x + bias[:n] if bias is not None else x


def lse_f32_path(y, W, bias, V, lab, wrong=None):
    """cm3p_mlm_lse in torch fp32: the fp32 logits, per 128-column tile (M_t, S_t), the combine in ascending tile order.  wrong:
    'pad_as_logits' (the columns [V, Vp) take part), 'target_neighbour' (the target's logit is read one column further), 'no_max'
    (sum exp(x) without the shift).  -> (loss_rows, lse_rows) fp32."""
    live = ce_live(lab, V)
    x = _x32(y, W, bias, V, lab, wrong == "pad_as_logits")
    n = x.shape[1]
    Ms, Ss = [], []
    for c0 in range(0, n, TILE):
        xt = x[:, c0:c0 + TILE]
        M = torch.zeros(x.shape[0]) if wrong == "no_max" else xt.max(1).values
        s = torch.zeros(x.shape[0])
        for c in range(xt.shape[1]):
            s = s + torch.exp(xt[:, c] - M)
        Ms.append(M)
        Ss.append(s)
    M = torch.stack(Ms).max(0).values
    S = torch.zeros(x.shape[0])
    for Mt, St in zip(Ms, Ss):
        S = S + St * torch.exp(Mt - M)
    lse = M + torch.log(S)
    t = lab.clamp(0, V - 1)
    if wrong == "target_neighbour":
        t = (t + 1) % V
    loss = lse - x.gather(1, t[:, None])[:, 0]
    z = torch.zeros(x.shape[0])
    return torch.where(live, loss, z), torch.where(live, lse, z)


def dlogits_f32_path(y, W, bias, V, lab, lse_in, sa, sb, wrong=None, colsum0=None):
    """cm3p_mlm_dlogits in torch fp32 -> (dl bf16 [T, Vp], colsum fp32 [Vp]): inside a 128-row tile the kernel's order (a lane's 4 rows,
    the 16 lanes by butterfly, the two waves), then the tiles one after another.  wrong: 'colsum_of_rounded' (the column sums add the bf16 values), 'pad_as_logits' (the pad columns get a gradient)."""
    T, Vp = y.shape[0], W.shape[0]
    live = ce_live(lab, V)
    s = torch.tensor(sa, dtype=torch.float32) * torch.tensor(sb, dtype=torch.float32)
    n = Vp if wrong == "pad_as_logits" else V
    x = _x32(y, W, bias, V, lab, wrong == "pad_as_logits")
    onehot = torch.zeros(T, n)
    onehot[torch.arange(T), lab.clamp(0, V - 1)] = 1.0
    g = torch.zeros(T, Vp)
    g[:, :n] = torch.where(live[:, None], s * (torch.exp(x - lse_in.float()[:, None]) - onehot), torch.zeros(()))
    dl = g.to(torch.bfloat16)
    add = dl.float() if wrong == "colsum_of_rounded" else g
    total = torch.zeros(Vp)
    lanes = torch.arange(16)
    for r0 in range(0, T, TILE):
        tile = torch.zeros(TILE, Vp)
        tile[:min(TILE, T - r0)] = add[r0:r0 + TILE]
        tile = tile.view(2, 4, 16, Vp)  # row = 64 wm + 16 i + lane
        part = torch.zeros(2, 16, Vp)
        for i in range(4):
            part = part + tile[:, i]
        for o in (1, 2, 4, 8):
            part = part + part[:, lanes ^ o]
        total = total + (part[0, 0] + part[1, 0])
    return dl, (colsum0.float() + total if colsum0 is not None else total)
