"""Float64 reference and acceptance rule of cm3p_mlm_topk (csrc/mlm_topk.hip, include/ext/predict/cm3p_mlm_topk.h), shared by
tests/test_mlm_topk_kernels_gpu.py (the kernel against them) and tests/test_mlm_topk_refs_host.py (a torch fp32 restatement of the
kernel's path against them, and wrong evaluations that must fail them).  No GPU and no cm3p_amd import here.

The logits and their per-element bound dx are tests/mlm_loss_refs.py's logits_ref (every row live); the reference order is (x
descending, column ascending), and lse with its bound is mlm_loss_refs.lse_ref: the kernel sums in cm3p_mlm_lse's order (15 adds in the
lane, 2 over the lanes, 1 over the waves, the tiles one after another), so lse_sum_depth holds as it stands.

Acceptance of one row (ranks 1 .. k of the kernel against ranks 1 .. k + 1 of the reference, xs their float64 values and dxs the bounds
of those columns):
  value   |top_val[i] - xs[i]| <= dxs[i].
  index   a rank is ambiguous when its gap to a neighbouring rank among 1 .. k + 1 is at most the sum of the two dx: fp32 rounding may
          then order the two the other way.  At every other rank top_idx[i] is the reference column.  At an ambiguous rank it is a
          column below V whose float64 logit lies within that column's dx of xs[i].  No column appears twice in a row.
  short   with V < k the slots V .. k - 1 hold index -1 and value -inf.
The share of rows with an ambiguous rank is a property of the inputs; AMBIGUOUS_CAP bounds it over the seam set, so that the exact
comparison is what nearly every row gets (tests/test_mlm_topk_refs_host.py asserts it from the reference alone).
"""
import torch

import mlm_loss_refs as MR
from mlm_loss_refs import PAD_VALUE, TILE, bits_equal, check, gen, tiles, vp_of  # noqa: F401

K_MAX = 8
SEAM_T = MR.SEAM_T
SEAM_H = MR.SEAM_H
SEAM_V = (5, 127, 128, 129, 200, 300)   # below, at and past one column tile; a second tile's part; three tiles
CAP_V = SEAM_V + (3167,)                # the set the cap on ambiguous rows is stated over
AMBIGUOUS_CAP = 0.02


def workspace_bytes(T, Vp, k):
    """cm3p_mlm_topk_workspace_bytes restated: k (value, column) pairs and one (M, S) pair of 8 bytes per (128-column tile, row)."""
    return T * tiles(Vp) * (k + 1) * 8


# ================================================================================================ data
def topk_case(T, V, H, g, bias=True):
    """mlm_case's operands without labels (every row is live): y bf16 [T, H] ~ N(0, 1), W bf16 [Vp, H] ~ N(0, 9 / H), bias fp32 [Vp]
    ~ N(0, 1) or None; pad rows of W and pad entries of bias hold PAD_VALUE."""
    y = torch.randn(T, H, generator=g)
    W = torch.randn(V, H, generator=g) * 3 / H ** 0.5
    b = torch.randn(V, generator=g) if bias else None
    Wp, bp = MR._pad(W, b, V, vp_of(V))
    return y.to(torch.bfloat16), Wp, bp


EXACT_KINDS = ("all equal", "equal maxima at 63 and 64", "equal maxima at 127 and 128", "winners at 0 and V - 1", "winners in 8 adjacent columns",
               "winners 128 columns apart", "all about -90", "all about +88")


def exact_case(V, H, g):
    """Rows whose logits are exact, as mlm_loss_refs.exact_case builds them: y[r] = e_r and W[:, r] = the row's bf16-representable
    logits, one row per EXACT_KINDS entry that fits V -> y, W, kinds.  The winners are 40, 39.5, ... over a background below 10."""
    kinds = [k for k in EXACT_KINDS if not ((k.endswith("63 and 64") and V < 65) or (k.endswith("127 and 128") and V < 129) or
                                            (k.endswith("adjacent columns") and V < 24) or (k.endswith("apart") and V < 128 * 7 + 6))]
    n = len(kinds)
    assert H >= n
    x = torch.zeros(n, V)
    for r, kind in enumerate(kinds):
        x[r] = (torch.randn(V, generator=g) * 3).clamp(-9, 9).to(torch.bfloat16).float()
        top = 40.0 - 0.5 * torch.arange(K_MAX)
        if kind == "all equal":
            x[r] = 1.703125
        elif kind.startswith("equal maxima"):
            c = 63 if "63" in kind else 127
            x[r, c] = x[r, c + 1] = 40.0
            x[r, 0] = 39.5
        elif kind == "winners at 0 and V - 1":
            x[r, V - 1], x[r, 0] = 40.0, 39.5
        elif kind == "winners in 8 adjacent columns":
            x[r, 16 + torch.randperm(K_MAX, generator=g)] = top
        elif kind == "winners 128 columns apart":
            x[r, 5 + TILE * torch.randperm(K_MAX, generator=g)] = top
        elif kind == "all about -90":
            x[r] = -90.0 + 0.5 * torch.randint(-2, 3, (V,), generator=g)
        elif kind == "all about +88":
            x[r] = 88.0 + 0.5 * torch.randint(-2, 3, (V,), generator=g)
    assert bool((x.to(torch.bfloat16).float() == x).all())
    y = torch.zeros(n, H)
    y[torch.arange(n), torch.arange(n)] = 1.0
    W = torch.zeros(V, H)
    W[:, :n] = x.t()
    Wp, _ = MR._pad(W, None, V, vp_of(V))
    return y.to(torch.bfloat16), Wp, kinds


# ================================================================================================ reference
def _live(T):
    return torch.zeros(T, dtype=torch.int64)  # (label 0 lies in every vocabulary: mlm_loss_refs computes every row)


def topk_ref(y, W, bias, V, k, exact=False):
    """-> dict x, dx [T, V] float64; cols [T, k + 1] int64 the reference's columns by (x descending, column ascending), -1 past V; xs,
    dxs [T, k + 1] their values (-inf past V) and bounds; amb [T, k] bool the ambiguous ranks; lse, lse_b [T]."""
    T = y.shape[0]
    r = MR.lse_ref(y, W, bias, V, _live(T), exact=exact)
    x, dx = r["x"], r["dx"]
    n = min(k + 1, V)
    order = torch.sort(-x, dim=1, stable=True).indices[:, :n]  # (ascending -x, stable: equal values keep the lower column in front)
    cols = torch.full((T, k + 1), -1, dtype=torch.int64)
    xs = torch.full((T, k + 1), float("-inf"), dtype=torch.float64)
    dxs = torch.zeros(T, k + 1, dtype=torch.float64)
    cols[:, :n], xs[:, :n], dxs[:, :n] = order, x.gather(1, order), dx.gather(1, order)
    close = torch.zeros(T, k + 1, dtype=torch.bool)  # close[:, i]: ranks i and i + 1 (0-based) may swap
    close[:, :n - 1] = (xs[:, :n - 1] - xs[:, 1:n]) <= (dxs[:, :n - 1] + dxs[:, 1:n])
    amb = close[:, :k].clone()
    amb[:, 1:] |= close[:, :k - 1]
    return dict(x=x, dx=dx, cols=cols, xs=xs, dxs=dxs, amb=amb, lse=r["lse"], lse_b=r["lse_b"], V=V, k=k)


def ambiguous_rows(ref):
    return int(ref["amb"].any(1).sum())


def check_topk(idx, val, ref, what):
    """The acceptance rule of the module docstring on idx int32 [T, k], val fp32 [T, k]; prints the worst value error / bound and the
    number of ambiguous ranks it met.  Raises AssertionError."""
    idx, val = idx.detach().cpu().to(torch.int64), val.detach().cpu().double()
    V, k = ref["V"], ref["k"]
    T = idx.shape[0]
    assert idx.shape == (T, k) and val.shape == (T, k), (what, idx.shape, val.shape)
    n = min(k, V)
    if n < k:
        assert bool((idx[:, n:] == -1).all()) and bool((val[:, n:] == float("-inf")).all()), f"{what}: slots past V are not (-1, -inf)"
    idx, val = idx[:, :n], val[:, :n]
    xs, dxs, amb, cols = ref["xs"][:, :n], ref["dxs"][:, :n], ref["amb"][:, :n], ref["cols"][:, :n]
    err = (val - xs).abs()
    bad = ~(err <= dxs)
    assert not bad.any(), f"{what}: {int(bad.sum())} values outside dx; first at {tuple(bad.nonzero()[0].tolist())}"
    inside = (idx >= 0) & (idx < V)
    assert bool(inside.all()), f"{what}: an index outside [0, {V}): {idx[~inside][:4].tolist()}"
    wrong = (idx != cols) & ~amb
    assert not wrong.any(), f"{what}: {int(wrong.sum())} unambiguous ranks hold another column; first at {tuple(wrong.nonzero()[0].tolist())}"
    near = (ref["x"].gather(1, idx) - xs).abs() <= ref["dx"].gather(1, idx)
    assert bool(near[amb].all()), f"{what}: an ambiguous rank holds a column whose logit is not within dx of the rank's value"
    srt = idx.sort(1).values
    assert not bool((srt[:, 1:] == srt[:, :-1]).any()), f"{what}: a column appears twice in a row"
    ratio = (err / dxs.clamp_min(1e-300))[dxs > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: value max err/bound {worst:.3g}, {int(amb.sum())} ambiguous ranks in {ambiguous_rows(ref)} of {T} rows")
    return worst


def check_exact(idx, val, ref, what):
    """Rows with exact logits: indices and values equal the reference's, ties included."""
    k, n = ref["k"], min(ref["k"], ref["V"])
    idx, val = idx.detach().cpu().to(torch.int64), val.detach().cpu().double()
    assert bool((idx == ref["cols"][:, :k]).all()), f"{what}: indices {idx.tolist()} vs {ref['cols'][:, :k].tolist()}"
    assert bool((val[:, :n] == ref["xs"][:, :n]).all()) and bool((val[:, n:] == float("-inf")).all()), f"{what}: values differ"


# ================================================================================================ the kernel's path in torch fp32
def topk_f32_path(y, W, bias, V, k, wrong=None):
    """cm3p_mlm_topk in torch fp32: the fp32 logits, per 128-column tile its k candidates by (value descending, column ascending), the
    tiles merged in ascending order (a candidate goes behind every equal value already there), lse by mlm_loss_refs.lse_f32_path.
    wrong: 'pad_as_logits' (the columns [V, Vp) take part), 'ties_high' (equal values rank the higher column first), 'lse_over_vp'
    (only lse sees the pad columns), 'merge_drops_kth' (the merge reads k - 1 candidates of a tile), 'rank_shift' (rank k + 1 is
    returned at rank k).  -> (idx int32 [T, k], val fp32 [T, k], lse fp32 [T])."""
    T = y.shape[0]
    lab = _live(T)
    x = MR._x32(y, W, bias, V, lab, wrong == "pad_as_logits")
    n = x.shape[1]
    kk = k + 1 if wrong == "rank_shift" else k
    tv = torch.full((T, kk), float("-inf"))
    tc = torch.full((T, kk), -1, dtype=torch.int64)
    for c0 in range(0, n, TILE):
        xt = x[:, c0:c0 + TILE]
        w = xt.shape[1]
        if wrong == "ties_high":
            o = (w - 1) - torch.sort(-xt.flip(1), dim=1, stable=True).indices
        else:
            o = torch.sort(-xt, dim=1, stable=True).indices
        m = min(kk - 1 if wrong == "merge_drops_kth" else kk, w)
        cv, cc = xt.gather(1, o[:, :m]), o[:, :m] + c0
        av, ac = torch.cat((tv, cv), 1), torch.cat((tc, cc), 1)
        keep = torch.sort(-av, dim=1, stable=True).indices[:, :kk]  # (what is there stays in front of an equal newcomer)
        tv, tc = av.gather(1, keep), ac.gather(1, keep)
    if wrong == "rank_shift":
        tv, tc = torch.cat((tv[:, :k - 1], tv[:, k:]), 1), torch.cat((tc[:, :k - 1], tc[:, k:]), 1)
    _, lse = MR.lse_f32_path(y, W, bias, V, lab, wrong="pad_as_logits" if wrong in ("pad_as_logits", "lse_over_vp") else None)
    return tc.to(torch.int32), tv, lse
