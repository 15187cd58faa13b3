"""_MLMHeadLogitFreeLossFn (the masked-LM head's loss without the logits tensor) against the node bound of tests/loss_head_refs.py,
|got - R| <= M_NODE |E - R|: R the float64 formula, E the same formula with the bf16 roundings of _MLMHeadLossFn - fp32 logits and a bf16
gradient of the logits, which is what this node computes too.  Every variant the existing node is tested in, each once with the
default chunking (one chunk) and once with 128-row chunks (T = 130 is two chunks, the second of two rows).

Each check prints |got - R| / |E - R| (`pytest -rP`).  CM3P_MLM_LOGIT_FREE_ERRORS_OUT=<file>: write the worst ratios this run measured
there (profiles/mlm_logit_free_err.txt holds one run's)."""
import json
import os

import pytest
import torch

import loss_head_refs as LR
from loss_head_refs import bits_equal, gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_MLM_LOGIT_FREE_ERRORS_OUT")
    if not _SEEN or not path:
        return
    worst = {}
    for seen in _SEEN.values():
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    with open(path, "w") as f:
        json.dump(dict(worst=worst, measured=_SEEN, margin=LR.M_NODE, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f,
                  indent=1, sort_keys=True)


def _note(test, quantity, ratio):
    seen = _SEEN.setdefault(test, {})
    seen[quantity] = max(seen.get(quantity, 0.0), float(ratio))


@pytest.fixture(params=(None, 128), ids=("one chunk", "128-row chunks"))
def chunk(request, monkeypatch):
    from cm3p_amd import modeling_cm3p as M

    monkeypatch.setattr(M, "MLM_LOGIT_FREE_CHUNK_ROWS", request.param)
    return request.param


def _leaves(p, h_dtype, p_dtype, h_grad=True):
    dev, vals = {}, {}
    for k, v in p.items():
        if v is None:
            dev[k] = vals[k] = None
            continue
        t = v.to(h_dtype if k == "h" else p_dtype)
        vals[k] = t.double()
        dev[k] = t.to(DEV).requires_grad_(h_grad if k == "h" else True)
    return dev, vals


def _apply(M, d, lab, num_items=None):
    return M._MLMHeadLogitFreeLossFn.apply(d["h"], d["Wd"], d["bd"], d["nw"], d["Wdec"], d["bdec"], LR.HEAD_EPS, lab, num_items)


def _grads_of(d):
    return {name: (None if d[key] is None else d[key].grad) for name, key in zip(LR.GRADS, ("h", "Wd", "bd", "nw", "Wdec", "bdec"))}


def _run(T, H, V, *, h_dtype=torch.float32, p_dtype=torch.float32, bias=True, num_items=None, lab_form="int64", h_grad=True, labels="quarter",
         test="node"):
    from cm3p_amd import modeling_cm3p as M

    g = gen("head", T, H, V, bias)  # (the data of tests/test_loss_head_gpu.py's node tests)
    p = LR.head_params(T, H, V, g, bias=bias)
    lab = LR.head_labels(T, V, g, labels)
    d, vals = _leaves(p, h_dtype, p_dtype, h_grad)
    B = 5 if T % 5 == 0 else 1
    lab_dev = lab.view(B, T // B).to(DEV)
    if lab_form == "int32":
        lab_dev = lab_dev.to(torch.int32)
    n_ref = ni = None
    if num_items == "int":
        ni = n_ref = 57
    elif num_items == "tensor":
        n_ref, ni = 57, torch.tensor(57, device=DEV)
    dloss = 0.7
    loss = _apply(M, d, lab_dev, ni)
    assert torch.is_tensor(loss) and loss.shape == () and loss.dtype == torch.float32
    (dloss * loss).backward()
    got = _grads_of(d)
    out_bf16 = tuple(n for n, k in zip(LR.GRADS, ("h", "Wd", "bd", "nw", "Wdec", "bdec")) if (h_dtype if k == "h" else p_dtype) == torch.bfloat16)
    R = LR.head_eval(vals, lab, False, num_items=n_ref, dloss=dloss)
    E = LR.head_eval(vals, lab, True, num_items=n_ref, dloss=dloss, out_bf16=out_bf16)
    tag = f"{T}x{H}x{V}"
    _note(test, "node loss", LR.node_check(loss, R["loss"], E["loss"], f"loss {tag}"))
    for name in LR.GRADS:
        if name == "dh" and not h_grad:
            assert got[name] is None
            continue
        if R[name] is None:
            assert got[name] is None, name
            continue
        want_dtype = h_dtype if name == "dh" else p_dtype
        assert got[name] is not None and got[name].dtype == want_dtype and got[name].shape == R[name].shape, (name, got[name].dtype)
        _note(test, f"node {name}", LR.node_check(got[name], R[name], E[name], f"{name} {tag}"))
    if h_grad:
        dead = (~LR.ce_live(lab, V)).to(DEV)
        assert not (got["dh"][dead] != 0).any(), "dh of a row without a label is not zero"
    return dict(d=d, lab_dev=lab_dev, ni=ni, loss=loss, got=got, dloss=dloss, M=M)


@pytest.mark.parametrize("T,H,V", LR.HEAD_SHAPES)
def test_logit_free_node_plain_variant(T, H, V, chunk):
    assert LR.M_NODE == 3.0 <= LR.M_NODE_MAX
    r = _run(T, H, V, test=f"logit-free[{T}-{H}-{V}]")
    M, d = r["M"], r["d"]
    for t in d.values():  # repeatable bits
        if t is not None:
            t.grad = None
    loss = _apply(M, d, r["lab_dev"], r["ni"])
    (r["dloss"] * loss).backward()
    bits_equal(loss, r["loss"].detach().cpu(), "loss again")
    for name, gd in _grads_of(d).items():
        bits_equal(gd, r["got"][name].cpu(), f"{name} again")


@pytest.mark.parametrize("variant", ["h bf16", "no biases", "parameters bf16", "all bf16 no biases", "num_items int", "num_items tensor",
                                     "labels int32", "h without grad", "out of range label", "all labelled"])
def test_logit_free_node_variants(variant, chunk):
    kw = {"h bf16": dict(h_dtype=torch.bfloat16), "no biases": dict(bias=False), "parameters bf16": dict(p_dtype=torch.bfloat16),
          "all bf16 no biases": dict(h_dtype=torch.bfloat16, p_dtype=torch.bfloat16, bias=False),
          "num_items int": dict(num_items="int"), "num_items tensor": dict(num_items="tensor"), "labels int32": dict(lab_form="int32"),
          "h without grad": dict(h_grad=False), "out of range label": dict(labels="out_of_range"), "all labelled": dict(labels="all")}[variant]
    T, H, V = (33, 64, 37) if variant == "all labelled" else (65, 128, 1000) if variant == "parameters bf16" else (130, 64, 37)
    _run(T, H, V, test=f"logit-free[{variant}]", **kw)


@pytest.mark.parametrize("h_dtype,p_dtype,bias", [(torch.float32, torch.float32, True), (torch.bfloat16, torch.bfloat16, False)])
def test_logit_free_node_with_nothing_labelled(h_dtype, p_dtype, bias, chunk):
    from cm3p_amd import modeling_cm3p as M

    T, H, V = 130, 64, 37
    g = gen("head none", bias)
    d, _ = _leaves(LR.head_params(T, H, V, g, bias=bias), h_dtype, p_dtype)
    lab = LR.head_labels(T, V, g, "none").to(DEV)
    loss = _apply(M, d, lab)
    loss.backward()
    assert loss.detach().reshape(1).view(torch.int32).item() == 0, "the loss of a batch without a label is not +0"
    for name, gd in _grads_of(d).items():
        if gd is not None:
            assert bool(torch.isfinite(gd).all()) and not (gd != 0).any(), f"{name} of a batch without a label is not zero"


def test_two_chunks_give_the_rows_one_chunk_gives(monkeypatch):
    """dh rows do not depend on the chunking (each row's dlogits, dgrad and everything below are the same operations): equal in bits.
    dWdec and dbdec sum the chunks in another order: within the node bound (above), not compared in bits."""
    from cm3p_amd import modeling_cm3p as M

    T, H, V = 130, 64, 3167
    g = gen("head", T, H, V, True)
    p, lab = LR.head_params(T, H, V, g), LR.head_labels(T, V, g).to(DEV)
    out = []
    for rows in (None, 128):
        monkeypatch.setattr(M, "MLM_LOGIT_FREE_CHUNK_ROWS", rows)
        d, _ = _leaves(p, torch.float32, torch.float32)
        loss = _apply(M, d, lab)
        loss.backward()
        out.append((loss.detach().cpu(), d["h"].grad.cpu()))
    bits_equal(out[1][0], out[0][0], "loss")
    bits_equal(out[1][1], out[0][1], "dh")
    monkeypatch.setattr(M, "MLM_LOGIT_FREE_CHUNK_ROWS", 100)
    with pytest.raises(ValueError):
        M._mlm_logit_free_chunk_rows(3200)
    monkeypatch.setattr(M, "MLM_LOGIT_FREE_CHUNK_ROWS", None)
    assert M._mlm_logit_free_chunk_rows(3200) == 41856 and M._mlm_logit_free_chunk_rows(50368) == 2560 and M._mlm_logit_free_chunk_rows(2 ** 21) == 128
