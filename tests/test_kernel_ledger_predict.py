"""tests/test_kernel_ledger_ext.py's rule for the headers under include/ext/predict/: every function they declare is either in LEDGER,
with the GPU test functions that compare its results with a reference restatement (node ids without parameters), or in EXEMPT with the
reason it has none.  A new entry point there cannot land without one or the other; every header of the directory is read, so neither
can a new header.  No GPU needed: the tests named here are found by parsing their files."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(glob.glob(os.path.join(ROOT, "include", "ext", "predict", "*.h")))

TK = "tests/test_mlm_topk_kernels_gpu.py::"
TP = "tests/test_mlm_predict_gpu.py::"

LEDGER = {
    "cm3p_mlm_topk": [TK + "test_every_row_column_and_k_seam_with_and_without_bias", TK + "test_the_model_vocabulary", TK + "test_rows_with_exact_logits",
                      TP + "test_predictions_against_the_full_route", TP + "test_unpadded_execution_and_the_bf16_stream",
                      TP + "test_accuracy_counts_equal_the_reference_arithmetic", TP + "test_the_topk_call_holds_no_logits_sized_tensor"],
}

EXEMPT = {
    "cm3p_mlm_topk_abi_version": "host query: ext/predict/cm3p_mlm_topk.h's version number (tests/test_mlm_topk_refs_host.py compares it with the binding)",
    "cm3p_mlm_topk_workspace_bytes": "host query: workspace size of cm3p_mlm_topk (tests/test_mlm_topk_refs_host.py restates its formula)",
}


def _declared():
    declared = set()
    assert {os.path.basename(h) for h in HEADERS} >= {"cm3p_mlm_topk.h"}
    for header in HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        found = set(re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text))
        assert found, f"no entry point parsed from {header}"
        declared |= found
    return declared


def _test_functions(relpath):
    tree = ast.parse(open(os.path.join(ROOT, relpath)).read())
    return {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}, tree


def test_every_entry_point_under_include_ext_predict_is_in_the_ledger_or_exempt():
    declared = _declared()
    covered = set(LEDGER) | set(EXEMPT)
    assert not declared - covered, f"entry points with neither a test nor an exemption: {sorted(declared - covered)}"
    assert not covered - declared, f"ledger names no longer in a header: {sorted(covered - declared)}"
    assert not set(LEDGER) & set(EXEMPT) and all(LEDGER.values()) and all(r.strip() for r in EXEMPT.values())


def test_every_named_test_exists_and_runs_on_the_gpu():
    missing = []
    for name, ids in LEDGER.items():
        for node in ids:
            path, func = node.split("::")
            assert os.path.exists(os.path.join(ROOT, path)), path
            funcs, tree = _test_functions(path)
            if func not in funcs:
                missing.append((name, node))
            # the file marks its tests `gpu` as a whole
            assert any(isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "pytestmark" and "gpu" in ast.dump(n.value) for n in tree.body), path
    assert not missing, missing


def test_the_other_ledgers_do_not_read_this_directory():
    """include/ext/predict/ is outside tests/test_kernel_ledger.py's glob (include/*.h), tests/test_kernel_ledger_ext.py's
    (include/ext/*.h) and tests/test_cabi.py's header on purpose: their tables and ABI numbers do not move with this extension."""
    import test_kernel_ledger as core
    import test_kernel_ledger_ext as ext

    for other in (core, ext):
        assert not [h for h in other.HEADERS if os.sep + "predict" + os.sep in h]
        assert not _declared() & (set(other.LEDGER) | set(other.EXEMPT))
    assert not _declared() & ext._declared()
