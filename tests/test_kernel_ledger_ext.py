"""tests/test_kernel_ledger.py's rule for the extension headers under include/ext/: every function they declare is either in LEDGER,
with the GPU test functions that compare its results with a reference restatement (node ids without parameters), or in EXEMPT with the
reason it has none.  A new entry point there cannot land without one or the other; every header under include/ext/ is read, so neither
can a new header.  No GPU needed: the tests named here are found by parsing their files."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(glob.glob(os.path.join(ROOT, "include", "ext", "*.h")))

MK = "tests/test_mlm_loss_kernels_gpu.py::"
MN = "tests/test_mlm_logit_free_node_gpu.py::"

_BOTH = [MK + "test_every_row_column_and_k_seam_with_and_without_bias", MK + "test_rows_with_exact_logits",
         MK + "test_a_whole_row_tile_ignored_leaves_zeros_and_the_rest_unaffected", MK + "test_offsets_past_2_to_31_elements",
         MN + "test_logit_free_node_plain_variant", MN + "test_logit_free_node_variants"]
LEDGER = {
    "cm3p_mlm_lse": _BOTH,
    "cm3p_mlm_dlogits": _BOTH + [MK + "test_accumulate_sums_two_halves_of_the_rows"],
}

EXEMPT = {
    "cm3p_mlm_loss_abi_version": "host query: ext/cm3p_mlm_loss.h's version number (tests/test_mlm_loss_refs_host.py compares it with the binding)",
    "cm3p_mlm_lse_workspace_bytes": "host query: workspace size of cm3p_mlm_lse (tests/test_mlm_loss_refs_host.py restates its formula)",
    "cm3p_mlm_dlogits_workspace_bytes": "host query: workspace size of cm3p_mlm_dlogits (tests/test_mlm_loss_refs_host.py restates its formula)",
}


def _declared():
    declared = set()
    assert {os.path.basename(h) for h in HEADERS} >= {"cm3p_mlm_loss.h"}
    for header in HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        found = set(re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text))
        assert found, f"no entry point parsed from {header}"
        declared |= found
    return declared


def _test_functions(relpath):
    tree = ast.parse(open(os.path.join(ROOT, relpath)).read())
    return {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}, tree


def test_every_entry_point_under_include_ext_is_in_the_ledger_or_exempt():
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


def test_the_core_ledger_does_not_read_this_directory():
    """include/ext/ is outside tests/test_kernel_ledger.py's glob (include/*.h) and tests/test_cabi.py's header on purpose: the core
    header, its signature table and its ABI number do not move with an extension."""
    import test_kernel_ledger as core

    assert not [h for h in core.HEADERS if os.sep + "ext" + os.sep in h]
    assert not _declared() & (set(core.LEDGER) | set(core.EXEMPT))
