"""The host-layer rule ("The Python host layer") on the loss side: every library entry point of the focal-negative kernels, the
capacity criterion and the federated class draw is marshalled by exactly one Python function.  ``_lib.py`` declares the ``argtypes`` by hand,
so a second copy of an argument list is a place where two ints can be swapped unnoticed.  A source scan, as
tests/test_dn_queries_host.py::test_each_entry_point_has_one_call_site; no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_CALL_SITE = {
    "msda_focal_neg_sum_f32": "focal.py",
    "msda_focal_neg_grad_f32": "focal.py",
    "msda_focal_neg_sum_masked_f32": "focal.py",
    "msda_focal_neg_grad_masked_f32": "focal.py",
    "msda_criterion_pairs_ex_f32": "criterion.py",
    "msda_criterion_pairs_backward_f32": "criterion.py",
    "msda_criterion_workspace_bytes": "criterion.py",
    "msda_fed_class_mask_f32": "fed_loss.py",
    "msda_fed_class_mask_slots_f32": "fed_loss.py",
}
NO_CALL_SITE = ("msda_criterion_pairs_f32",)      # an export for C callers: the Python path passes flags = 0 to msda_criterion_pairs_ex_f32


def _call_sites(sym):
    hits = []
    for path in sorted(glob.glob(os.path.join(ROOT, "richsem_amd", "*.py"))):
        if os.path.basename(path) != "_lib.py":
            hits += [os.path.basename(path)] * len(re.findall(r"\.%s\(" % sym, open(path, encoding="utf-8").read()))
    return hits


def test_each_loss_entry_point_has_one_call_site():
    for sym, where in ONE_CALL_SITE.items():
        assert _call_sites(sym) == [where], (sym, _call_sites(sym))
    for sym in NO_CALL_SITE:
        assert _call_sites(sym) == [], (sym, _call_sites(sym))


def test_the_focal_module_imports_nothing_of_the_package_but_the_library_binding():
    """focal.py sits under matcher.py, fed_loss.py and criterion.py: it must not import any of them back (nor may fed_loss.py import
    matcher.py or criterion.py)"""
    def package_imports(name):
        text = open(os.path.join(ROOT, "richsem_amd", name), encoding="utf-8").read()
        found = set()
        for m in re.finditer(r"^\s*from \.(\w*) import ([\w, ]+)", text, re.M):
            found |= {m.group(1)} if m.group(1) else {n.strip() for n in m.group(2).split(",")}
        return found
    assert package_imports("focal.py") == {"_lib"}
    assert package_imports("fed_loss.py") <= {"_lib", "focal"}
