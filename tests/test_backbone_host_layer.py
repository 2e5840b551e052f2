"""The host-layer rule ("The Python host layer") on the backbone side.  Every library entry point of the Swin, ConvNeXt and
FocalNet kernels is marshalled by exactly one Python function, in the file named here; ``backbone_ops.py`` is a leaf under the three
backbone files, which never import one another, nor any underscore name of the package.  A source scan, as
tests/test_loss_host_layer.py; no GPU."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKBONES = ("swin.py", "convnext.py", "focalnet.py")

ONE_CALL_SITE = {
    "msda_swin_attn_forward_bf16": "swin.py",
    "msda_swin_attn_backward_bf16": "swin.py",
    "msda_swin_attn_workspace_bytes": "swin.py",
    "msda_swin_merge_norm_forward_bf16": "swin.py",
    "msda_swin_merge_norm_backward_bf16": "swin.py",
    "msda_swin_linear_bf16": "backbone_ops.py",
    "msda_swin_layernorm_forward_bf16": "backbone_ops.py",
    "msda_swin_layernorm_backward_bf16": "backbone_ops.py",
    "msda_swin_layernorm_workspace_bytes": "backbone_ops.py",
    "msda_swin_norm_nchw_forward_bf16": "backbone_ops.py",
    "msda_swin_norm_nchw_backward_bf16": "backbone_ops.py",
    "msda_swin_patch_rows_bf16": "backbone_ops.py",
    "msda_swin_patch_rows_backward_bf16": "backbone_ops.py",
    "msda_layer_scale_forward_bf16": "backbone_ops.py",
    "msda_layer_scale_backward_bf16": "backbone_ops.py",
    "msda_dwconv7_bf16": "convnext.py",
    "msda_dwconv7_wgrad_bf16": "convnext.py",
    "msda_dwconv7_workspace_bytes": "convnext.py",
    "msda_fmod_context_forward_bf16": "focalnet.py",
    "msda_fmod_context_backward_bf16": "focalnet.py",
    "msda_fmod_modulate_forward_bf16": "focalnet.py",
    "msda_fmod_modulate_backward_bf16": "focalnet.py",
    "msda_fmod_workspace_bytes": "focalnet.py",
}


def _source(name):
    return open(os.path.join(ROOT, "richsem_amd", name), encoding="utf-8").read()


def _call_sites(sym):
    hits = []
    for path in sorted(glob.glob(os.path.join(ROOT, "richsem_amd", "*.py"))):
        if os.path.basename(path) != "_lib.py":
            hits += [os.path.basename(path)] * len(re.findall(r"\.%s\(" % sym, open(path, encoding="utf-8").read()))
    return hits


def _package_imports(name, inside=None):
    """-> {package module: names imported from it} over every relative import of the file (``from . import m`` counts as module ``m``),
    those inside functions included; ``inside``: of that function alone"""
    tree = ast.parse(_source(name))
    if inside is not None:
        tree, = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == inside]
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level:
            for alias in node.names:
                module = node.module.split(".")[0] if node.module else alias.name
                found.setdefault(module, set()).add(alias.name)
    return found


def test_the_table_names_every_backbone_entry_point():
    from richsem_amd import _lib
    bound = {s for s in _lib.SYMBOLS if s.startswith(("msda_swin_", "msda_dwconv7_", "msda_layer_scale_", "msda_fmod_"))}
    assert bound == set(ONE_CALL_SITE)


def test_each_backbone_entry_point_has_one_call_site():
    for sym, where in ONE_CALL_SITE.items():
        assert _call_sites(sym) == [where], (sym, _call_sites(sym))


def test_the_leaf_module_imports_nothing_of_the_package_but_the_binding_and_the_cache():
    top = _package_imports("backbone_ops.py")
    assert set(top) <= {"_lib", "param_cache", "functions"}, top
    inner = _package_imports("backbone_ops.py", inside="wgrad")      # functions.linear imports conv.py: at call time only
    assert top.get("functions", set()) == inner.get("functions", set()) == {"linear_bgrad", "linear_wgrad"}
    module_level = [n for n in ast.parse(_source("backbone_ops.py")).body if isinstance(n, ast.ImportFrom) and n.level]
    assert {(n.module or n.names[0].name) for n in module_level} <= {"_lib", "param_cache"}


def test_no_backbone_imports_another_nor_an_underscore_name():
    for name in BACKBONES:
        imports = _package_imports(name)
        others = {b[:-3] for b in BACKBONES if b != name}
        assert not others & set(imports), (name, sorted(others & set(imports)))
        assert "backbone_ops" in imports, name
        private = {(m, n) for m, names in imports.items() for n in names if n.startswith("_") and (m, n) != ("_lib", "_lib")}
        assert not private, (name, sorted(private))
        assert not re.search(r"\bbackbone_ops\._", _source(name)), name
