"""No GPU: the host side of the Swin stage boundaries -- the msda_swin_merge_norm_* / msda_swin_norm_nchw_* / msda_swin_patch_rows_* entry
points are declared, bound and exported and check every argument before any launch (the pointers below are fake and never dereferenced);
the opt-in attributes and ``set_fused_stages``; ``PatchEmbed.tokens``; and the float64 fixture of tests/golden/layer_swin_reference.npz with
both switches set (CPU and fp64 tensors run the torch formula either way) at the tolerances of tests/test_swin_host.py."""
import copy
import inspect
import os
import re
import subprocess

import pytest
import torch

import swin_attn_ref as R
from richsem_amd import _build, _lib, swin

P = 0x10000      # a 16-byte aligned fake device pointer
NULL_POINTER, BAD_DIMS, TOO_LARGE, MISALIGNED = -1, -2, -4, -5
NET = dict(embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=7, out_indices=(0, 1), mlp_ratio=2., drop_path_rate=0.)
NEW = ("msda_swin_merge_norm_forward_bf16", "msda_swin_merge_norm_backward_bf16", "msda_swin_norm_nchw_forward_bf16",
       "msda_swin_norm_nchw_backward_bf16", "msda_swin_patch_rows_bf16", "msda_swin_patch_rows_backward_bf16")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "richsem_msda.h")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    header = open(HEADER).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    for sym in NEW:
        assert re.search(r"^int " + sym + r"\(", header, re.M), sym
        assert sym in _lib.SYMBOLS and getattr(lib, sym).argtypes is not None, sym
        assert re.search(r" T " + sym + r"$", exported, re.M), sym
    assert _lib.ABI_VERSION == 13 == lib.msda_abi_version()
    assert "#define RICHSEM_MSDA_ABI_VERSION 13" in header
    assert _build.SOURCES.index("swin_stage.hip") == _build.SOURCES.index("swin_block_mfma.hip") + 1
    import richsem_amd
    assert richsem_amd.swin_merge_norm is swin.swin_merge_norm and richsem_amd.swin_norm_nchw is swin.swin_norm_nchw
    assert richsem_amd.swin_patch_rows is swin.swin_patch_rows


def _merge_fwd(lib, **kw):
    a = dict(x=P, gamma=P, beta=P, B=2, H=13, W=9, C=96, out=P, mean=P, rstd=P)
    a.update(kw)
    return lib.msda_swin_merge_norm_forward_bf16(a["x"], a["gamma"], a["beta"], 1e-5, a["B"], a["H"], a["W"], a["C"], a["out"], a["mean"], a["rstd"], None)


def _merge_bwd(lib, **kw):
    a = dict(dy=P, x=P, mean=P, rstd=P, gamma=P, B=2, H=13, W=9, C=96, dx=P, dgamma=P, dbeta=P, ws=P)
    a.update(kw)
    return lib.msda_swin_merge_norm_backward_bf16(a["dy"], a["x"], a["mean"], a["rstd"], a["gamma"], a["B"], a["H"], a["W"], a["C"], a["dx"],
                                                  a["dgamma"], a["dbeta"], a["ws"], None)


def _nchw_fwd(lib, **kw):
    a = dict(x=P, gamma=P, beta=P, B=2, HW=35, C=64, out=P, mean=P, rstd=P)
    a.update(kw)
    return lib.msda_swin_norm_nchw_forward_bf16(a["x"], a["gamma"], a["beta"], 1e-5, a["B"], a["HW"], a["C"], a["out"], a["mean"], a["rstd"], None)


def _nchw_bwd(lib, **kw):
    a = dict(dy=P, x=P, mean=P, rstd=P, gamma=P, B=2, HW=35, C=64, dx=P, dgamma=P, dbeta=P, ws=P)
    a.update(kw)
    return lib.msda_swin_norm_nchw_backward_bf16(a["dy"], a["x"], a["mean"], a["rstd"], a["gamma"], a["B"], a["HW"], a["C"], a["dx"], a["dgamma"],
                                                 a["dbeta"], a["ws"], None)


def _patch(lib, backward=False, **kw):
    a = dict(src=P, B=1, Cin=3, H=13, W=18, ph=4, pw=4, dst=P)
    a.update(kw)
    f = lib.msda_swin_patch_rows_backward_bf16 if backward else lib.msda_swin_patch_rows_bf16
    return f(a["src"], a["B"], a["Cin"], a["H"], a["W"], a["ph"], a["pw"], a["dst"], None)


def _patch_bwd(lib, **kw):
    return _patch(lib, backward=True, **kw)


def _refused(lib, call, entry, cases):
    for kw, code in cases:
        assert call(lib, **kw) == code, kw
        assert _lib.last_error().startswith(entry + ": "), (kw, _lib.last_error())


def test_merge_norm_refuses_before_any_launch(lib):
    _refused(lib, _merge_fwd, "msda_swin_merge_norm_forward_bf16", (
        (dict(C=1056), BAD_DIMS), (dict(C=48), BAD_DIMS), (dict(C=0), BAD_DIMS), (dict(B=0), BAD_DIMS), (dict(H=0), BAD_DIMS), (dict(W=-1), BAD_DIMS),
        (dict(B=1 << 10, H=1 << 10, W=1 << 10, C=32), TOO_LARGE), (dict(B=1, H=1, W=(1 << 26) - 1, C=32), TOO_LARGE),      # (the rows' 4 C alone)
        (dict(x=None), NULL_POINTER), (dict(gamma=None), NULL_POINTER), (dict(beta=None), NULL_POINTER), (dict(out=None), NULL_POINTER),
        (dict(x=P + 8), MISALIGNED), (dict(out=P + 2), MISALIGNED), (dict(mean=P + 2), MISALIGNED), (dict(gamma=P + 1), MISALIGNED)))
    _refused(lib, _merge_bwd, "msda_swin_merge_norm_backward_bf16", (
        (dict(C=1056), BAD_DIMS), (dict(C=48), BAD_DIMS), (dict(H=0), BAD_DIMS), (dict(B=1 << 10, H=1 << 10, W=1 << 10, C=32), TOO_LARGE),
        (dict(dy=None), NULL_POINTER), (dict(x=None), NULL_POINTER), (dict(mean=None), NULL_POINTER), (dict(rstd=None), NULL_POINTER),
        (dict(gamma=None), NULL_POINTER), (dict(dx=None), NULL_POINTER), (dict(ws=None), NULL_POINTER), (dict(ws=None, dgamma=None), NULL_POINTER),
        (dict(dy=P + 8), MISALIGNED), (dict(dx=P + 2), MISALIGNED), (dict(dgamma=P + 2), MISALIGNED), (dict(ws=P + 1), MISALIGNED)))
    with pytest.raises(RuntimeError, match="msda_swin_merge_norm_forward_bf16"):
        _lib.check(_merge_fwd(lib, C=48))


def test_norm_nchw_refuses_before_any_launch(lib):
    _refused(lib, _nchw_fwd, "msda_swin_norm_nchw_forward_bf16", (
        (dict(C=4128), BAD_DIMS), (dict(C=48), BAD_DIMS), (dict(C=0), BAD_DIMS), (dict(B=0), BAD_DIMS), (dict(HW=0), BAD_DIMS),
        (dict(B=1 << 10, HW=1 << 10, C=4096), TOO_LARGE), (dict(B=1 << 16, HW=1 << 16, C=32), TOO_LARGE),
        (dict(x=None), NULL_POINTER), (dict(gamma=None), NULL_POINTER), (dict(beta=None), NULL_POINTER), (dict(out=None), NULL_POINTER),
        (dict(x=P + 8), MISALIGNED), (dict(out=P + 2), MISALIGNED), (dict(rstd=P + 2), MISALIGNED), (dict(beta=P + 1), MISALIGNED)))
    _refused(lib, _nchw_bwd, "msda_swin_norm_nchw_backward_bf16", (
        (dict(C=4128), BAD_DIMS), (dict(C=48), BAD_DIMS), (dict(HW=0), BAD_DIMS), (dict(B=1 << 10, HW=1 << 10, C=4096), TOO_LARGE),
        (dict(dy=None), NULL_POINTER), (dict(x=None), NULL_POINTER), (dict(mean=None), NULL_POINTER), (dict(rstd=None), NULL_POINTER),
        (dict(gamma=None), NULL_POINTER), (dict(dx=None), NULL_POINTER), (dict(ws=None), NULL_POINTER),
        (dict(dy=P + 8), MISALIGNED), (dict(dx=P + 2), MISALIGNED), (dict(dbeta=P + 2), MISALIGNED), (dict(ws=P + 1), MISALIGNED)))


def test_patch_rows_refuse_before_any_launch(lib):
    for call, entry in ((_patch, "msda_swin_patch_rows_bf16"), (_patch_bwd, "msda_swin_patch_rows_backward_bf16")):
        _refused(lib, call, entry, (
            (dict(B=0), BAD_DIMS), (dict(Cin=0), BAD_DIMS), (dict(H=0), BAD_DIMS), (dict(W=0), BAD_DIMS), (dict(ph=0), BAD_DIMS), (dict(pw=-4), BAD_DIMS),
            (dict(Cin=513), BAD_DIMS),      # Kp = 8224
            (dict(B=1 << 10, Cin=3, H=1 << 10, W=1 << 10), TOO_LARGE), (dict(B=1, Cin=1, H=1 << 14, W=1 << 14, ph=1, pw=1), TOO_LARGE),      # (rows x 32)
            (dict(src=None), NULL_POINTER), (dict(dst=None), NULL_POINTER)))
    _refused(lib, _patch, "msda_swin_patch_rows_bf16", ((dict(src=P + 1), MISALIGNED), (dict(dst=P + 8), MISALIGNED), (dict(dst=P + 2), MISALIGNED)))
    _refused(lib, _patch_bwd, "msda_swin_patch_rows_backward_bf16", ((dict(src=P + 8), MISALIGNED), (dict(dst=P + 1), MISALIGNED)))


def test_library_functions_refuse_cpu_tensors():
    x = torch.zeros(2, 15, 32, dtype=torch.bfloat16)
    n4, n1 = torch.nn.LayerNorm(128), torch.nn.LayerNorm(32)
    for call in (lambda: swin.swin_merge_norm(x, 3, 5, n4.weight, n4.bias, 1e-5), lambda: swin.swin_norm_nchw(x, 3, 5, n1.weight, n1.bias, 1e-5),
                 lambda: swin.swin_patch_rows(torch.zeros(1, 3, 8, 8, dtype=torch.bfloat16), 4)):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            call()
    assert swin.patch_width(3, 4) == 64 and swin.patch_width(5, (2, 4)) == 64 and swin.patch_width(2, 4) == 32
    assert swin.patch_grid(13, 18, 4) == (4, 5)


# ---- the opt-in attributes -------------------------------------------------------------------------------------------------------------
def _stage_flags(net):
    return [net.patch_embed.fused] + [layer.downsample.fused for layer in net.layers if layer.downsample is not None] + [net.fused_stages]


def test_stage_switch_is_off_by_default_not_in_the_state_dict_and_apart_from_the_blocks():
    net = swin.SwinTransformer(**NET)
    blocks = [b for layer in net.layers for b in layer.blocks]
    assert swin.PatchMerging.fused is False and swin.PatchEmbed.fused is False and swin.SwinTransformer.fused_stages is False
    assert _stage_flags(net) == [False, False, False] and net.layers[1].downsample is None
    keys = list(net.state_dict().keys())
    assert net.set_fused_stages() is net and _stage_flags(net) == [True, True, True] and not any(b.fused for b in blocks)
    assert list(net.state_dict().keys()) == keys and not any("fused" in k or "_forms" in k for k in keys)
    assert _stage_flags(copy.deepcopy(net)) == [True, True, True]
    net.set_fused(True)
    assert _stage_flags(net) == [True, True, True] and all(b.fused for b in blocks)
    net.set_fused_stages(False)
    assert _stage_flags(net) == [False, False, False] and all(b.fused for b in blocks)
    net.set_fused(False).set_fused_stages(True)
    net.set_fused(True).set_fused(False)
    assert _stage_flags(net) == [True, True, True] and not any(b.fused for b in blocks)
    layer = swin.BasicLayer(dim=32, depth=2, num_heads=1, downsample=swin.PatchMerging).set_fused(True)
    assert layer.downsample.fused is False
    for cls in (swin.PatchMerging, swin.PatchEmbed, swin.SwinTransformer, swin.BasicLayer):
        assert not any("fused" in p for p in inspect.signature(cls.__init__).parameters), cls


def _close(name, got):
    want, flat = R.fixture_compare(name, got)
    torch.testing.assert_close(flat, want, rtol=1e-9, atol=1e-10 * float(want.abs().max()) + 1e-12, msg=lambda m: f"{name}: {m}")


def _check_gradients(tag, module, x, outs):
    sum((o * R.fixture_exact(f"{tag}.g{i}")).sum() for i, o in enumerate(outs)).backward()
    _close(f"{tag}.x_grad", x.grad)
    for k, p in module.named_parameters():
        _close(f"{tag}.grad.{k}", p.grad)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_basic_layer_with_both_switches_set_matches_the_reference_in_float64(n):
    H, W, w, nH = (int(v) for v in R.fixture()[f"layer{n}.cfg"])
    layer = swin.BasicLayer(dim=32 * nH, depth=2, num_heads=nH, window_size=w, mlp_ratio=1., downsample=swin.PatchMerging).double()
    layer.load_state_dict(R.fixture_state_dict(f"layer{n}"), strict=True)
    layer.set_fused(True).downsample.fused = True
    x = R.fixture_exact(f"layer{n}.x").requires_grad_(True)
    x_out, _, _, x_down, _, _ = layer(x, H, W)
    _close(f"layer{n}.out0", x_out)
    _close(f"layer{n}.out1", x_down)
    _check_gradients(f"layer{n}", layer, x, (x_out, x_down))


def test_backbone_with_both_switches_set_matches_the_reference_in_float64():
    net = swin.SwinTransformer(**NET).double().set_fused(True).set_fused_stages(True)
    net.load_state_dict(R.fixture_state_dict("net"), strict=True)
    img = R.fixture_exact("net.x").requires_grad_(True)
    feats = net.forward_raw(img)
    for i, f in enumerate(feats):
        _close(f"net.out{i}", f)
    _check_gradients("net", net, img, feats)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("shape, norm", [((2, 3, 40, 52), torch.nn.LayerNorm), ((2, 3, 13, 18), torch.nn.LayerNorm), ((1, 3, 13, 18), None)])
def test_patch_embed_tokens_agree_with_forward_in_float64(shape, norm, fused):
    torch.manual_seed(3)
    embed = swin.PatchEmbed(4, 3, 32, norm).double()
    embed.fused = fused
    img = torch.randn(*shape, dtype=torch.float64)
    tok, Wh, Ww = embed.tokens(img)
    out = embed(img)
    assert (Wh, Ww) == (-(-shape[2] // 4), -(-shape[3] // 4)) == tuple(out.shape[2:]) and tok.shape == (shape[0], Wh * Ww, 32)
    assert torch.equal(tok, out.flatten(2).transpose(1, 2))


def test_ape_keeps_the_map_path_with_the_stages_set():
    torch.manual_seed(4)
    net = swin.SwinTransformer(pretrain_img_size=28, ape=True, **NET).double()
    img = torch.randn(1, 3, 28, 28, dtype=torch.float64)
    with torch.no_grad():
        want = net.forward_raw(img)
        got = net.set_fused_stages(True).forward_raw(img)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
