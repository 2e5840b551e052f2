"""No GPU: the host side of the Swin block's library path -- the msda_swin_linear_bf16 / msda_swin_layernorm_* entry points are declared,
bound and exported and check every argument before any launch (the pointers below are fake and never dereferenced); the opt-in attribute
``fused`` of the blocks; and the float64 fixture of tests/golden/layer_swin_reference.npz with ``set_fused(True)`` (CPU and fp64 tensors
run the torch formula either way) at the tolerances of tests/test_swin_host.py."""
import ctypes
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
NEW = ("msda_swin_linear_bf16", "msda_swin_layernorm_forward_bf16", "msda_swin_layernorm_workspace_bytes", "msda_swin_layernorm_backward_bf16")
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
    assert "swin_block_mfma.hip" in _build.SOURCES and _build.SOURCES.index("swin_block_mfma.hip") == _build.SOURCES.index("swin_attn_mfma.hip") + 1
    import richsem_amd
    assert richsem_amd.swin_mlp is swin.swin_mlp and richsem_amd.swin_linear is swin.swin_linear and richsem_amd.swin_layernorm is swin.swin_layernorm


def _linear(lib, **kw):
    a = dict(x=P, w=P, bias=P, aux=P, epi=0, T=17, K=96, N=384, out=P, out2=None)
    a.update(kw)
    return lib.msda_swin_linear_bf16(a["x"], a["w"], a["bias"], a["aux"], a["epi"], a["T"], a["K"], a["N"], a["out"], a["out2"], None)


def _ln_fwd(lib, **kw):
    a = dict(x=P, gamma=P, beta=P, T=17, C=96, out=P, mean=P, rstd=P)
    a.update(kw)
    return lib.msda_swin_layernorm_forward_bf16(a["x"], a["gamma"], a["beta"], 1e-5, a["T"], a["C"], a["out"], a["mean"], a["rstd"], None)


def _ln_bwd(lib, **kw):
    a = dict(dy=P, x=P, mean=P, rstd=P, gamma=P, add=P, T=17, C=96, dx=P, dgamma=P, dbeta=P, ws=P)
    a.update(kw)
    return lib.msda_swin_layernorm_backward_bf16(a["dy"], a["x"], a["mean"], a["rstd"], a["gamma"], a["add"], a["T"], a["C"], a["dx"], a["dgamma"],
                                                 a["dbeta"], a["ws"], None)


def _refused(lib, call, entry, cases):
    for kw, code in cases:
        assert call(lib, **kw) == code, kw
        assert _lib.last_error().startswith(entry + ": "), (kw, _lib.last_error())


def test_linear_refuses_before_any_launch(lib):
    _refused(lib, _linear, "msda_swin_linear_bf16", (
        (dict(K=48), BAD_DIMS), (dict(N=0), BAD_DIMS), (dict(N=8224), BAD_DIMS), (dict(K=16), BAD_DIMS), (dict(epi=4), BAD_DIMS),
        (dict(epi=-1), BAD_DIMS), (dict(T=0), BAD_DIMS),
        (dict(epi=2, aux=None), NULL_POINTER), (dict(epi=3, aux=None), NULL_POINTER), (dict(x=None), NULL_POINTER),
        (dict(w=None), NULL_POINTER), (dict(out=None), NULL_POINTER),
        (dict(T=1 << 24, K=128), TOO_LARGE), (dict(T=1 << 24, N=128), TOO_LARGE),
        (dict(x=P + 8), MISALIGNED), (dict(out=P + 2), MISALIGNED), (dict(out2=P + 8, epi=1), MISALIGNED), (dict(aux=P + 4, epi=2), MISALIGNED),
        (dict(bias=P + 2), MISALIGNED)))
    with pytest.raises(RuntimeError, match="msda_swin_linear_bf16"):
        _lib.check(_linear(lib, K=48))


def test_layernorm_refuses_before_any_launch(lib):
    _refused(lib, _ln_fwd, "msda_swin_layernorm_forward_bf16", (
        (dict(C=4128), BAD_DIMS), (dict(C=48), BAD_DIMS), (dict(C=0), BAD_DIMS), (dict(T=0), BAD_DIMS), (dict(T=1 << 20, C=4096), TOO_LARGE),
        (dict(x=None), NULL_POINTER), (dict(gamma=None), NULL_POINTER), (dict(beta=None), NULL_POINTER), (dict(out=None), NULL_POINTER),
        (dict(x=P + 8), MISALIGNED), (dict(out=P + 2), MISALIGNED), (dict(mean=P + 2), MISALIGNED), (dict(gamma=P + 1), MISALIGNED)))
    _refused(lib, _ln_bwd, "msda_swin_layernorm_backward_bf16", (
        (dict(C=4128), BAD_DIMS), (dict(C=48), BAD_DIMS), (dict(T=0), BAD_DIMS), (dict(T=1 << 20, C=4096), TOO_LARGE),
        (dict(dy=None), NULL_POINTER), (dict(mean=None), NULL_POINTER), (dict(rstd=None), NULL_POINTER), (dict(dx=None), NULL_POINTER),
        (dict(ws=None), NULL_POINTER),      # with dgamma or dbeta wanted
        (dict(add=P + 8), MISALIGNED), (dict(dx=P + 2), MISALIGNED), (dict(dgamma=P + 2), MISALIGNED), (dict(ws=P + 1), MISALIGNED)))


def test_layernorm_workspace_bytes(lib):
    n = ctypes.c_int64(0)
    assert lib.msda_swin_layernorm_workspace_bytes(200, 96, ctypes.byref(n)) == 0
    assert n.value == 4 * 2 * 96 * 4 == swin.layernorm_workspace_bytes(200, 96)      # four partial rows of 64 tokens
    assert lib.msda_swin_layernorm_workspace_bytes(64, 32, ctypes.byref(n)) == 0 and n.value == 2 * 32 * 4
    assert lib.msda_swin_layernorm_workspace_bytes(200, 96, None) == NULL_POINTER
    assert lib.msda_swin_layernorm_workspace_bytes(200, 4128, ctypes.byref(n)) == BAD_DIMS
    assert _lib.last_error().startswith("msda_swin_layernorm_workspace_bytes: ")


def test_library_functions_refuse_cpu_tensors():
    x = torch.zeros(4, 32, dtype=torch.bfloat16)
    lin, norm = torch.nn.Linear(32, 32), torch.nn.LayerNorm(32)
    for call in (lambda: swin.swin_linear(x, lin.weight, lin.bias), lambda: swin.swin_layernorm(x, norm.weight, norm.bias),
                 lambda: swin.swin_mlp(x, norm, lin, lin)):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            call()
    with pytest.raises(ValueError, match="epilogue"):
        swin.swin_linear(x, lin.weight, lin.bias, epilogue="gelu")


# ---- the opt-in attribute --------------------------------------------------------------------------------------------------------------
def test_fused_is_off_by_default_not_in_the_state_dict_and_set_on_every_block():
    net = swin.SwinTransformer(**NET)
    blocks = [b for layer in net.layers for b in layer.blocks]
    assert len(blocks) == 4 and not any(b.fused for b in blocks) and swin.SwinTransformerBlock.fused is False
    keys = list(net.state_dict().keys())
    assert net.set_fused(True) is net and all(b.fused is True for b in blocks)
    assert list(net.state_dict().keys()) == keys and not any("fused" in k or "_forms" in k for k in keys)
    net.layers[1].set_fused(False)
    assert [b.fused for b in blocks] == [True, True, False, False]
    net.set_fused(False)
    assert not any(b.fused for b in blocks)
    import inspect
    assert "fused" not in inspect.signature(swin.SwinTransformerBlock.__init__).parameters
    import copy
    assert copy.deepcopy(net.set_fused(True)).layers[0].blocks[0].fused is True


def _close(name, got):
    want, flat = R.fixture_compare(name, got)
    torch.testing.assert_close(flat, want, rtol=1e-9, atol=1e-10 * float(want.abs().max()) + 1e-12, msg=lambda m: f"{name}: {m}")


def _check_gradients(tag, module, x, outs):
    sum((o * R.fixture_exact(f"{tag}.g{i}")).sum() for i, o in enumerate(outs)).backward()
    _close(f"{tag}.x_grad", x.grad)
    for k, p in module.named_parameters():
        _close(f"{tag}.grad.{k}", p.grad)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_basic_layer_with_fused_set_matches_the_reference_in_float64(n):
    H, W, w, nH = (int(v) for v in R.fixture()[f"layer{n}.cfg"])
    layer = swin.BasicLayer(dim=32 * nH, depth=2, num_heads=nH, window_size=w, mlp_ratio=1., downsample=swin.PatchMerging).double()
    layer.load_state_dict(R.fixture_state_dict(f"layer{n}"), strict=True)
    layer.set_fused(True)
    x = R.fixture_exact(f"layer{n}.x").requires_grad_(True)
    x_out, _, _, x_down, _, _ = layer(x, H, W)
    _close(f"layer{n}.out0", x_out)
    _close(f"layer{n}.out1", x_down)
    _check_gradients(f"layer{n}", layer, x, (x_out, x_down))


def test_backbone_with_fused_set_matches_the_reference_in_float64():
    net = swin.SwinTransformer(**NET).double().set_fused(True)
    net.load_state_dict(R.fixture_state_dict("net"), strict=True)
    img = R.fixture_exact("net.x").requires_grad_(True)
    feats = net.forward_raw(img)
    for i, f in enumerate(feats):
        _close(f"net.out{i}", f)
    _check_gradients("net", net, img, feats)


def test_fused_refuses_stochastic_depth_in_training_mode_only_on_the_device_path():
    blk = swin.SwinTransformerBlock(32, 1, window_size=4, drop_path=0.25)
    blk.fused = True
    blk.H = blk.W = 4
    assert blk(torch.zeros(1, 16, 32)).shape == (1, 16, 32)      # CPU fp32: the torch formula, stochastic depth included
    assert "drop_path" in swin.SwinTransformerBlock.__doc__ and "NotImplementedError" in swin.SwinTransformerBlock.__doc__
