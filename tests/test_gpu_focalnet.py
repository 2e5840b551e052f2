"""GPU (-m gpu): the FocalNet mirrors of richsem_amd/focalnet.py on their DEVICE path -- bf16, the context aggregation and the modulation
product on the msda_fmod_* kernels -- against the float64 fixture of the reference's own classes
(tests/golden/layer_focalnet_reference.npz): the ten modulations, the two blocks and the toy network, outputs and every gradient, with
``fused`` off and on.

The rule is that of tests/test_gpu_swin.py.  Each test also runs a plain torch bf16 composition of the same module in the reference's NCHW
order of operations, written from the formulas on the fixture's state dict (tests/focalnet_ref.py: comp_modulation, comp_block; the
network below) -- not the package's code -- and requires, per tensor,

    err(kernel path, fixture) <= 2 * err(composition, fixture)

with err the root mean square of the difference over the tensor's stored elements.  RICHSEM_REPORT=1 prints both errors per tensor
(recorded in profiles/r35_focalnet.md).  That the kernels ran is asserted by counting the calls of the library's entry points."""
import pytest
import torch
import torch.nn.functional as F

import focalnet_ref as R
import test_gpu_swin as G
from test_gpu_convnext import Calls

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NET = dict(embed_dim=32, depths=[1, 2, 1], focal_levels=[3, 4, 3], focal_windows=[5, 3, 5], use_conv_embed=True, use_postln=True,
           use_layerscale=True, normalize_modulator=True, drop_path_rate=0., out_indices=(0, 1, 2), mlp_ratio=1.)
NET_SHAPES = [(2, 32, 12, 14), (2, 64, 6, 7), (2, 128, 3, 4)]
BLOCK_KW = dict(mlp_ratio=1., focal_level=3, focal_window=5, use_postln=True, use_layerscale=True)


@pytest.fixture(autouse=True)
def _focalnet_fixture(monkeypatch):
    """the comparison helpers of test_gpu_swin read the fixture through their module's ``R``: point them at this file's"""
    monkeypatch.setattr(G, "R", R)


def comp_embed(P, pre, x, patch):
    """PatchEmbed with a norm: the map padded to a multiple of ``patch``, the convolution (7 x 7 / 4 / 2 for the stem, 3 x 3 / 2 / 1 else),
    LayerNorm over the channels -> (tokens (B, Wh Ww, C), Wh, Ww)"""
    H, W = x.shape[2:]
    x = F.pad(x, (0, -W % patch, 0, -H % patch))
    stem = patch == 4
    x = F.conv2d(x, P[pre + "proj.weight"], P[pre + "proj.bias"], stride=patch, padding=2 if stem else 1)
    Wh, Ww = x.shape[2:]
    C = x.shape[1]
    return F.layer_norm(x.flatten(2).transpose(1, 2), (C,), P[pre + "norm.weight"], P[pre + "norm.bias"], 1e-5), Wh, Ww


def comp_net(P, img):
    x, H, W = comp_embed(P, "patch_embed.", img, 4)
    outs = []
    for i, depth in enumerate(NET["depths"]):
        for j in range(depth):
            x = R.comp_block(P, f"layers.{i}.blocks.{j}.", x, H, W, NET["focal_levels"][i], True, False)
        B, N, C = x.shape
        out = F.layer_norm(x, (C,), P[f"norm{i}.weight"], P[f"norm{i}.bias"], 1e-5)
        outs.append(out.view(B, H, W, C).permute(0, 3, 1, 2).contiguous())
        if i < len(NET["depths"]) - 1:
            x, H, W = comp_embed(P, f"layers.{i}.downsample.", x.transpose(1, 2).reshape(B, C, H, W), 2)
    return tuple(outs)


def _assert_kernels_ran(calls, modulations, fused, linears=0, norms=0, scales=0, nchw=0):
    """per modulation one context forward, one context backward and the product's two calls on either path; with ``fused`` also the
    products (forward and input gradient: f, h, proj 6 per modulation; fc1, fc2 4 per block), the LayerNorms, the layer scales and the NCHW
    norms, counted by the caller; without it none of those"""
    assert calls["msda_fmod_context_forward_bf16"] == modulations == calls["msda_fmod_context_backward_bf16"]
    assert calls["msda_fmod_modulate_forward_bf16"] == modulations == calls["msda_fmod_modulate_backward_bf16"]
    if not fused:
        linears = norms = scales = nchw = 0
    assert calls["msda_swin_linear_bf16"] == linears
    assert calls["msda_swin_layernorm_forward_bf16"] == norms == calls["msda_swin_layernorm_backward_bf16"]
    assert calls["msda_layer_scale_forward_bf16"] == scales == calls["msda_layer_scale_backward_bf16"]
    assert calls["msda_swin_norm_nchw_forward_bf16"] == nchw == calls["msda_swin_norm_nchw_backward_bf16"]


def _params(sd):
    return {k: v.cuda().requires_grad_(True) for k, v in sd.items()}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", range(10))
def test_modulation_device_path_against_the_fixture(n, fused, monkeypatch):
    from richsem_amd import focalnet
    tag = f"mod{n}"
    B, H, W, C, L, window, normalize = (int(v) for v in R.fixture()[f"{tag}.cfg"])
    sd = R.fixture_state_dict(tag, BF)
    mod = focalnet.FocalModulation(C, focal_level=L, focal_window=window, normalize_modulator=bool(normalize)).to(BF)
    mod.load_state_dict(sd, strict=True)
    mod.cuda().set_fused(fused)
    calls = Calls(monkeypatch)
    x = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    y = mod(x)
    assert y.shape == (B, H, W, C) and y.dtype == BF
    G._backward(tag, (y,))
    _assert_kernels_ran(calls, 1, fused, linears=6)
    kernel = G._results(tag, (y,), x, {k: p.grad for k, p in mod.named_parameters()})

    P = _params(sd)
    xc = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    outs = (R.comp_modulation(P, "", xc, L, bool(normalize), False),)
    G._backward(tag, outs)
    G._compare(tag, kernel, G._results(tag, outs, xc, {k: p.grad for k, p in P.items()}))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", [0, 1])
def test_block_device_path_against_the_fixture(n, fused, monkeypatch):
    from richsem_amd import focalnet
    tag = f"block{n}"
    B, H, W, C, postln = (int(v) for v in R.fixture()[f"{tag}.cfg"])
    sd = R.fixture_state_dict(tag, BF)
    blk = focalnet.FocalModulationBlock(C, use_postln_in_modulation=bool(postln), **BLOCK_KW).to(BF)
    blk.load_state_dict(sd, strict=True)
    blk.cuda().set_fused(fused)
    blk.H, blk.W = H, W
    calls = Calls(monkeypatch)
    x = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    y = blk(x)
    assert y.shape == (B, H * W, C) and y.dtype == BF
    G._backward(tag, (y,))
    _assert_kernels_ran(calls, 1, fused, linears=10, norms=2 + postln, scales=2)
    kernel = G._results(tag, (y,), x, {k: p.grad for k, p in blk.named_parameters()})

    P = _params(sd)
    xc = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    outs = (R.comp_block(P, "", xc, H, W, BLOCK_KW["focal_level"], False, bool(postln)),)
    G._backward(tag, outs)
    G._compare(tag, kernel, G._results(tag, outs, xc, {k: p.grad for k, p in P.items()}))


@pytest.mark.parametrize("fused", [False, True])
def test_toy_backbone_device_path_against_the_fixture(fused, monkeypatch):
    from richsem_amd import focalnet
    sd = R.fixture_state_dict("net", BF)
    net = focalnet.FocalNet(**NET).to(BF)
    net.load_state_dict(sd, strict=True)
    net.cuda().set_fused(fused)
    calls = Calls(monkeypatch)
    img = R.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    feats = net.forward_features(img)
    assert [tuple(f.shape) for f in feats] == NET_SHAPES and all(f.is_contiguous() for f in feats)
    G._backward("net", feats)
    blocks = sum(NET["depths"])      # norms: two per block, the stem's and the two downsampling layers'
    _assert_kernels_ran(calls, blocks, fused, linears=10 * blocks, norms=2 * blocks + 3, scales=2 * blocks, nchw=3)
    kernel = G._results("net", feats, img, {k: p.grad for k, p in net.named_parameters()})

    P = _params(sd)
    imgc = R.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    outs = comp_net(P, imgc)
    G._backward("net", outs)
    G._compare("net", kernel, G._results("net", outs, imgc, {k: p.grad for k, p in P.items()}))
