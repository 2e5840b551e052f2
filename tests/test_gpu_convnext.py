"""GPU (-m gpu): the ConvNeXt mirrors of richsem_amd/convnext.py on their DEVICE path -- bf16, channels-last, the depthwise-convolution
kernels always and with ``fused`` the library kernels for everything else -- against the float64 fixture of the reference's own classes
(tests/golden/layer_convnext_reference.npz): the four blocks and the toy network, outputs and every gradient (``dwconv.weight``, ``gamma``
and the image gradient included).

The rule is that of tests/test_gpu_swin.py.  Each test also runs a plain torch bf16 composition of the same module in the reference's NCHW
order of operations, written below from the formulas on the fixture's state dict -- not the package's code -- and requires, per tensor,

    err(kernel path, fixture) <= 2 * err(composition, fixture)

with err the root mean square of the difference over the tensor's stored elements.  RICHSEM_REPORT=1 prints both errors per tensor
(recorded in profiles/r34_convnext.md).  That the kernels ran is asserted by counting the calls of the library's entry points."""
import pytest
import torch
import torch.nn.functional as F

import convnext_ref as R
import test_gpu_swin as G

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NET = dict(depths=(1, 1, 2, 1), dims=(32, 64, 96, 128), layer_scale_init_value=1., out_indices=(0, 1, 2, 3))
NET_SHAPES = [(2, 32, 11, 13), (2, 64, 5, 6), (2, 96, 2, 3), (2, 128, 1, 1)]


@pytest.fixture(autouse=True)
def _convnext_fixture(monkeypatch):
    """the comparison helpers of test_gpu_swin read the fixture through their module's ``R``: point them at this file's"""
    monkeypatch.setattr(G, "R", R)


# ---- the composition: NCHW, the reference's order ----------------------------------------------------------------------------------------
def comp_norm_nchw(x, w, b):
    mean = x.mean(1, keepdim=True)
    var = (x - mean).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((x - mean) / torch.sqrt(var + 1e-6)) + b[:, None, None]


def comp_block(P, pre, x):
    C = x.shape[1]
    z = F.conv2d(x, P[pre + "dwconv.weight"], P[pre + "dwconv.bias"], padding=3, groups=C).permute(0, 2, 3, 1)
    z = F.layer_norm(z, (C,), P[pre + "norm.weight"], P[pre + "norm.bias"], 1e-6)
    z = F.linear(F.gelu(F.linear(z, P[pre + "pwconv1.weight"], P[pre + "pwconv1.bias"])), P[pre + "pwconv2.weight"], P[pre + "pwconv2.bias"])
    return x + (P[pre + "gamma"] * z).permute(0, 3, 1, 2)


def comp_net(P, x):
    outs = []
    for i in range(4):
        d = f"downsample_layers.{i}."
        if i == 0:
            x = comp_norm_nchw(F.conv2d(x, P[d + "0.weight"], P[d + "0.bias"], stride=4), P[d + "1.weight"], P[d + "1.bias"])
        else:
            x = F.conv2d(comp_norm_nchw(x, P[d + "0.weight"], P[d + "0.bias"]), P[d + "1.weight"], P[d + "1.bias"], stride=2)
        for j in range(NET["depths"][i]):
            x = comp_block(P, f"stages.{i}.{j}.", x)
        outs.append(comp_norm_nchw(x, P[f"norm{i}.weight"], P[f"norm{i}.bias"]))
    return tuple(outs)


# ---- that the kernels ran ------------------------------------------------------------------------------------------------------------------
class Calls:
    """counts the calls of the library's entry points made through ``_lib.load()``"""

    def __init__(self, monkeypatch):
        from richsem_amd import _lib
        real, self.count = _lib.load(), {}
        outer = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)

                def call(*a):
                    outer.count[name] = outer.count.get(name, 0) + 1
                    return fn(*a)
                return call
        monkeypatch.setattr(_lib, "load", lambda: Proxy())

    def __getitem__(self, name):
        return self.count.get(name, 0)


def _assert_kernels_ran(calls, blocks, fused, downsamples=0, stem=False, norms=0, image_grad=False):
    """per block one forward convolution, one flipped one and one weight gradient on either path; with ``fused`` also the layer scale, the
    products, the LayerNorms, the NCHW norms and the patch rows, counted below; without it none of those"""
    assert calls["msda_dwconv7_bf16"] == 2 * blocks and calls["msda_dwconv7_wgrad_bf16"] == blocks
    if not fused:
        assert calls["msda_layer_scale_forward_bf16"] == 0 and calls["msda_swin_linear_bf16"] == 0 and calls["msda_swin_layernorm_forward_bf16"] == 0
        return
    assert calls["msda_layer_scale_forward_bf16"] == blocks == calls["msda_layer_scale_backward_bf16"]
    # forward products: 2 per block, 1 per downsampling layer, 1 for the stem; backward: 2 per block, 1 per downsampling layer, the stem's
    # only when the image needs a gradient
    assert calls["msda_swin_linear_bf16"] == 4 * blocks + 2 * downsamples + (1 + image_grad) * stem
    assert calls["msda_swin_layernorm_forward_bf16"] == blocks + downsamples + stem == calls["msda_swin_layernorm_backward_bf16"]
    assert calls["msda_swin_norm_nchw_forward_bf16"] == norms == calls["msda_swin_norm_nchw_backward_bf16"]
    assert calls["msda_swin_patch_rows_bf16"] == stem and calls["msda_swin_patch_rows_backward_bf16"] == image_grad * stem


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_block_device_path_against_the_fixture(n, fused, monkeypatch):
    from richsem_amd import convnext
    tag = f"block{n}"
    B, H, W, C = (int(v) for v in R.fixture()[f"{tag}.cfg"])
    sd = R.fixture_state_dict(tag, BF)
    blk = convnext.Block(dim=C, layer_scale_init_value=1.).to(BF)
    blk.load_state_dict(sd, strict=True)
    blk.cuda().set_fused(fused)
    calls = Calls(monkeypatch)
    x = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    y = blk(x)
    assert y.shape == (B, C, H, W) and y.dtype == BF
    G._backward(tag, (y,))
    _assert_kernels_ran(calls, 1, fused)
    kernel = G._results(tag, (y,), x, {k: p.grad for k, p in blk.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
    xc = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    outs = (comp_block(P, "", xc),)
    G._backward(tag, outs)
    G._compare(tag, kernel, G._results(tag, outs, xc, {k: p.grad for k, p in P.items()}))


@pytest.mark.parametrize("fused", [False, True])
def test_toy_backbone_device_path_against_the_fixture(fused, monkeypatch):
    from richsem_amd import convnext
    sd = R.fixture_state_dict("net", BF)
    net = convnext.ConvNeXt(**NET).to(BF)
    net.load_state_dict(sd, strict=True)
    net.cuda().set_fused(fused)
    calls = Calls(monkeypatch)
    img = R.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    feats = net.forward_features(img)
    assert [tuple(f.shape) for f in feats] == NET_SHAPES and all(f.is_contiguous() for f in feats)
    G._backward("net", feats)
    _assert_kernels_ran(calls, sum(NET["depths"]), fused, downsamples=3, stem=True, norms=4, image_grad=True)
    kernel = G._results("net", feats, img, {k: p.grad for k, p in net.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
    imgc = R.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    outs = comp_net(P, imgc)
    G._backward("net", outs)
    G._compare("net", kernel, G._results("net", outs, imgc, {k: p.grad for k, p in P.items()}))
