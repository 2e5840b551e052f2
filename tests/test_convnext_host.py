"""No GPU: the ConvNeXt mirrors of richsem_amd/convnext.py on their float64 torch path against tests/golden/layer_convnext_reference.npz
(written by the reference's own classes and autograd, tests/golden/make_golden_convnext.py), the state-dict contract, the refused arguments,
and the host side of the msda_dwconv7_* / msda_layer_scale_* entry points (every argument check comes before any launch: the pointers
below are fake and never dereferenced)."""
import ctypes

import pytest
import torch

import convnext_ref as R
from richsem_amd import _build, _lib, convnext

P = 0x10000      # a 16-byte aligned fake device pointer
NULL_POINTER, BAD_DIMS, TOO_LARGE, MISALIGNED = -1, -2, -4, -5
NET = dict(depths=(1, 1, 2, 1), dims=(32, 64, 96, 128), layer_scale_init_value=1., out_indices=(0, 1, 2, 3))
NET_SHAPES = [(2, 32, 11, 13), (2, 64, 5, 6), (2, 96, 2, 3), (2, 128, 1, 1)]


def _close(name, got):
    want, flat = R.fixture_compare(name, got)
    torch.testing.assert_close(flat, want, rtol=1e-9, atol=1e-10 * float(want.abs().max()) + 1e-12, msg=lambda m: f"{name}: {m}")


def _check_gradients(tag, module, x, outs):
    loss = sum((o * R.fixture_exact(f"{tag}.g{i}")).sum() for i, o in enumerate(outs))
    loss.backward()
    _close(f"{tag}.x_grad", x.grad)
    names = [k for k, _ in module.named_parameters()]
    assert sorted(f"{tag}.grad.{k}" for k in names) == sorted(k for k in R.fixture() if k.startswith(f"{tag}.grad.") and not k.endswith((".stride", ".sum")))
    for k, p in module.named_parameters():
        _close(f"{tag}.grad.{k}", p.grad)


def _block(n, fused=False):
    B, H, W, C = (int(v) for v in R.fixture()[f"block{n}.cfg"])
    blk = convnext.Block(dim=C, layer_scale_init_value=1.).double()
    blk.load_state_dict(R.fixture_state_dict(f"block{n}"), strict=True)
    return blk.set_fused(fused), (B, C, H, W)


def _net(fused=False, **kw):
    net = convnext.ConvNeXt(**{**NET, **kw}).double()
    net.load_state_dict(R.fixture_state_dict("net"), strict=True)
    return net.set_fused(fused)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_block_matches_the_reference_in_float64(n, fused):
    """``fused`` changes nothing on a CPU / float64 tensor"""
    blk, shape = _block(n, fused)
    x = R.fixture_exact(f"block{n}.x").requires_grad_(True)
    assert tuple(x.shape) == shape
    y = blk(x)
    _close(f"block{n}.out0", y)
    _check_gradients(f"block{n}", blk, x, (y,))


@pytest.mark.parametrize("fused", [False, True])
def test_backbone_matches_the_reference_in_float64(fused):
    net = _net(fused)
    img = R.fixture_exact("net.x").requires_grad_(True)
    feats = net.forward_features(img)
    assert [tuple(f.shape) for f in feats] == NET_SHAPES      # the unpadded convolutions drop trailing rows and columns at every level
    for i, f in enumerate(feats):
        _close(f"net.out{i}", f)
    _check_gradients("net", net, img, feats)


def test_channels_last_functions_are_the_block_in_float64():
    """dwconv7 and layer_scale on a CPU float64 map (their torch composition): the block restated channels-last, as the device path runs it"""
    blk, _ = _block(1)
    x = R.fixture_exact("block1.x")
    m = x.permute(0, 2, 3, 1)
    z = convnext.dwconv7(m, blk.dwconv.weight, blk.dwconv.bias)
    z = blk.pwconv2(blk.act(blk.pwconv1(blk.norm(z))))
    _close("block1.out0", convnext.layer_scale(z, blk.gamma, m).permute(0, 3, 1, 2))
    w49 = convnext.dwconv7_weight_form(blk.dwconv.weight)
    assert w49.dtype == torch.float32 and tuple(w49.shape) == (49, 96)
    assert torch.equal(w49[7 * 2 + 5], blk.dwconv.weight[:, 0, 2, 5].float())
    val, _ = R.dwconv_reference(m, w49.double(), blk.dwconv.bias.detach(), None, 0)
    torch.testing.assert_close(val["out"], convnext.dwconv7(m, blk.dwconv.weight, blk.dwconv.bias).detach(), rtol=1e-12, atol=1e-12)


def test_state_dict_keys_are_the_references_both_ways():
    net = convnext.ConvNeXt(**NET).double().set_fused(True)
    stored = R.fixture_state_dict("net")
    assert list(net.state_dict().keys()) == list(stored.keys())
    assert not any("fused" in k for k in net.state_dict())
    for k in ("downsample_layers.0.0.weight", "downsample_layers.1.0.bias", "stages.2.1.dwconv.weight", "stages.0.0.norm.bias",
              "stages.3.0.pwconv1.weight", "stages.1.0.pwconv2.bias", "stages.2.0.gamma", "norm3.weight"):
        assert k in stored, k
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == tuple(stored[k].shape), k
    net.load_state_dict(stored, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        net.load_state_dict({**stored, "head.weight": torch.zeros(1)}, strict=True)
    assert net.dims == NET["dims"] and convnext.Block.fused is False and convnext.ConvNeXt(**NET).fused is False


def test_forward_returns_features_with_interpolated_masks():
    net = _net()
    img = R.fixture_exact("net.x")
    mask = torch.zeros(2, 45, 54, dtype=torch.bool)
    mask[1, :, 30:] = True
    levels = net(img, mask)
    raw = net.forward_features(img)
    assert len(levels) == 4
    for (feat, m), want in zip(levels, raw):
        assert torch.equal(feat, want) and m.dtype == torch.bool and m.shape == (2,) + feat.shape[-2:]
        assert torch.equal(m, torch.nn.functional.interpolate(mask[None].float(), size=feat.shape[-2:]).to(torch.bool)[0])
    assert len(_net(out_indices=(1, 3)).forward_features(img)) == 2


def test_layer_norm_formats_agree():
    gen = torch.Generator().manual_seed(3)
    a, b = convnext.LayerNorm(32).double(), convnext.LayerNorm(32, data_format="channels_first").double()
    assert a.eps == b.eps == 1e-6
    with torch.no_grad():
        for p in list(a.parameters()) + list(b.parameters()):
            p.copy_(torch.randn(32, generator=gen, dtype=torch.float64))
        b.load_state_dict(a.state_dict())
    x = torch.randn(2, 32, 3, 4, generator=gen, dtype=torch.float64)
    torch.testing.assert_close(b(x), a(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2), rtol=1e-12, atol=1e-12)
    with pytest.raises(NotImplementedError):
        convnext.LayerNorm(32, data_format="nchw")


def test_build_convnext_and_exports():
    import richsem_amd
    assert richsem_amd.dwconv7 is convnext.dwconv7 and richsem_amd.ConvNeXt is convnext.ConvNeXt and richsem_amd.build_convnext is convnext.build_convnext
    assert richsem_amd.layer_scale is convnext.layer_scale and richsem_amd.convnext_block is convnext.convnext_block
    with pytest.raises(NotImplementedError, match="pretrained"):
        convnext.build_convnext("convnext_xlarge_22k", True)
    with pytest.raises(ValueError, match="unknown model"):
        convnext.build_convnext("convnext_tiny", False)
    net = convnext.build_convnext("convnext_xlarge_22k", False, depths=[1, 1, 1, 1], out_indices=[3])
    assert net.dims == [256, 512, 1024, 2048] and len(net.stages[2]) == 1
    assert net.stages[0][0].gamma is not None and float(net.stages[0][0].gamma.detach()[0]) == pytest.approx(1e-6)
    assert convnext.Block(32, layer_scale_init_value=0).gamma is None


def test_refusals():
    bf = torch.bfloat16
    blk = convnext.Block(32, drop_path=0.25).set_fused(True)
    assert isinstance(blk.drop_path, convnext.DropPath) and blk.training
    with pytest.raises(NotImplementedError, match="stochastic depth"):      # before anything touches a device
        convnext.convnext_block(torch.zeros(1, 2, 2, 32, dtype=bf), blk)
    blk.eval()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        convnext.convnext_block(torch.zeros(1, 2, 2, 32, dtype=bf), blk)
    w49, w = torch.zeros(49, 32), torch.zeros(32, 1, 7, 7)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        convnext.dwconv7_kernel(torch.zeros(1, 2, 2, 32, dtype=bf), w49)
    with pytest.raises(RuntimeError, match="bfloat16"):
        convnext.dwconv7_kernel(torch.zeros(1, 2, 2, 32), w49)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        convnext.dwconv7_kernel(torch.zeros(1, 2, 2, 48, dtype=bf), torch.zeros(49, 48))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        convnext.dwconv7_kernel(torch.zeros(1, 1, 1, 4128, dtype=bf), torch.zeros(49, 4128))
    with pytest.raises(RuntimeError, match="channels-last map"):
        convnext.dwconv7_kernel(torch.zeros(4, 32, dtype=bf), w49)
    with pytest.raises(RuntimeError, match="channels-last map"):
        convnext.dwconv7_wgrad_kernel(torch.zeros(4, 32, dtype=bf), torch.zeros(4, 32, dtype=bf))
    with pytest.raises(RuntimeError, match=r"weight \(C, 1, 7, 7\)"):      # an NCHW tensor where the map belongs
        convnext.dwconv7(torch.zeros(1, 32, 5, 6), w)
    with pytest.raises(RuntimeError, match=r"weight \(C, 1, 7, 7\)"):
        convnext.dwconv7(torch.zeros(1, 5, 6, 32), torch.zeros(32, 1, 3, 3))
    with pytest.raises(RuntimeError, match="bias"):
        convnext.dwconv7(torch.zeros(1, 5, 6, 32), w, torch.zeros(31))
    with pytest.raises(RuntimeError, match="layer_scale"):
        convnext.layer_scale(torch.zeros(4, 32), torch.zeros(64), torch.zeros(4, 32))
    with pytest.raises(RuntimeError, match="layer_scale"):
        convnext.layer_scale(torch.zeros(4, 32), torch.zeros(32), torch.zeros(5, 32))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        convnext.layer_scale_kernel(torch.zeros(4, 32, dtype=bf), torch.zeros(32), torch.zeros(4, 32, dtype=bf))
    with pytest.raises(RuntimeError, match="bfloat16"):
        convnext.layer_scale_backward_kernel(torch.zeros(4, 32), torch.zeros(4, 32), torch.zeros(32))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        convnext.layer_scale_kernel(torch.zeros(4, 40, dtype=bf), torch.zeros(40), torch.zeros(4, 40, dtype=bf))
    with pytest.raises(ValueError, match="four stages"):
        convnext.ConvNeXt(depths=(1, 1), dims=(32, 64))


# ---- the entry points' argument checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _conv(lib, **kw):
    a = dict(x=P, w=P, bias=P, add=P, flip=0, B=2, H=13, W=9, C=96, out=P)
    a.update(kw)
    return lib.msda_dwconv7_bf16(a["x"], a["w"], a["bias"], a["add"], a["flip"], a["B"], a["H"], a["W"], a["C"], a["out"], None)


def _wgrad(lib, **kw):
    a = dict(dy=P, x=P, B=2, H=13, W=9, C=96, dw=P, dbias=P, ws=P)
    a.update(kw)
    return lib.msda_dwconv7_wgrad_bf16(a["dy"], a["x"], a["B"], a["H"], a["W"], a["C"], a["dw"], a["dbias"], a["ws"], None)


def _scale(lib, **kw):
    a = dict(z=P, gamma=P, res=P, tokens=65, C=96, out=P)
    a.update(kw)
    return lib.msda_layer_scale_forward_bf16(a["z"], a["gamma"], a["res"], a["tokens"], a["C"], a["out"], None)


def _scale_bwd(lib, **kw):
    a = dict(dout=P, z=P, gamma=P, tokens=65, C=96, dz=P, dgamma=P, ws=P)
    a.update(kw)
    return lib.msda_layer_scale_backward_bf16(a["dout"], a["z"], a["gamma"], a["tokens"], a["C"], a["dz"], a["dgamma"], a["ws"], None)


MAP_CASES = [(dict(C=48), BAD_DIMS), (dict(C=0), BAD_DIMS), (dict(C=4128), BAD_DIMS), (dict(B=0), BAD_DIMS), (dict(H=0), BAD_DIMS),
             (dict(W=-1), BAD_DIMS), (dict(B=1 << 12, H=1 << 9, W=1 << 9, C=64), TOO_LARGE)]


@pytest.mark.parametrize("call, entry, cases", [
    (_conv, "msda_dwconv7_bf16", MAP_CASES + [
        (dict(flip=2), BAD_DIMS), (dict(flip=-1), BAD_DIMS), (dict(x=None), NULL_POINTER), (dict(w=None), NULL_POINTER),
        (dict(out=None), NULL_POINTER), (dict(x=P + 8), MISALIGNED), (dict(add=P + 2), MISALIGNED), (dict(out=P + 4), MISALIGNED),
        (dict(w=P + 2), MISALIGNED), (dict(bias=P + 1), MISALIGNED)]),
    (_wgrad, "msda_dwconv7_wgrad_bf16", MAP_CASES + [
        (dict(dy=None), NULL_POINTER), (dict(x=None), NULL_POINTER), (dict(dw=None), NULL_POINTER), (dict(ws=None), NULL_POINTER),
        (dict(dy=P + 8), MISALIGNED), (dict(x=P + 2), MISALIGNED), (dict(dw=P + 2), MISALIGNED), (dict(dbias=P + 1), MISALIGNED),
        (dict(ws=P + 2), MISALIGNED)]),
    (_scale, "msda_layer_scale_forward_bf16", [
        (dict(C=40), BAD_DIMS), (dict(C=4128), BAD_DIMS), (dict(tokens=0), BAD_DIMS), (dict(tokens=1 << 20, C=2048), TOO_LARGE),
        (dict(z=None), NULL_POINTER), (dict(gamma=None), NULL_POINTER), (dict(res=None), NULL_POINTER), (dict(out=None), NULL_POINTER),
        (dict(z=P + 8), MISALIGNED), (dict(res=P + 2), MISALIGNED), (dict(out=P + 4), MISALIGNED), (dict(gamma=P + 2), MISALIGNED)]),
    (_scale_bwd, "msda_layer_scale_backward_bf16", [
        (dict(C=40), BAD_DIMS), (dict(tokens=0), BAD_DIMS), (dict(tokens=1 << 20, C=2048), TOO_LARGE),
        (dict(dout=None), NULL_POINTER), (dict(gamma=None), NULL_POINTER), (dict(dz=None), NULL_POINTER), (dict(ws=None), NULL_POINTER),
        (dict(z=None), NULL_POINTER), (dict(dout=P + 8), MISALIGNED), (dict(z=P + 2), MISALIGNED), (dict(dz=P + 4), MISALIGNED),
        (dict(dgamma=P + 2), MISALIGNED), (dict(ws=P + 1), MISALIGNED)]),
])
def test_entry_points_refuse_before_any_launch(lib, call, entry, cases):
    for kw, code in cases:
        assert call(lib, **kw) == code, kw
        assert _lib.last_error().startswith(entry + ": "), (kw, _lib.last_error())
    with pytest.raises(RuntimeError, match=entry):
        _lib.check(call(lib, C=40))


def test_workspace_bytes(lib):
    n = ctypes.c_int64(0)
    # 512 workgroups are aimed at: 512 / (C / 32) parts at most, each of ceil(tiles / that) (image, 16 x 16 tile) pairs; 50 rows of C floats per part
    for (B, H, W, C), parts in (((2, 13, 9, 96), 2), ((1, 16, 17, 64), 2), ((3, 17, 17, 4096), 4), ((2, 200, 336, 256), 61), ((1, 1, 1, 32), 1)):
        assert lib.msda_dwconv7_workspace_bytes(B, H, W, C, ctypes.byref(n)) == 0
        assert n.value == parts * 50 * C * 4 == convnext.dwconv7_workspace_bytes(B, H, W, C), (B, H, W, C, n.value)
    assert lib.msda_dwconv7_workspace_bytes(2, 13, 9, 96, None) == NULL_POINTER
    assert lib.msda_dwconv7_workspace_bytes(2, 13, 9, 100, ctypes.byref(n)) == BAD_DIMS
    assert _lib.last_error().startswith("msda_dwconv7_workspace_bytes: ")
