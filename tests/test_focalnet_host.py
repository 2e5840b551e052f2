"""No GPU: the FocalNet mirrors of richsem_amd/focalnet.py on their float64 torch path against tests/golden/layer_focalnet_reference.npz
(written by the reference's own classes and autograd, tests/golden/make_golden_focalnet.py), the state-dict contract, the named models'
arguments, the fallback rule, the refused arguments, ``use_checkpoint``, and the host side of the msda_fmod_* entry points (every argument
check comes before any launch: the pointers below are fake and never dereferenced)."""
import ctypes

import pytest
import torch

import focalnet_ref as R
from richsem_amd import _build, _lib, focalnet

P = 0x10000      # a 16-byte aligned fake device pointer
NULL_POINTER, BAD_DIMS, TOO_LARGE, MISALIGNED = -1, -2, -4, -5
NET = dict(embed_dim=32, depths=[1, 2, 1], focal_levels=[3, 4, 3], focal_windows=[5, 3, 5], use_conv_embed=True, use_postln=True,
           use_layerscale=True, normalize_modulator=True, drop_path_rate=0., out_indices=(0, 1, 2), mlp_ratio=1.)
NET_SHAPES = [(2, 32, 12, 14), (2, 64, 6, 7), (2, 128, 3, 4)]
BLOCK_KW = dict(mlp_ratio=1., focal_level=3, focal_window=5, use_postln=True, use_layerscale=True)


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


def _modulation(n):
    B, H, W, C, L, window, normalize = (int(v) for v in R.fixture()[f"mod{n}.cfg"])
    mod = focalnet.FocalModulation(C, focal_level=L, focal_window=window, normalize_modulator=bool(normalize)).double()
    mod.load_state_dict(R.fixture_state_dict(f"mod{n}"), strict=True)
    return mod, (B, H, W, C)


def _block(n):
    B, H, W, C, postln = (int(v) for v in R.fixture()[f"block{n}.cfg"])
    blk = focalnet.FocalModulationBlock(C, use_postln_in_modulation=bool(postln), **BLOCK_KW).double()
    blk.load_state_dict(R.fixture_state_dict(f"block{n}"), strict=True)
    blk.H, blk.W = H, W
    return blk, (B, H * W, C)


def _net(**kw):
    net = focalnet.FocalNet(**{**NET, **kw}).double()
    net.load_state_dict(R.fixture_state_dict("net"), strict=True)
    return net


@pytest.mark.parametrize("n", range(10))
def test_modulation_matches_the_reference_in_float64(n):
    mod, shape = _modulation(n)
    x = R.fixture_exact(f"mod{n}.x").requires_grad_(True)
    assert tuple(x.shape) == shape
    y = mod(x)
    _close(f"mod{n}.out0", y)
    _check_gradients(f"mod{n}", mod, x, (y,))


@pytest.mark.parametrize("n", [0, 1])
def test_block_matches_the_reference_in_float64(n):
    blk, shape = _block(n)
    x = R.fixture_exact(f"block{n}.x").requires_grad_(True)
    assert tuple(x.shape) == shape
    y = blk(x)
    _close(f"block{n}.out0", y)
    _check_gradients(f"block{n}", blk, x, (y,))


def test_backbone_matches_the_reference_in_float64():
    net = _net()
    img = R.fixture_exact("net.x").requires_grad_(True)
    feats = net.forward_features(img)
    assert [tuple(f.shape) for f in feats] == NET_SHAPES
    for i, f in enumerate(feats):
        _close(f"net.out{i}", f)
    _check_gradients("net", net, img, feats)


def test_use_checkpoint_gives_the_same_gradients():
    img = R.fixture_exact("net.x")
    grads = []
    for flag in (False, True):
        net = _net(use_checkpoint=flag)
        assert all(layer.use_checkpoint is flag for layer in net.layers)
        x = img.clone().requires_grad_(True)
        feats = net.forward_features(x)
        sum((f * R.fixture_exact(f"net.g{i}")).sum() for i, f in enumerate(feats)).backward()
        grads.append([x.grad] + [p.grad for p in net.parameters()])
    for a, b in zip(*grads):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-14)


def test_the_composition_is_the_helpers_definition():
    """focal_context on a CPU float64 map (its torch composition) against tests/focalnet_ref.py's chained formulas"""
    shape, (L, window, normalize) = (2, 5, 4, 32), R.CONFIGS[1]
    ctx0, gates, ws, _ = R.make_inputs(shape, L, window, torch.Generator().manual_seed(1))
    C = shape[-1]
    params = [w.double().t().reshape(C, 1, K, K).contiguous() for w, K in zip(ws, R.sizes(L, window))]
    A = focalnet.focal_context(ctx0.double(), gates.double(), params, normalize)
    stored, x = {}, ctx0.double()
    for l, K in enumerate(R.sizes(L, window)):
        stored[f"u{l}"] = R.conv(x, ws[l].double(), K)
        x = R.gelu(stored[f"u{l}"])
    stored["m"] = x.mean((1, 2))
    stored["g"] = R.gelu(stored["m"])
    val, _ = R.forward_reference(ctx0, gates, ws, L, window, normalize, stored)
    torch.testing.assert_close(A, val["A"], rtol=1e-10, atol=1e-12)
    form = focalnet.focal_weight_form(params)
    assert form.dtype == torch.float32 and tuple(form.shape) == (9 + 25 + 49 + 81, C) and torch.equal(form, R.weight_form(ws))
    assert torch.equal(form[9 + 5 * 1 + 3], params[1][:, 0, 1, 3].float())


def test_state_dict_keys_are_the_references_both_ways():
    net = focalnet.FocalNet(**NET).double()
    stored = R.fixture_state_dict("net")
    assert list(net.state_dict().keys()) == list(stored.keys())
    for k in ("patch_embed.proj.weight", "patch_embed.norm.bias", "layers.1.blocks.1.gamma_1", "layers.0.blocks.0.gamma_2",
              "layers.0.blocks.0.norm1.weight", "layers.1.blocks.0.modulation.f.weight", "layers.1.blocks.0.modulation.h.bias",
              "layers.2.blocks.0.modulation.proj.weight", "layers.1.blocks.1.modulation.focal_layers.3.0.weight", "layers.0.blocks.0.norm2.bias",
              "layers.2.blocks.0.mlp.fc1.weight", "layers.0.blocks.0.mlp.fc2.bias", "layers.0.downsample.proj.weight", "layers.1.downsample.norm.weight",
              "norm2.weight"):
        assert k in stored, k
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == tuple(stored[k].shape), k
    net.load_state_dict(stored, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        net.load_state_dict({**stored, "head.weight": torch.zeros(1)}, strict=True)
    blk, _ = _block(1)
    assert "modulation.ln.weight" in blk.state_dict() and "modulation.ln.weight" not in _block(0)[0].state_dict()
    assert focalnet.FocalModulationBlock(32).gamma_1 == 1.0 and "gamma_1" not in focalnet.FocalModulationBlock(32).state_dict()
    assert tuple(net.patch_embed.proj.kernel_size) == (7, 7) and tuple(net.patch_embed.proj.stride) == (4, 4) and tuple(net.patch_embed.proj.padding) == (2, 2)
    assert tuple(net.layers[0].downsample.proj.kernel_size) == (3, 3) and tuple(net.layers[0].downsample.proj.stride) == (2, 2)
    plain = focalnet.PatchEmbed(patch_size=4, embed_dim=32)
    assert tuple(plain.proj.kernel_size) == (4, 4) and plain.norm is None and plain(torch.zeros(1, 3, 9, 10)).shape == (1, 32, 3, 3)


def test_forward_returns_features_with_interpolated_masks_and_frozen_stages():
    net = _net()
    img = R.fixture_exact("net.x")
    mask = torch.zeros(2, 45, 54, dtype=torch.bool)
    mask[1, :, 30:] = True
    levels = net(img, mask)
    raw = net.forward_features(img)
    assert len(levels) == 3
    for (feat, m), want in zip(levels, raw):
        assert torch.equal(feat, want) and m.dtype == torch.bool and m.shape == (2,) + feat.shape[-2:]
        assert torch.equal(m, torch.nn.functional.interpolate(mask[None].float(), size=feat.shape[-2:]).to(torch.bool)[0])
    two = _net_subset((0, 2))
    assert len(two.forward_features(img)) == 2 and not hasattr(two, "norm1")
    frozen = focalnet.FocalNet(**{**NET, "frozen_stages": 2}).train()
    assert not frozen.patch_embed.training and not any(p.requires_grad for p in frozen.patch_embed.parameters())
    assert not frozen.layers[0].training and not any(p.requires_grad for p in frozen.layers[0].parameters())
    assert frozen.layers[1].training and all(p.requires_grad for p in frozen.layers[1].parameters())


def _net_subset(out_indices):
    net = focalnet.FocalNet(**{**NET, "out_indices": out_indices}).double()
    stored = {k: v for k, v in R.fixture_state_dict("net").items() if not k.startswith("norm") or int(k[4]) in out_indices}
    net.load_state_dict(stored, strict=True)
    return net


def test_named_models_and_exports():
    import richsem_amd
    assert richsem_amd.focal_context is focalnet.focal_context and richsem_amd.FocalNet is focalnet.FocalNet
    assert richsem_amd.build_focalnet is focalnet.build_focalnet and richsem_amd.FocalModulation is focalnet.FocalModulation
    common = dict(depths=[2, 2, 18, 2], use_conv_embed=True, use_postln=True, use_layerscale=True)
    want = {
        "focalnet_L_384_22k": dict(common, embed_dim=192, focal_levels=[3] * 4, focal_windows=[5] * 4, use_postln_in_modulation=False,
                                   normalize_modulator=False),
        "focalnet_L_384_22k_fl4": dict(common, embed_dim=192, focal_levels=[4] * 4, focal_windows=[3] * 4, use_postln_in_modulation=False,
                                       normalize_modulator=True, drop_path_rate=0.3),
        "focalnet_XL_384_22k": dict(common, embed_dim=256, focal_levels=[3] * 4, focal_windows=[5] * 4, use_postln_in_modulation=False,
                                    normalize_modulator=False),
        "focalnet_H_224_22k_fl4_fd": dict(common, embed_dim=352, focal_levels=[4] * 4, focal_windows=[3] * 4, use_postln_in_modulation=True,
                                          normalize_modulator=False),
    }
    assert set(want) == set(focalnet.MODELS)
    for name, cfg in want.items():
        assert focalnet.focalnet_config(name) == cfg, name
        sizes = [w + 2 * l for w, L in zip(cfg["focal_windows"], cfg["focal_levels"]) for l in range(L)]
        assert all(k in focalnet.KERNEL_SIZES for k in sizes)      # every level of every named model is a kernel size
    assert focalnet.focalnet_config("focalnet_L_384_22k", focal_levels=2, out_indices=(1, 2, 3))["focal_levels"] == [2] * 4
    with pytest.raises(NotImplementedError, match="pretrained"):
        focalnet.build_focalnet("focalnet_L_384_22k", True)
    with pytest.raises(NotImplementedError, match="pretrained"):
        focalnet.build_focalnet("focalnet_L_384_22k", pretrained="focalnet_large_lrf_384.pth")
    with pytest.raises(ValueError, match="unknown model"):
        focalnet.build_focalnet("focalnet_tiny")
    net = focalnet.build_focalnet("focalnet_H_224_22k_fl4_fd", embed_dim=32, depths=[1, 1, 1, 1], out_indices=(3,), use_checkpoint=True)
    blk = net.layers[2].blocks[0]
    assert net.num_features == [32, 64, 128, 256] and blk.modulation.use_postln_in_modulation and blk.use_postln and net.layers[3].use_checkpoint
    assert [layer[0].kernel_size[0] for layer in blk.modulation.focal_layers] == [3, 5, 7, 9]
    assert float(blk.gamma_1.detach()[0]) == pytest.approx(1e-4) and isinstance(net.layers[3].blocks[0].drop_path, focalnet.DropPath)


def test_the_fallback_rule():
    bf = torch.bfloat16
    assert focalnet.kernel_shape(96, (5, 7, 9)) and focalnet.kernel_shape(4096, (3, 5, 7, 9)) and focalnet.kernel_shape(32, (9,))
    assert not focalnet.kernel_shape(96, (9, 11))      # the bare classes' default: focal_window 9, two levels
    assert not focalnet.kernel_shape(48, (3, 5)) and not focalnet.kernel_shape(4128, (3,)) and not focalnet.kernel_shape(32, ())
    assert not focalnet.kernel_shape(32, (3, 7)) and not focalnet.kernel_shape(32, (1, 3)) and not focalnet.kernel_shape(32, (3, 5, 7, 9, 11))
    assert not focalnet.kernel_path(torch.zeros(1, 2, 2, 32, dtype=bf), (3, 5))      # a CPU tensor
    assert not focalnet.kernel_path(torch.zeros(1, 2, 2, 32), (3, 5))
    # ... so a CPU bf16 tensor and the default K = 11 run the composition
    gen = torch.Generator().manual_seed(2)
    mod = focalnet.FocalModulation(32, focal_level=2, focal_window=9)
    assert mod(torch.randn(1, 3, 4, 32, generator=gen)).shape == (1, 3, 4, 32)
    ws = [torch.randn(32, 1, 3, 3, generator=gen), torch.randn(32, 1, 5, 5, generator=gen)]
    ctx0, gates = torch.randn(1, 3, 4, 32, generator=gen), torch.randn(1, 3, 4, 3, generator=gen)
    a16 = focalnet.focal_context(ctx0.to(bf), gates.to(bf), [w.to(bf) for w in ws], True)
    assert a16.dtype == bf
    torch.testing.assert_close(a16.float(), focalnet.focal_context(ctx0, gates, ws, True), rtol=0.1, atol=0.1)
    assert torch.equal(focalnet.modulate(ctx0, ctx0), ctx0 * ctx0)


def test_refusals():
    bf = torch.bfloat16
    ctx0, gates, form = torch.zeros(1, 2, 2, 32, dtype=bf), torch.zeros(1, 2, 2, 3, dtype=bf), torch.zeros(34, 32)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        focalnet.context_forward_kernel(ctx0, gates, form, (3, 5), False)
    with pytest.raises(RuntimeError, match="bfloat16"):
        focalnet.context_forward_kernel(ctx0.float(), gates, form, (3, 5), False)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        focalnet.context_forward_kernel(torch.zeros(1, 2, 2, 48, dtype=bf), gates, torch.zeros(34, 48), (3, 5), False)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        focalnet.context_forward_kernel(ctx0, gates, torch.zeros(9 + 49, 32), (3, 7), False)
    with pytest.raises(RuntimeError, match=r"gates \(B, H, W, L \+ 1\)"):
        focalnet.context_forward_kernel(ctx0, torch.zeros(1, 2, 2, 2, dtype=bf), form, (3, 5), False)
    with pytest.raises(RuntimeError, match="weight form"):
        focalnet.context_forward_kernel(ctx0, gates, torch.zeros(33, 32), (3, 5), False)
    with pytest.raises(RuntimeError, match=r"gates \(B, H, W, L \+ 1\)"):
        focalnet.focal_context(torch.zeros(1, 2, 2, 32), torch.zeros(1, 2, 3, 3), [torch.zeros(32, 1, 3, 3)] * 2)
    with pytest.raises(RuntimeError, match=r"weights \(C, 1, K, K\)"):
        focalnet.focal_context(torch.zeros(1, 2, 2, 32), torch.zeros(1, 2, 2, 2), [torch.zeros(16, 1, 3, 3)])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        focalnet.modulate_kernel(ctx0, ctx0)
    with pytest.raises(RuntimeError, match="bfloat16"):
        focalnet.modulate_backward_kernel(ctx0.float(), ctx0.float(), ctx0.float())
    with pytest.raises(RuntimeError, match="one shape"):
        focalnet.modulate(ctx0, gates)
    blk = focalnet.FocalModulationBlock(32, focal_level=1, focal_window=3)
    blk.H, blk.W = 2, 2
    with pytest.raises(RuntimeError, match="tokens"):
        blk(torch.zeros(1, 5, 32))
    # ``fused``: off by default, not in the state dict, bf16 on the device only, no stochastic depth in training mode
    assert focalnet.FocalModulationBlock.fused is False and focalnet.FocalModulation.fused is False and focalnet.FocalNet.fused is False
    net = focalnet.FocalNet(**NET).set_fused(True)
    assert net.fused and net.patch_embed.fused and net.layers[0].downsample.fused and net.layers[1].blocks[1].fused
    assert net.layers[1].blocks[1].modulation.fused and not any("fused" in k for k in net.state_dict())
    assert list(net.state_dict().keys()) == list(focalnet.FocalNet(**NET).state_dict().keys())
    assert not net.set_fused(False).layers[2].blocks[0].modulation.fused
    drop = focalnet.FocalModulationBlock(32, drop_path=0.25, focal_level=1, focal_window=3).set_fused(True)
    drop.H, drop.W = 2, 2
    assert isinstance(drop.drop_path, focalnet.DropPath) and drop.training
    with pytest.raises(NotImplementedError, match="stochastic depth"):      # before anything touches a device
        drop(torch.zeros(1, 4, 32, dtype=bf))
    drop.eval()
    with pytest.raises(RuntimeError, match="bfloat16 tensor on the device"):
        drop(torch.zeros(1, 4, 32, dtype=bf))
    with pytest.raises(RuntimeError, match="bfloat16 tensor on the device"):
        focalnet.FocalModulation(32, focal_level=1, focal_window=3).set_fused(True)(torch.zeros(1, 2, 2, 32))


# ---- the entry points' argument checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _forward(lib, **kw):
    a = dict(ctx0=P, ld0=200, gates=P, ldg=200, w=P, B=2, H=13, W=9, C=96, L=3, window=5, normalize=0, u=P, mg=P, A=P, ws=P)
    a.update(kw)
    return lib.msda_fmod_context_forward_bf16(a["ctx0"], a["ld0"], a["gates"], a["ldg"], a["w"], a["B"], a["H"], a["W"], a["C"], a["L"], a["window"],
                                              a["normalize"], a["u"], a["mg"], a["A"], a["ws"], None)


def _backward(lib, **kw):
    a = dict(dA=P, ctx0=P, ld0=200, gates=P, ldg=200, w=P, u=P, mg=P, B=2, H=13, W=9, C=96, L=3, window=5, normalize=1, du=P, dctx0=P, ldd0=96,
             dgates=P, lddg=4, dw=P, ws=P)
    a.update(kw)
    return lib.msda_fmod_context_backward_bf16(a["dA"], a["ctx0"], a["ld0"], a["gates"], a["ldg"], a["w"], a["u"], a["mg"], a["B"], a["H"], a["W"],
                                               a["C"], a["L"], a["window"], a["normalize"], a["du"], a["dctx0"], a["ldd0"], a["dgates"], a["lddg"],
                                               a["dw"], a["ws"], None)


def _modulate(lib, **kw):
    a = dict(q=P, ldq=200, mod=P, tokens=65, C=96, out=P)
    a.update(kw)
    return lib.msda_fmod_modulate_forward_bf16(a["q"], a["ldq"], a["mod"], a["tokens"], a["C"], a["out"], None)


def _modulate_bwd(lib, **kw):
    a = dict(dout=P, q=P, ldq=200, mod=P, tokens=65, C=96, dq=P, lddq=96, dmod=P)
    a.update(kw)
    return lib.msda_fmod_modulate_backward_bf16(a["dout"], a["q"], a["ldq"], a["mod"], a["tokens"], a["C"], a["dq"], a["lddq"], a["dmod"], None)


MAP_CASES = [(dict(C=48), BAD_DIMS), (dict(C=0), BAD_DIMS), (dict(C=4128, ld0=4128), BAD_DIMS), (dict(B=0), BAD_DIMS), (dict(H=0), BAD_DIMS),
             (dict(W=-1), BAD_DIMS), (dict(B=1 << 12, H=1 << 9, W=1 << 9, C=64), TOO_LARGE),
             (dict(L=0), BAD_DIMS), (dict(L=5, window=3), BAD_DIMS), (dict(L=4, window=5), BAD_DIMS), (dict(L=2, window=9), BAD_DIMS),
             (dict(window=4, L=1), BAD_DIMS), (dict(window=1, L=1), BAD_DIMS), (dict(normalize=2), BAD_DIMS),
             (dict(ld0=95), BAD_DIMS), (dict(ld0=100), BAD_DIMS), (dict(ldg=3), BAD_DIMS)]
TOKEN_CASES = [(dict(C=40), BAD_DIMS), (dict(C=4128), BAD_DIMS), (dict(tokens=0), BAD_DIMS), (dict(tokens=1 << 20, C=2048, ldq=2048), TOO_LARGE),
               (dict(ldq=88), BAD_DIMS), (dict(ldq=100), BAD_DIMS)]


@pytest.mark.parametrize("call, entry, cases", [
    (_forward, "msda_fmod_context_forward_bf16", MAP_CASES + [
        (dict(ctx0=None), NULL_POINTER), (dict(gates=None), NULL_POINTER), (dict(w=None), NULL_POINTER), (dict(u=None), NULL_POINTER),
        (dict(mg=None), NULL_POINTER), (dict(A=None), NULL_POINTER), (dict(ws=None), NULL_POINTER), (dict(ctx0=P + 8), MISALIGNED),
        (dict(u=P + 2), MISALIGNED), (dict(A=P + 4), MISALIGNED), (dict(w=P + 2), MISALIGNED), (dict(mg=P + 1), MISALIGNED),
        (dict(gates=P + 1), MISALIGNED), (dict(ws=P + 2), MISALIGNED)]),
    (_backward, "msda_fmod_context_backward_bf16", MAP_CASES + [
        (dict(ldd0=88), BAD_DIMS), (dict(ldd0=100), BAD_DIMS), (dict(lddg=3), BAD_DIMS),
        (dict(dA=None), NULL_POINTER), (dict(ctx0=None), NULL_POINTER), (dict(gates=None), NULL_POINTER), (dict(w=None), NULL_POINTER),
        (dict(u=None), NULL_POINTER), (dict(mg=None), NULL_POINTER), (dict(du=None), NULL_POINTER), (dict(dctx0=None), NULL_POINTER),
        (dict(dgates=None), NULL_POINTER), (dict(ws=None), NULL_POINTER), (dict(dA=P + 8), MISALIGNED), (dict(du=P + 2), MISALIGNED),
        (dict(dctx0=P + 4), MISALIGNED), (dict(dgates=P + 1), MISALIGNED), (dict(dw=P + 2), MISALIGNED), (dict(ws=P + 1), MISALIGNED)]),
    (_modulate, "msda_fmod_modulate_forward_bf16", TOKEN_CASES + [
        (dict(q=None), NULL_POINTER), (dict(mod=None), NULL_POINTER), (dict(out=None), NULL_POINTER), (dict(q=P + 8), MISALIGNED),
        (dict(mod=P + 2), MISALIGNED), (dict(out=P + 4), MISALIGNED)]),
    (_modulate_bwd, "msda_fmod_modulate_backward_bf16", TOKEN_CASES + [
        (dict(lddq=88), BAD_DIMS), (dict(dout=None), NULL_POINTER), (dict(q=None), NULL_POINTER), (dict(mod=None), NULL_POINTER),
        (dict(dq=None), NULL_POINTER), (dict(dmod=None), NULL_POINTER), (dict(dout=P + 8), MISALIGNED), (dict(dq=P + 2), MISALIGNED),
        (dict(dmod=P + 4), MISALIGNED)]),
])
def test_entry_points_refuse_before_any_launch(lib, call, entry, cases):
    for kw, code in cases:
        assert call(lib, **kw) == code, kw
        assert _lib.last_error().startswith(entry + ": "), (kw, _lib.last_error())
    with pytest.raises(RuntimeError, match=entry):
        _lib.check(call(lib, C=40))


def test_workspace_bytes(lib):
    n = ctypes.c_int64(0)
    # the largest of: a row of C floats per (image, 16 x 16 tile) (the mean); per image up to 64 parts of 64 k pixels plus one row (dg, dm);
    # 81 rows per part of the weight gradient, 512 / (C / 32) parts at most
    for (B, H, W, C), floats in (((2, 13, 9, 96), 2 * 81 * 96), ((1, 1, 1, 32), 81 * 32), ((3, 17, 17, 4096), 4 * 81 * 4096),
                                 ((2, 200, 336, 192), 78 * 81 * 192)):
        assert lib.msda_fmod_workspace_bytes(B, H, W, C, ctypes.byref(n)) == 0
        assert n.value == floats * 4 == focalnet.workspace_bytes(B, H, W, C), (B, H, W, C, n.value)
    assert lib.msda_fmod_workspace_bytes(2, 13, 9, 96, None) == NULL_POINTER
    assert lib.msda_fmod_workspace_bytes(2, 13, 9, 100, ctypes.byref(n)) == BAD_DIMS
    assert _lib.last_error().startswith("msda_fmod_workspace_bytes: ")
