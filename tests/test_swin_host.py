"""No GPU: the Swin mirrors of richsem_amd/swin.py on their float64 torch path against tests/golden/layer_swin_reference.npz (written by the
reference's own classes and autograd, tests/golden/make_golden_swin.py), the state-dict contract, the refused arguments, and the host side
of the msda_swin_attn_* entry points (every argument check comes before any launch: the pointers below are fake and never dereferenced)."""
import ctypes

import pytest
import torch

import swin_attn_ref as R
from richsem_amd import _build, _lib, swin

P = 0x10000      # a 16-byte aligned fake device pointer
NULL_POINTER, BAD_DIMS, TOO_LARGE, MISALIGNED = -1, -2, -4, -5
NET = dict(embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=7, out_indices=(0, 1), mlp_ratio=2., drop_path_rate=0.)


def _close(name, got):
    want, flat = R.fixture_compare(name, got)
    torch.testing.assert_close(flat, want, rtol=1e-9, atol=1e-10 * float(want.abs().max()) + 1e-12, msg=lambda m: f"{name}: {m}")


def _layer(n, dtype=torch.float64):
    H, W, w, nH = (int(v) for v in R.fixture()[f"layer{n}.cfg"])
    layer = swin.BasicLayer(dim=32 * nH, depth=2, num_heads=nH, window_size=w, mlp_ratio=1., downsample=swin.PatchMerging).to(dtype)
    layer.load_state_dict(R.fixture_state_dict(f"layer{n}", dtype), strict=True)
    return layer, H, W


def _check_gradients(tag, module, x, outs):
    loss = sum((o * R.fixture_exact(f"{tag}.g{i}")).sum() for i, o in enumerate(outs))
    loss.backward()
    _close(f"{tag}.x_grad", x.grad)
    names = [k for k, _ in module.named_parameters()]
    assert sorted(f"{tag}.grad.{k}" for k in names) == sorted(k for k in R.fixture() if k.startswith(f"{tag}.grad.") and not k.endswith((".stride", ".sum")))
    for k, p in module.named_parameters():
        _close(f"{tag}.grad.{k}", p.grad)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_basic_layer_matches_the_reference_in_float64(n):
    layer, H, W = _layer(n)
    x = R.fixture_exact(f"layer{n}.x").requires_grad_(True)
    x_out, h, w_, x_down, h2, w2 = layer(x, H, W)
    assert (h, w_, h2, w2) == (H, W, (H + 1) // 2, (W + 1) // 2)
    _close(f"layer{n}.out0", x_out)
    _close(f"layer{n}.out1", x_down)
    _check_gradients(f"layer{n}", layer, x, (x_out, x_down))


def test_backbone_matches_the_reference_in_float64():
    net = swin.SwinTransformer(**NET).double()
    net.load_state_dict(R.fixture_state_dict("net"), strict=True)
    img = R.fixture_exact("net.x").requires_grad_(True)
    feats = net.forward_raw(img)
    assert [tuple(f.shape) for f in feats] == [(2, 32, 10, 13), (2, 64, 5, 7)]
    for i, f in enumerate(feats):
        _close(f"net.out{i}", f)
    _check_gradients("net", net, img, feats)


def test_state_dict_keys_are_the_references_both_ways():
    net = swin.SwinTransformer(**NET).double()
    stored = R.fixture_state_dict("net")
    assert list(net.state_dict().keys()) == list(stored.keys())
    assert any(k.endswith("relative_position_index") for k in stored)
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == tuple(stored[k].shape) and (v.dtype.is_floating_point or torch.equal(v, stored[k])), k


def test_forward_returns_features_with_interpolated_masks():
    net = swin.SwinTransformer(**NET).double()
    net.load_state_dict(R.fixture_state_dict("net"), strict=True)
    img = R.fixture_exact("net.x")
    mask = torch.zeros(2, 40, 52, dtype=torch.bool)
    mask[1, :, 30:] = True
    levels = net(img, mask)
    raw = net.forward_raw(img)
    for (feat, m), want in zip(levels, raw):
        assert torch.equal(feat, want) and m.dtype == torch.bool and m.shape == (2,) + feat.shape[-2:]
        assert torch.equal(m, torch.nn.functional.interpolate(mask[None].float(), size=feat.shape[-2:]).to(torch.bool)[0])


def test_frozen_stages_and_out_indices():
    net = swin.SwinTransformer(**{**NET, "frozen_stages": 2, "out_indices": (1,)})
    assert not any(p.requires_grad for p in net.patch_embed.parameters()) and not any(p.requires_grad for p in net.layers[0].parameters())
    assert all(p.requires_grad for p in net.layers[1].parameters())
    net.train()
    assert not net.layers[0].training and not net.patch_embed.training and net.layers[1].training
    assert hasattr(net, "norm1") and not hasattr(net, "norm0")
    assert len(net.forward_raw(torch.zeros(1, 3, 32, 32))) == 1


def test_drop_path_is_per_sample_and_off_in_eval():
    dp = swin.DropPath(0.5)
    x = torch.ones(64, 3, 5)
    dp.eval()
    assert torch.equal(dp(x), x)
    dp.train()
    torch.manual_seed(0)
    y = dp(x)
    per_sample = y.reshape(64, -1)
    assert bool(((per_sample == 0).all(1) | (per_sample == 2).all(1)).all()) and 0 < int((per_sample[:, 0] == 0).sum()) < 64
    blk = swin.SwinTransformerBlock(32, 1, window_size=4, drop_path=0.25)
    assert isinstance(blk.drop_path, swin.DropPath) and blk.drop_path.drop_prob == 0.25


@pytest.mark.parametrize("make, name", [
    (lambda: swin.WindowAttention(32, (7, 7), 1, attn_drop=0.1), "attn_drop"),
    (lambda: swin.WindowAttention(32, (7, 7), 1, proj_drop=0.1), "drop"),
    (lambda: swin.SwinTransformerBlock(32, 1, drop=0.1), "drop"),
    (lambda: swin.SwinTransformerBlock(32, 1, attn_drop=0.1), "attn_drop"),
    (lambda: swin.BasicLayer(32, 2, 1, use_checkpoint=True), "use_checkpoint"),
    (lambda: swin.SwinTransformer(**{**NET, "use_checkpoint": True}), "use_checkpoint"),
    (lambda: swin.SwinTransformer(**{**NET, "drop_rate": 0.1}), "drop"),
    (lambda: swin.SwinTransformer(**{**NET, "attn_drop_rate": 0.1}), "attn_drop"),
])
def test_unsupported_arguments_raise(make, name):
    with pytest.raises(NotImplementedError, match=name):
        make()


def test_window_attention_refuses_cpu_tensors_and_is_exported():
    import richsem_amd
    assert richsem_amd.window_attention is swin.window_attention and richsem_amd.SwinTransformer is swin.SwinTransformer
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        swin.window_attention(torch.zeros(1, 4, 4, 96, dtype=torch.bfloat16), torch.zeros(49, 1), 1, 4, 0)


def test_torch_composition_equals_the_float64_restatement():
    """the package's pixel-index composition and the roll / partition restatement of tests/swin_attn_ref.py, two routes to one formula"""
    gen = torch.Generator().manual_seed(5)
    for (B, Hp, Wp, nH, w, s) in ((2, 14, 21, 2, 7, 3), (1, 12, 24, 3, 12, 11), (2, 4, 12, 1, 4, 1), (1, 7, 7, 1, 7, 0)):
        qkv, table, dout = R.random_inputs(B, Hp, Wp, nH, w, gen)
        q64 = qkv.double().requires_grad_(True)
        t64 = table.double().requires_grad_(True)
        out = swin.window_attention_torch(q64, t64, nH, w, s)
        (out * dout.double()).sum().backward()
        val, _ = R.reference(qkv, table, dout, nH, w, s)
        for name, got in (("out", out), ("dqkv", q64.grad), ("dtable", t64.grad)):
            torch.testing.assert_close(got.detach(), val[name], rtol=1e-10, atol=1e-11, msg=lambda m: f"{name} {(B, Hp, Wp, nH, w, s)}: {m}")


# ---- the entry points' argument checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _fwd(lib, **kw):
    a = dict(qkv=P, table=P, B=1, Hp=14, Wp=21, C=64, nH=2, w=7, s=3, out=P, lse=P)
    a.update(kw)
    return lib.msda_swin_attn_forward_bf16(a["qkv"], a["table"], a["B"], a["Hp"], a["Wp"], a["C"], a["nH"], a["w"], a["s"], a["out"], a["lse"], None)


def _bwd(lib, **kw):
    a = dict(qkv=P, table=P, out=P, lse=P, dout=P, B=1, Hp=14, Wp=21, C=64, nH=2, w=7, s=3, dqkv=P, dtable=P, ws=P)
    a.update(kw)
    return lib.msda_swin_attn_backward_bf16(a["qkv"], a["table"], a["out"], a["lse"], a["dout"], a["B"], a["Hp"], a["Wp"], a["C"], a["nH"], a["w"],
                                            a["s"], a["dqkv"], a["dtable"], a["ws"], None)


@pytest.mark.parametrize("call, entry", [(_fwd, "msda_swin_attn_forward_bf16"), (_bwd, "msda_swin_attn_backward_bf16")])
def test_entry_points_refuse_before_any_launch(lib, call, entry):
    for kw, code in ((dict(w=13, Hp=13, Wp=13, s=0), BAD_DIMS),       # w w > 144
                     (dict(Hp=15), BAD_DIMS), (dict(Wp=20), BAD_DIMS),      # map not a multiple of the window
                     (dict(C=48), BAD_DIMS), (dict(C=96), BAD_DIMS),        # channels != 32 heads
                     (dict(s=7), BAD_DIMS), (dict(s=-1), BAD_DIMS), (dict(B=0), BAD_DIMS), (dict(nH=0, C=0), BAD_DIMS),
                     (dict(B=1 << 20, Hp=7 * 64, Wp=7 * 64), TOO_LARGE),
                     (dict(qkv=None), NULL_POINTER), (dict(table=None), NULL_POINTER), (dict(lse=None), NULL_POINTER),
                     (dict(qkv=P + 8), MISALIGNED), (dict(out=P + 2), MISALIGNED), (dict(table=P + 2), MISALIGNED)):
        assert call(lib, **kw) == code, kw
        assert _lib.last_error().startswith(entry + ": "), (kw, _lib.last_error())
    with pytest.raises(RuntimeError, match=entry):
        _lib.check(call(lib, C=48))


def test_workspace_bytes(lib):
    n = ctypes.c_int64(0)
    assert lib.msda_swin_attn_workspace_bytes(2, 14, 21, 64, 2, 7, ctypes.byref(n)) == 0
    assert n.value == 2 * 6 * 2 * 169 * 4 == swin.workspace_bytes(2, 14, 21, 64, 2, 7)
    assert lib.msda_swin_attn_workspace_bytes(2, 14, 21, 64, 2, 7, None) == NULL_POINTER
    assert lib.msda_swin_attn_workspace_bytes(2, 14, 22, 64, 2, 7, ctypes.byref(n)) == BAD_DIMS
    assert _lib.last_error().startswith("msda_swin_attn_workspace_bytes: ")
