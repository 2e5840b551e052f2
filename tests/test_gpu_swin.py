"""GPU (-m gpu): the Swin mirrors of richsem_amd/swin.py on their DEVICE path -- bf16, the window-attention kernels -- against the float64
fixture of the reference's own classes (tests/golden/layer_swin_reference.npz): the three BasicLayers (two blocks + PatchMerging, maps that
need padding, w = 7 and 12) and the toy SwinTransformer, outputs and every gradient.

The tolerance is not a number fixed in advance.  Each test also runs a plain torch bf16 composition of the same layer, written below
from the formulas (LayerNorm, pad, qkv, roll, window partition, bias gather, -100 region mask, softmax, reverse, roll back, proj, crop,
residual, MLP; PatchMerging; patch embedding) on the fixture's state dict -- not the package's code -- and requires, per tensor,

    err(kernel path, fixture) <= 2 * err(composition, fixture)

Two correct bf16 implementations differ by rounding order; the factor 2 is that margin.  err is the root mean square of the difference
over the tensor's stored elements (the whole tensor, or the fixture's every stride-th element): a mean over hundreds of elements is a
stable figure for two implementations that round differently, which a maximum is not.  RICHSEM_REPORT=1 prints both errors per tensor
(recorded in profiles/r31_swin_attention.md)."""
import os

import pytest
import torch
import torch.nn.functional as F

import swin_attn_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))
NET = dict(embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=7, out_indices=(0, 1), mlp_ratio=2., drop_path_rate=0.)


# ---- the composition ---------------------------------------------------------------------------------------------------------------------
def comp_attention(qkv, table, nH, w, s):
    B, Hp, Wp, C3 = qkv.shape
    C, N, nW = C3 // 3, w * w, (Hp // w) * (Wp // w)
    x = torch.roll(qkv, shifts=(-s, -s), dims=(1, 2)) if s else qkv
    win = x.view(B, Hp // w, w, Wp // w, w, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
    attn = (win[0] * 32 ** -0.5) @ win[1].transpose(-2, -1)
    attn = attn + table[R.bias_pairs(w).reshape(-1).to(table.device)].view(N, N, nH).permute(2, 0, 1).contiguous().unsqueeze(0)
    if s:
        reg = R.regions(Hp, Wp, w, s).to(qkv.device)
        mask = ((reg[:, :, None] != reg[:, None, :]).to(attn.dtype) * -100.0)
        attn = (attn.view(B, nW, nH, N, N) + mask[None, :, None]).view(-1, nH, N, N)
    o = (attn.softmax(-1) @ win[2]).transpose(1, 2).reshape(B, Hp // w, Wp // w, w, w, C)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    return torch.roll(o, shifts=(s, s), dims=(1, 2)) if s else o


def comp_block(P, pre, x, H, W, w, s, nH):
    B, L, C = x.shape
    h = F.layer_norm(x, (C,), P[pre + "norm1.weight"], P[pre + "norm1.bias"]).view(B, H, W, C)
    h = F.pad(h, (0, 0, 0, (w - W % w) % w, 0, (w - H % w) % w))
    qkv = F.linear(h, P[pre + "attn.qkv.weight"], P[pre + "attn.qkv.bias"])
    a = comp_attention(qkv, P[pre + "attn.relative_position_bias_table"], nH, w, s)
    a = F.linear(a, P[pre + "attn.proj.weight"], P[pre + "attn.proj.bias"])[:, :H, :W].reshape(B, L, C)
    x = x + a
    h = F.layer_norm(x, (C,), P[pre + "norm2.weight"], P[pre + "norm2.bias"])
    return x + F.linear(F.gelu(F.linear(h, P[pre + "mlp.fc1.weight"], P[pre + "mlp.fc1.bias"])), P[pre + "mlp.fc2.weight"], P[pre + "mlp.fc2.bias"])


def comp_merge(P, pre, x, H, W):
    B, L, C = x.shape
    x = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(B, -1, 4 * C)
    return F.linear(F.layer_norm(x, (4 * C,), P[pre + "norm.weight"], P[pre + "norm.bias"]), P[pre + "reduction.weight"])


def comp_layer(P, pre, x, H, W, w, nH, down):
    for i in range(2):
        x = comp_block(P, f"{pre}blocks.{i}.", x, H, W, w, (w // 2) * (i % 2), nH)
    return x, (comp_merge(P, pre + "downsample.", x, H, W) if down else x)


def comp_net(P, img):
    x = F.conv2d(img, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=4)
    B, C, H, W = x.shape
    x = F.layer_norm(x.flatten(2).transpose(1, 2), (C,), P["patch_embed.norm.weight"], P["patch_embed.norm.bias"])
    o0, x = comp_layer(P, "layers.0.", x, H, W, 7, 1, True)
    f0 = F.layer_norm(o0, (C,), P["norm0.weight"], P["norm0.bias"]).view(B, H, W, C).permute(0, 3, 1, 2)
    H, W = (H + 1) // 2, (W + 1) // 2
    o1, _ = comp_layer(P, "layers.1.", x, H, W, 7, 2, False)
    f1 = F.layer_norm(o1, (2 * C,), P["norm1.weight"], P["norm1.bias"]).view(B, H, W, 2 * C).permute(0, 3, 1, 2)
    return f0, f1


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------
def _err(name, got):
    want, flat = R.fixture_compare(name, got)
    if name + ".stride" in R.fixture():      # (the sum of all elements is a float64 check: not part of a bf16 error)
        want, flat = want[:-1], flat[:-1]
    assert bool(torch.isfinite(flat).all()), name
    return float((flat - want).pow(2).mean().sqrt()), float(want.pow(2).mean().sqrt())


def _compare(tag, kernel, comp):
    """kernel, comp: dicts fixture name -> tensor"""
    assert sorted(kernel) == sorted(comp)
    lines, bad = [], []
    for name in sorted(kernel):
        (ek, scale), (ec, _) = _err(name, kernel[name]), _err(name, comp[name])
        lines.append(f"[measured] {name} rms={scale:.3g} kernel_err={ek:.3g} composition_err={ec:.3g} ratio={ek / max(ec, 1e-300):.2f}")
        if not ek <= 2 * ec:
            bad.append(lines[-1])
    if REPORT:
        print("\n".join(lines), flush=True)
    assert not bad, "\n".join(bad)


def _backward(tag, outs):
    sum((o.float() * R.fixture_exact(f"{tag}.g{i}", torch.float32).cuda()).sum() for i, o in enumerate(outs)).backward()


def _results(tag, outs, x, grads):
    res = {f"{tag}.out{i}": o for i, o in enumerate(outs)}
    res[f"{tag}.x_grad"] = x.grad
    res.update({f"{tag}.grad.{k}": g for k, g in grads.items()})
    return res


@pytest.mark.parametrize("n", [0, 1, 2])
def test_basic_layer_device_path_against_the_fixture(n):
    from richsem_amd import swin
    tag = f"layer{n}"
    H, W, w, nH = (int(v) for v in R.fixture()[f"{tag}.cfg"])
    sd = R.fixture_state_dict(tag, BF)
    layer = swin.BasicLayer(dim=32 * nH, depth=2, num_heads=nH, window_size=w, mlp_ratio=1., downsample=swin.PatchMerging).to(BF)
    layer.load_state_dict(sd, strict=True)
    layer.cuda()
    x = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    x_out, _, _, x_down, _, _ = layer(x, H, W)
    _backward(tag, (x_out, x_down))
    kernel = _results(tag, (x_out, x_down), x, {k: p.grad for k, p in layer.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point}
    xc = R.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    outs = comp_layer(P, "", xc, H, W, w, nH, True)
    _backward(tag, outs)
    _compare(tag, kernel, _results(tag, outs, xc, {k: p.grad for k, p in P.items()}))


def test_toy_backbone_device_path_against_the_fixture():
    from richsem_amd import swin
    sd = R.fixture_state_dict("net", BF)
    net = swin.SwinTransformer(**NET).to(BF)
    net.load_state_dict(sd, strict=True)
    net.cuda()
    img = R.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    feats = net.forward_raw(img)
    assert [tuple(f.shape) for f in feats] == [(2, 32, 10, 13), (2, 64, 5, 7)]
    _backward("net", feats)
    kernel = _results("net", feats, img, {k: p.grad for k, p in net.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point}
    imgc = R.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    outs = comp_net(P, imgc)
    _backward("net", outs)
    _compare("net", kernel, _results("net", outs, imgc, {k: p.grad for k, p in P.items()}))
