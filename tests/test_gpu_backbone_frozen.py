"""GPU (-m gpu): the fused backbone paths with ONE tensor frozen at a time.

Every autograd function of richsem_amd/backbone_ops.py, swin.py, convnext.py and focalnet.py reads ``ctx.needs_input_grad`` at positions its
author counted by hand, to skip the work a frozen parameter does not need.  A wrong position returns a gradient to the wrong tensor, or
skips one that was wanted.  So, per module: one run with everything trainable and one fixed cotangent; then, for each named parameter alone
and for the input alone, ``requires_grad=False`` and the same run again on the same tensors.  The frozen tensor's ``.grad`` is None; the
output and EVERY other gradient have the bits of the first run (compared as integers, so that a NaN does not equal itself away).

Bit equality is a property here because the kernels have no atomics (tests/test_gpu_swin_block.py asserts it call against call) and because
every shape is below ``LinearBf16Function.MIN_TOKENS``: every weight gradient is the transposed GEMM and every bias gradient the column
sum, whichever subset is frozen.  (Above it, freezing a weight moves its bias's gradient to another kernel: not claimed.)  The shapes are
the smallest at which the plumbing can go wrong: 65 tokens make two 64-token partial rows of the ``dgamma`` sums and a ragged last tile; the
5 x 13 map pads the window grid and leaves a partial 16 x 16 convolution tile; the 18 x 22 image pads the patch grid and its Kp = 64 > 48
exercises the dropped padding columns of the weight gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H, W = 5, 13


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _prepare(module, seed):
    """seeded noise on every parameter (norm weights of exactly 1 and layer scales of 1e-4 would hide a swapped pair), then bf16 on the device"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=gen))
    return module.to(BF).cuda()


def _tokens(seed):
    return torch.randn(1, H * W, 32, generator=torch.Generator().manual_seed(seed)).to(BF).cuda()


def _swin_block():
    from richsem_amd import swin
    blk = _prepare(swin.SwinTransformerBlock(32, 1, window_size=4, shift_size=2, mlp_ratio=2.), 1)
    blk.fused, blk.H, blk.W = True, H, W
    return blk, blk, _tokens(1), None


def _swin_merging():
    from richsem_amd import swin
    merge = _prepare(swin.PatchMerging(32), 2)
    merge.fused = True
    return merge, lambda x: merge(x, H, W), _tokens(2), None


def _swin_embed():
    from richsem_amd import swin
    embed = _prepare(swin.PatchEmbed(4, 3, 32, torch.nn.LayerNorm), 3)
    embed.fused = True
    return embed, embed, torch.randn(1, 3, 18, 22, generator=torch.Generator().manual_seed(3)).to(BF).cuda(), None


def _convnext_block():
    from richsem_amd import convnext
    blk = _prepare(convnext.Block(32), 4).set_fused(True)
    return blk, blk, torch.randn(1, 32, H, W, generator=torch.Generator().manual_seed(4)).to(BF).cuda(), None


def _convnext_net():
    from richsem_amd import convnext
    net = _prepare(convnext.ConvNeXt(depths=(1, 1, 1, 1), dims=(32, 64, 96, 128)), 5).set_fused(True)
    img = torch.randn(1, 3, 32, 48, generator=torch.Generator().manual_seed(5)).to(BF).cuda()
    return net, net.forward_features, img, lambda k: k.startswith(("downsample_layers.", "norm"))


def _focal_block(flag):
    from richsem_amd import focalnet
    blk = _prepare(focalnet.FocalModulationBlock(32, mlp_ratio=2., focal_level=2, focal_window=3, use_postln=flag,
                                                 use_postln_in_modulation=flag, use_layerscale=flag), 6 + flag).set_fused(True)
    blk.H, blk.W = H, W
    return blk, blk, _tokens(6 + flag), None


CASES = {"swin block": _swin_block, "swin merging": _swin_merging, "swin embed": _swin_embed, "convnext block": _convnext_block,
         "convnext net": _convnext_net, "focalnet block post-LN": lambda: _focal_block(True), "focalnet block pre-LN": lambda: _focal_block(False)}


def _run(module, call, x, cots):
    """-> (outputs, gradients by name, the cotangents): one eager forward and backward"""
    module.zero_grad(set_to_none=True)
    x.grad = None
    out = call(x)
    outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
    if cots is None:
        gen = torch.Generator().manual_seed(7)
        cots = [torch.randn(o.shape, generator=gen).to(BF).cuda() for o in outs]
    torch.autograd.backward(outs, cots)
    grads = {k: p.grad for k, p in module.named_parameters()}
    grads["input"] = x.grad
    return [o.detach() for o in outs], grads, cots


@pytest.mark.parametrize("name", list(CASES))
def test_freezing_one_tensor_changes_no_other_bit(name):
    module, call, x, swept = CASES[name]()
    leaves = dict(module.named_parameters())
    leaves["input"] = x
    for t in leaves.values():
        t.requires_grad_(True)
    outs, grads, cots = _run(module, call, x, None)
    assert all(g is not None and bool(torch.isfinite(g.float()).all()) for g in grads.values()), [k for k, g in grads.items() if g is None]
    assert all(grads[k].dtype == BF and grads[k].shape == t.shape for k, t in leaves.items())
    for frozen in [k for k in leaves if k == "input" or swept is None or swept(k)]:
        leaves[frozen].requires_grad_(False)
        outs2, grads2, _ = _run(module, call, x, cots)
        leaves[frozen].requires_grad_(True)
        assert grads2[frozen] is None, frozen
        assert all(_same(a, b) for a, b in zip(outs, outs2)), f"the output with {frozen} frozen"
        wrong = [k for k in grads if k != frozen and not _same(grads[k], grads2[k])]
        assert not wrong, f"with {frozen} frozen, the gradients of {wrong} differ from the run with everything trainable"
