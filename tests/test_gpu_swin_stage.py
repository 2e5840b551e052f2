"""GPU (-m gpu): the kernels of csrc/swin_stage.hip -- merging norm, output norm to NCHW, patch rows -- against the element-wise bounds of
tests/swin_stage_ref.py (swin_block_ref's LayerNorm bounds on the gathered matrix), exact probes checked bit for bit, NaN-poisoned result
buffers with guard rows, reproducibility, what the autograd functions save, and the float64 fixture of the reference's classes with the
stage switch set under the rule of tests/test_gpu_swin.py (err(kernel path) <= 2 err(torch bf16 composition)).

The shapes are those of tests/swin_stage_ref.py, on which tests/test_swin_stage_ref.py shows every wrong variant leaving the bounds.
Merging norm: one pixel (three padded quadrants), odd H and W, even both, 72 rows (two partial rows of the dgamma sum), the widest row
(4 C = 4096).  NCHW norm: one token, the fixture's odd 35 and even 130 tokens per image over two images (channel rows on 2-byte
boundaries, a 64-token part that spans two images), C = 1536 (16-token tiles, 67 = 4 tiles + 3) and C = 4096 (4-token tiles, 200 tokens:
four 64-token parts).  Capture into a HIP graph is NOT tested here ("Class head")."""
import os

import pytest
import torch
import torch.nn.functional as F

import swin_attn_ref as A
import swin_stage_ref as S
from test_gpu_swin import NET, _backward, _compare, _results, comp_layer, comp_net
from test_gpu_swin_block import Poisoned

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))
EPS = 1e-5


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(*ts):
    return [t.cuda().contiguous() if t is not None else None for t in ts]


def _inside(tag, got, val, bound):
    res = S.ratios(got, val, bound)
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()), flush=True)
    assert res and all(r <= 1.0 for r in res.values()), (tag, res)


def _ptr(p):
    return p.ptr() if p is not None else None


def _workspace(tokens, C):
    from richsem_amd import swin
    return torch.full((swin.layernorm_workspace_bytes(tokens, C) // 4,), float("nan"), device="cuda")


# ---- raw calls into poisoned buffers ---------------------------------------------------------------------------------------------------
def call_merge_norm(x, gamma, beta, eps=EPS, stats=True):
    from richsem_amd import _lib
    B, H, W, C = x.shape
    rows = B * ((H + 1) // 2) * ((W + 1) // 2)
    out, mean, rstd = Poisoned(rows, 4 * C, BF), Poisoned(rows, 1, torch.float32), Poisoned(rows, 1, torch.float32)
    _lib.check(_lib.load().msda_swin_merge_norm_forward_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, B, H, W, C, out.ptr(),
                                                             mean.ptr() if stats else None, rstd.ptr() if stats else None, _lib.raw_stream(x.device)))
    res = {"out": out.result("merge norm out")}
    if stats:
        res.update(mean=mean.result("mean")[:, 0], rstd=rstd.result("rstd")[:, 0])
    return res


def call_merge_norm_backward(dy, x, mean, rstd, gamma, want_gamma=True, want_beta=True):
    from richsem_amd import _lib
    B, H, W, C = x.shape
    dx = Poisoned(B * H * W, C, BF)
    dg, db = (Poisoned(4 * C, 1, torch.float32) if want_gamma else None), (Poisoned(4 * C, 1, torch.float32) if want_beta else None)
    ws = _workspace(dy.shape[0], 4 * C) if want_gamma or want_beta else None
    _lib.check(_lib.load().msda_swin_merge_norm_backward_bf16(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                              B, H, W, C, dx.ptr(), _ptr(dg), _ptr(db), ws.data_ptr() if ws is not None else None,
                                                              _lib.raw_stream(x.device)))
    res = {"dx": dx.result("merge norm dx").view(B, H, W, C)}      # (every pixel of the map written, nothing outside it)
    if want_gamma:
        res["dgamma"] = dg.result("dgamma")[:, 0]
    if want_beta:
        res["dbeta"] = db.result("dbeta")[:, 0]
    return res


def call_norm_nchw(x, gamma, beta, eps=EPS, stats=True):
    from richsem_amd import _lib
    B, HW, C = x.shape
    # (one row of B C HW elements between the guards: C is a multiple of 32, so the result starts on a 16-byte boundary whatever HW is)
    out, mean, rstd = Poisoned(1, B * C * HW, BF), Poisoned(B * HW, 1, torch.float32), Poisoned(B * HW, 1, torch.float32)
    _lib.check(_lib.load().msda_swin_norm_nchw_forward_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, B, HW, C, out.ptr(),
                                                            mean.ptr() if stats else None, rstd.ptr() if stats else None, _lib.raw_stream(x.device)))
    res = {"out": out.result("norm nchw out").view(B, C, HW)}
    if stats:
        res.update(mean=mean.result("mean")[:, 0], rstd=rstd.result("rstd")[:, 0])
    return res


def call_norm_nchw_backward(dy, x, mean, rstd, gamma, want_gamma=True, want_beta=True):
    from richsem_amd import _lib
    B, HW, C = x.shape
    dx = Poisoned(B * HW, C, BF)
    dg, db = (Poisoned(C, 1, torch.float32) if want_gamma else None), (Poisoned(C, 1, torch.float32) if want_beta else None)
    ws = _workspace(B * HW, C) if want_gamma or want_beta else None
    _lib.check(_lib.load().msda_swin_norm_nchw_backward_bf16(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                             B, HW, C, dx.ptr(), _ptr(dg), _ptr(db), ws.data_ptr() if ws is not None else None,
                                                             _lib.raw_stream(x.device)))
    res = {"dx": dx.result("norm nchw dx").view(B, HW, C)}
    if want_gamma:
        res["dgamma"] = dg.result("dgamma")[:, 0]
    if want_beta:
        res["dbeta"] = db.result("dbeta")[:, 0]
    return res


def call_patch_rows(img, ph, pw):
    from richsem_amd import _lib, swin
    B, Cin, H, W = img.shape
    Wh, Ww = swin.patch_grid(H, W, (ph, pw))
    rows = Poisoned(B * Wh * Ww, swin.patch_width(Cin, (ph, pw)), BF)
    _lib.check(_lib.load().msda_swin_patch_rows_bf16(img.data_ptr(), B, Cin, H, W, ph, pw, rows.ptr(), _lib.raw_stream(img.device)))
    return rows.result("patch rows")


def call_patch_rows_backward(drows, shape, ph, pw):
    from richsem_amd import _lib
    B, Cin, H, W = shape
    dimg = Poisoned(B * Cin * H, W, BF)
    _lib.check(_lib.load().msda_swin_patch_rows_backward_bf16(drows.data_ptr(), B, Cin, H, W, ph, pw, dimg.ptr(), _lib.raw_stream(drows.device)))
    return dimg.result("patch rows backward").view(B, Cin, H, W)


def _partial_calls_are_bit_equal(call, full):
    for wg, wb in ((False, False), (True, False), (False, True)):
        part = call(want_gamma=wg, want_beta=wb)
        assert sorted(part) == sorted(["dx"] + ["dgamma"] * wg + ["dbeta"] * wb)
        for k, v in part.items():
            assert _same(v, full[k]), k


# ---- merging norm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, H, W, C", S.MERGE_SHAPES)
def test_merge_norm_forward_and_backward_are_inside_the_bounds(B, H, W, C):
    x, dy, gamma, beta = S.merge_inputs(B, H, W, C, torch.Generator().manual_seed(B + H + W + C))
    xd, dyd, gd, bd = _dev(x, dy, gamma, beta)
    val, bound = S.merge_norm_reference(x, gamma, beta, EPS)
    got = call_merge_norm(xd, gd, bd)
    _inside(f"merge norm {(B, H, W, C)}", got, val, bound)
    alone = call_merge_norm(xd, gd, bd, stats=False)
    assert sorted(alone) == ["out"] and _same(alone["out"], got["out"])
    again = call_merge_norm(xd, gd, bd)
    assert all(_same(again[k], got[k]) for k in got)
    mean, rstd = got["mean"].contiguous(), got["rstd"].contiguous()
    val, bound = S.merge_norm_backward_reference(dy, x, gamma, EPS)
    full = call_merge_norm_backward(dyd, xd, mean, rstd, gd)
    assert sorted(full) == ["dbeta", "dgamma", "dx"]
    _inside(f"merge norm backward {(B, H, W, C)}", full, val, bound)
    _partial_calls_are_bit_equal(lambda **kw: call_merge_norm_backward(dyd, xd, mean, rstd, gd, **kw), full)
    again = call_merge_norm_backward(dyd, xd, mean, rstd, gd)
    assert all(_same(again[k], full[k]) for k in full)


@pytest.mark.parametrize("B, H, W, C", [(2, 4, 6, 32), (1, 2, 2, 1024)])
def test_merge_norm_sign_probe_lands_every_pixel_bit_for_bit(B, H, W, C):
    """eps = 0, even H and W, x = s(pixel) (-1)^c: mean 0 and variance 1 exactly, out[row, q C + c] = rnd(s(pixel of quadrant q) (-1)^c gamma + beta)"""
    gen = torch.Generator().manual_seed(H * W + C)
    x = S.sign_probe((B, H, W, C), gen)
    gamma, beta = 1 + 0.5 * torch.randn(4 * C, generator=gen), 0.5 * torch.randn(4 * C, generator=gen)
    got = call_merge_norm(*_dev(x, gamma, beta), eps=0.0)
    want = (S.gather(x.float(), S.merge_index(B, H, W, C)) * gamma + beta).to(BF)
    assert _same(got["out"].cpu(), want)
    assert not bool(got["mean"].any()) and bool((got["rstd"] == 1).all())


def test_merge_norm_zero_gradient_gives_exact_zeros_over_the_whole_map():
    B, H, W, C = 2, 13, 9, 32
    x, dy, gamma, beta = S.merge_inputs(B, H, W, C, torch.Generator().manual_seed(5))
    xd, gd, bd = _dev(x, gamma, beta)
    st = call_merge_norm(xd, gd, bd)
    got = call_merge_norm_backward(torch.zeros_like(dy).cuda(), xd, st["mean"].contiguous(), st["rstd"].contiguous(), gd)
    assert got["dx"].shape == (B, H, W, C) and not bool(got["dx"].any()) and not bool(got["dgamma"].any()) and not bool(got["dbeta"].any())


# ---- output norm to NCHW ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, HW, C", S.NCHW_SHAPES)
def test_norm_nchw_forward_and_backward_are_inside_the_bounds(B, HW, C):
    x, dy, gamma, beta = S.nchw_inputs(B, HW, C, torch.Generator().manual_seed(B + HW + C))
    xd, dyd, gd, bd = _dev(x, dy, gamma, beta)
    val, bound = S.norm_nchw_reference(x, gamma, beta, EPS)
    got = call_norm_nchw(xd, gd, bd)
    _inside(f"norm nchw {(B, HW, C)}", got, val, bound)
    alone = call_norm_nchw(xd, gd, bd, stats=False)
    assert sorted(alone) == ["out"] and _same(alone["out"], got["out"])
    again = call_norm_nchw(xd, gd, bd)
    assert all(_same(again[k], got[k]) for k in got)
    mean, rstd = got["mean"].contiguous(), got["rstd"].contiguous()
    val, bound = S.norm_nchw_backward_reference(dy, x, gamma, EPS)
    full = call_norm_nchw_backward(dyd, xd, mean, rstd, gd)
    assert sorted(full) == ["dbeta", "dgamma", "dx"]
    _inside(f"norm nchw backward {(B, HW, C)}", full, val, bound)
    _partial_calls_are_bit_equal(lambda **kw: call_norm_nchw_backward(dyd, xd, mean, rstd, gd, **kw), full)
    again = call_norm_nchw_backward(dyd, xd, mean, rstd, gd)
    assert all(_same(again[k], full[k]) for k in full)


@pytest.mark.parametrize("B, HW, C", [(2, 35, 64), (1, 67, 1536)])
def test_norm_nchw_sign_probe_lands_every_token_bit_for_bit(B, HW, C):
    gen = torch.Generator().manual_seed(HW + C)
    x = S.sign_probe((B, HW, C), gen)
    gamma, beta = 1 + 0.5 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)
    got = call_norm_nchw(*_dev(x, gamma, beta), eps=0.0)
    assert _same(got["out"].cpu(), (x.float() * gamma + beta).to(BF).transpose(1, 2).contiguous())
    assert not bool(got["mean"].any()) and bool((got["rstd"] == 1).all())


def test_norm_nchw_constant_rows_return_beta_down_every_channel_row():
    gen = torch.Generator().manual_seed(3)
    for B, HW, C in ((2, 35, 96), (1, 67, 1536)):
        x = (torch.randn(B, HW, 1, generator=gen) * 3).to(BF).expand(B, HW, C).contiguous()
        gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        got = call_norm_nchw(*_dev(x, gamma, beta))
        assert _same(got["out"].cpu(), beta.to(BF)[None, :, None].expand(B, C, HW).contiguous())
        assert torch.equal(got["mean"].cpu(), x[..., 0].reshape(-1).float())


# ---- patch rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, patch", S.PATCH_SHAPES)
def test_patch_rows_are_the_unfold_of_the_padded_image_bit_for_bit(shape, patch):
    ph, pw = patch
    gen = torch.Generator().manual_seed(sum(shape))
    img = torch.randn(*shape, generator=gen).to(BF)
    want = S.patch_rows_reference(img, ph, pw)
    got = call_patch_rows(img.cuda(), ph, pw)
    assert _same(got.cpu(), want)
    K = shape[1] * ph * pw
    assert not bool(got[:, K:].view(torch.int16).any())      # (exact zeros: not even a negative zero)
    assert _same(call_patch_rows(img.cuda(), ph, pw), got)
    drows = torch.randn(want.shape, generator=gen).to(BF)
    back = call_patch_rows_backward(drows.cuda(), shape, ph, pw)
    assert _same(back.cpu(), S.patch_rows_backward_reference(drows, shape, ph, pw))


# ---- the autograd functions ------------------------------------------------------------------------------------------------------------
def _saved(fn):
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        out = fn()
    return out, saved


def test_functions_save_the_input_and_statistics_and_nothing_under_no_grad():
    from richsem_amd import swin
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 15, 32, generator=gen).to(BF).cuda().requires_grad_(True)
    n4, n1 = torch.nn.LayerNorm(128).cuda(), torch.nn.LayerNorm(32).cuda().to(BF)
    img = torch.randn(1, 3, 13, 18, generator=gen).to(BF).cuda().requires_grad_(True)
    calls = {"merge": lambda: swin.swin_merge_norm(x, 3, 5, n4.weight, n4.bias, 1e-5), "nchw": lambda: swin.swin_norm_nchw(x, 3, 5, n1.weight, n1.bias, 1e-5),
             "rows": lambda: swin.swin_patch_rows(img, 4)}
    shapes = {"merge": (2, 6, 128), "nchw": (2, 32, 3, 5), "rows": (1, 20, 64)}
    want_saved = {"merge": [(2, 15, 32), (12,), (12,), (128,)], "nchw": [(2, 15, 32), (30,), (30,), (32,)], "rows": []}
    for name, call in calls.items():
        out, saved = _saved(call)
        assert tuple(out.shape) == shapes[name] and out.dtype == BF and out.is_contiguous() and out.grad_fn is not None
        assert sorted(saved) == sorted(want_saved[name]), (name, saved)
        with torch.no_grad():
            quiet, saved = _saved(call)
        assert saved == [] and quiet.grad_fn is None and _same(quiet, out.detach())
        out.backward(torch.randn(out.shape, generator=gen).to(BF).cuda())
    # gradients in the parameters' dtypes: fp32 masters for the merging norm, bf16 parameters for the output norm
    assert n4.weight.grad.dtype == n4.bias.grad.dtype == torch.float32 and n1.weight.grad.dtype == n1.bias.grad.dtype == BF
    assert x.grad.dtype == BF and x.grad.shape == x.shape and img.grad.dtype == BF and img.grad.shape == img.shape
    frozen = torch.randn(2, 15, 32, generator=gen).to(BF).cuda()
    n4.weight.requires_grad_(False)
    n4.zero_grad(set_to_none=True)
    swin.swin_merge_norm(frozen, 3, 5, n4.weight, n4.bias, 1e-5).float().sum().backward()
    assert n4.weight.grad is None and n4.bias.grad is not None


def test_fused_stages_raise_outside_the_limits_instead_of_falling_back():
    from richsem_amd import swin
    merge = swin.PatchMerging(48).to(BF).cuda()      # C = 48: not a multiple of 32
    merge.fused = True
    with pytest.raises(RuntimeError, match="msda_swin_merge_norm_forward_bf16"):
        merge(torch.zeros(1, 16, 48, dtype=BF, device="cuda"), 4, 4)
    merge = swin.PatchMerging(32, norm_layer=lambda d: torch.nn.GroupNorm(1, d)).to(BF).cuda()
    merge.fused = True
    with pytest.raises(NotImplementedError, match="nn.LayerNorm"):
        merge(torch.zeros(1, 16, 32, dtype=BF, device="cuda"), 4, 4)
    embed = swin.PatchEmbed(4, 3, 48, torch.nn.LayerNorm).to(BF).cuda()      # embed_dim 48
    embed.fused = True
    with pytest.raises(RuntimeError, match="msda_swin_linear_bf16"):
        embed(torch.zeros(1, 3, 8, 8, dtype=BF, device="cuda"))
    embed = swin.PatchEmbed(4, 3, 32, None).to(BF).cuda()      # patch_norm=False: the projection alone
    embed.fused = True
    img = torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(2)).to(BF).cuda()
    with torch.no_grad():
        tok, Wh, Ww = embed.tokens(img)
        assert (Wh, Ww) == (2, 2) and tok.shape == (1, 4, 32) and embed(img).shape == (1, 32, 2, 2)
        embed.fused = False
        want = embed(img).float()      # (torch's bf16 convolution: a different rounding order, each element within a bf16 rounding or two)
    assert float((want - tok.transpose(1, 2).reshape(1, 32, 2, 2).float()).pow(2).mean().sqrt()) < 2.0 ** -7 * float(want.pow(2).mean().sqrt())


# ---- the fixture with the stage switch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [True, False])
@pytest.mark.parametrize("n", [0, 1, 2])
def test_basic_layer_fused_stages_against_the_fixture(n, blocks):
    from richsem_amd import swin
    tag = f"layer{n}"
    H, W, w, nH = (int(v) for v in A.fixture()[f"{tag}.cfg"])
    sd = A.fixture_state_dict(tag, BF)
    layer = swin.BasicLayer(dim=32 * nH, depth=2, num_heads=nH, window_size=w, mlp_ratio=1., downsample=swin.PatchMerging).to(BF)
    layer.load_state_dict(sd, strict=True)
    layer.cuda().set_fused(blocks).downsample.fused = True
    x = A.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    x_out, _, _, x_down, _, _ = layer(x, H, W)
    _backward(tag, (x_out, x_down))
    kernel = _results(tag, (x_out, x_down), x, {k: p.grad for k, p in layer.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point}
    xc = A.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    outs = comp_layer(P, "", xc, H, W, w, nH, True)
    _backward(tag, outs)
    _compare(tag, kernel, _results(tag, outs, xc, {k: p.grad for k, p in P.items()}))


@pytest.mark.parametrize("blocks", [True, False])
def test_toy_backbone_fused_stages_against_the_fixture(blocks):
    from richsem_amd import swin
    sd = A.fixture_state_dict("net", BF)
    net = swin.SwinTransformer(**NET).to(BF)
    net.load_state_dict(sd, strict=True)
    net.cuda().set_fused(blocks).set_fused_stages(True)
    img = A.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    feats = net.forward_raw(img)
    assert [tuple(f.shape) for f in feats] == [(2, 32, 10, 13), (2, 64, 5, 7)] and all(f.is_contiguous() for f in feats)
    _backward("net", feats)
    kernel = _results("net", feats, img, {k: p.grad for k, p in net.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point}
    imgc = A.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    outs = comp_net(P, imgc)
    _backward("net", outs)
    _compare("net", kernel, _results("net", outs, imgc, {k: p.grad for k, p in P.items()}))


# ---- the padded embedding --------------------------------------------------------------------------------------------------------------
def test_padded_patch_embedding_against_the_float64_module():
    """PatchEmbed(4, 3, 32, LayerNorm) on a (2, 3, 13, 18) image (padded both ways), output and all gradients: the reference is the package's
    float64 CPU module (pinned by the fixture in tests/test_swin_host.py), the comparator a torch bf16 composition written here; per tensor
    err(kernel path) <= 2 err(composition), err = rms of the difference to the float64 result"""
    from richsem_amd import swin
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    ref = swin.PatchEmbed(4, 3, 32, torch.nn.LayerNorm)
    with torch.no_grad():
        ref.norm.weight.add_(0.3 * torch.randn(32, generator=gen))
        ref.norm.bias.add_(0.3 * torch.randn(32, generator=gen))
        for p in ref.parameters():      # the stored values are bf16: their float64 copies are exact
            p.copy_(p.to(BF))
    img = torch.randn(2, 3, 13, 18, generator=gen).to(BF)
    g = torch.randn(2, 32, 4, 5, generator=gen)

    def run(module, image, grad):
        image = image.requires_grad_(True)
        out = module(image)
        (out.float() * grad if out.dtype == BF else out * grad).sum().backward()
        res = {"out": out.detach(), "img_grad": image.grad}
        res.update({k: p.grad for k, p in module.named_parameters()})
        return res

    import copy
    want = run(copy.deepcopy(ref).double(), img.double(), g.double())
    dev = copy.deepcopy(ref).to(BF).cuda()
    dev.fused = True
    kernel = run(dev, img.cuda(), g.cuda())

    P = {k: p.detach().to(BF).cuda().requires_grad_(True) for k, p in ref.named_parameters()}
    imgc = img.cuda().requires_grad_(True)
    x = F.conv2d(F.pad(imgc, (0, 2, 0, 3)), P["proj.weight"], P["proj.bias"], stride=4)
    x = F.layer_norm(x.flatten(2).transpose(1, 2), (32,), P["norm.weight"], P["norm.bias"]).transpose(1, 2).reshape(2, 32, 4, 5)
    (x.float() * g.cuda()).sum().backward()
    comp = {"out": x.detach(), "img_grad": imgc.grad}
    comp.update({k: p.grad for k, p in P.items()})

    assert sorted(kernel) == sorted(comp) == sorted(want) and len(want) == 6
    bad = []
    for name in sorted(want):
        assert kernel[name].shape == want[name].shape and bool(torch.isfinite(kernel[name].float()).all()), name
        ek = float((kernel[name].double().cpu() - want[name]).pow(2).mean().sqrt())
        ec = float((comp[name].double().cpu() - want[name]).pow(2).mean().sqrt())
        line = f"[measured] padded embed {name} rms={float(want[name].pow(2).mean().sqrt()):.3g} kernel_err={ek:.3g} composition_err={ec:.3g} ratio={ek / max(ec, 1e-300):.2f}"
        if REPORT:
            print(line, flush=True)
        if not ek <= 2 * ec:
            bad.append(line)
    assert not bad, "\n".join(bad)
