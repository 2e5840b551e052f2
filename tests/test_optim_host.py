"""CPU: the library optimizer's definition, bounds, parameter groups, chunk planner and host argument checks (no kernel is launched).

tests/optim_ref.py restates clip_grad_norm_ + AdamW (+ EMA) in float64 with element-wise bounds; here it is checked against torch itself
in float64, its fp32 emulation of the kernels sits inside the bounds, and four wrong restatements sit far outside them."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as R
from richsem_amd import _build, _lib

GROUPS = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1),
          dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]
SHAPES = [(7,), (3, 5), (1,), (64,), (2, 2)]
GROUP_OF = [0, 1, 0, 1, 0]
NO_GRAD = 2                  # this tensor never has a gradient
MAX_NORM = 0.1               # the gradients below have norm ~ 30: clipping is active by a factor of ~300


def _inputs(seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    p = [torch.randn(s, generator=gen).to(dtype) for s in SHAPES]
    grads = [[None if i == NO_GRAD else (torch.randn(s, generator=gen) * 3).to(dtype) for i, s in enumerate(SHAPES)] for _ in range(3)]
    return p, grads


def _chain(fn, p, grads, max_norm, **kw):
    """three steps of ``fn`` (reference or emulate), each from the previous step's results; -> list of the three value dicts"""
    m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    step, outs = [0] * len(p), []
    for g in grads:
        out = fn(p, g, m, v, step, GROUPS, GROUP_OF, max_norm, **kw)
        out = out[0] if isinstance(out, tuple) else out
        p, m, v, step = out["p"], out["m"], out["v"], out["step"]
        outs.append(out)
    return outs


@pytest.mark.parametrize("max_norm", [MAX_NORM, 0.0, 1e4])
def test_reference_is_torch_adamw_after_clip_grad_norm(max_norm):
    p0, grads = _inputs(0, torch.float64)
    params = [x.clone().requires_grad_(True) for x in p0]
    opt = torch.optim.AdamW([dict(params=[params[i] for i in range(len(params)) if GROUP_OF[i] == gi], **G) for gi, G in enumerate(GROUPS)],
                            foreach=False)
    outs = _chain(R.reference, p0, grads, max_norm)
    for k, g in enumerate(grads):
        for x, gi in zip(params, g):
            x.grad = None if gi is None else gi.clone()
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm > 0 else None      # (engine.py:111: only when max_norm > 0)
        opt.step()
        if norm is not None:
            assert abs(float(norm) - float(outs[k]["total_norm"])) <= 1e-12 * float(norm)
        for i, x in enumerate(params):
            want = [x.detach()] + ([opt.state[x]["exp_avg"], opt.state[x]["exp_avg_sq"]] if i != NO_GRAD else [])
            for a, b in zip(want, (outs[k]["p"][i], outs[k]["m"][i], outs[k]["v"][i])):
                assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), (k, i)
        assert outs[k]["step"] == [k + 1 if i != NO_GRAD else 0 for i in range(len(params))]
    assert NO_GRAD not in [i for i, x in enumerate(params) if len(opt.state[x])]
    assert torch.equal(params[NO_GRAD].detach(), p0[NO_GRAD])


@pytest.mark.parametrize("max_norm", [MAX_NORM, 0.0, 1e4])
def test_emulation_of_the_kernels_is_inside_the_bounds(max_norm):
    p, grads = _inputs(1)
    gen = torch.Generator().manual_seed(5)
    ema = [None if i == 3 else torch.randn(s, generator=gen) for i, s in enumerate(SHAPES)]
    m, v, step = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p], [0] * len(p)
    for g in grads:
        args = (p, g, m, v, step, GROUPS, GROUP_OF, max_norm)
        val, bnd = R.reference(*args, ema=ema, ema_decay=0.99)
        got = R.emulate(*args, ema=ema, ema_decay=0.99)
        ratio = R.ratios(got, val, bnd)
        assert max(ratio.values()) <= 1.0, ratio
        assert got["step"] == val["step"]
        for i in range(len(p)):
            if g[i] is None:
                assert all(torch.equal(got[k][i], (p, m, v, ema)[j][i]) for j, k in enumerate(R.TENSORS))
        p, m, v, step, ema = got["p"], got["m"], got["v"], got["step"], got["ema"]


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_bounds_tell_wrong_restatements_apart(variant):
    """L2-coupled decay, eps inside the square root, clipping left off, the bias corrections one step off: each is a plausible AdamW that is
    NOT torch's, and each lands more than ten bounds away somewhere within three steps (norm ~300 x max_norm, wd = 0.1, steps 1..3)"""
    p, grads = _inputs(2)
    m, v, step = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p], [0] * len(p)
    worst = 0.0
    for g in grads:
        args = (p, g, m, v, step, GROUPS, GROUP_OF, MAX_NORM)
        val, bnd = R.reference(*args)
        wrong, _ = R.reference(*args, variant=variant)
        worst = max(worst, max(R.ratios(wrong, val, bnd, keys=("p", "m", "v")).values()))
        got = R.emulate(*args)
        p, m, v, step = got["p"], got["m"], got["v"], got["step"]
    assert worst > 10.0, (variant, worst)


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        lin = lambda: torch.nn.Linear(2, 2)
        self.backbone = torch.nn.ModuleList([torch.nn.ModuleDict({"conv": lin(), "norm": torch.nn.LayerNorm(2)}), lin()])
        self.encoder = torch.nn.ModuleDict({"sampling_offsets": lin(), "norm": torch.nn.LayerNorm(2), "proj": lin()})
        self.reference_points = lin()
        self.frozen = lin()
        for q in self.frozen.parameters():
            q.requires_grad_(False)


def test_param_groups_are_the_references_three_groupings():
    from richsem_amd.optim import param_groups
    model = _Toy()
    names = {id(q): n for n, q in model.named_parameters()}
    got = lambda **kw: [sorted(names[id(q)] for q in g["params"]) for g in param_groups(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-3, **kw)]
    opts = lambda **kw: [{k: v for k, v in g.items() if k != "params"} for g in param_groups(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-3, **kw)]
    bb0 = ["backbone.0.conv.bias", "backbone.0.conv.weight", "backbone.0.norm.bias", "backbone.0.norm.weight"]
    bb1 = ["backbone.1.bias", "backbone.1.weight"]
    enc = ["encoder.norm.bias", "encoder.norm.weight", "encoder.proj.bias", "encoder.proj.weight"]
    so = ["encoder.sampling_offsets.bias", "encoder.sampling_offsets.weight"]
    rp = ["reference_points.bias", "reference_points.weight"]
    assert got() == [sorted(enc + so + rp), sorted(bb0 + bb1)]
    assert opts() == [{}, {"lr": 1e-5}]
    # ddetr_in_mmdet: "backbone.0" only -- backbone.1 stays in the first group
    assert got(param_dict_type="ddetr_in_mmdet") == [sorted(bb1 + enc), bb0, sorted(so + rp)]
    assert opts(param_dict_type="ddetr_in_mmdet") == [{"lr": 1e-4}, {"lr": 1e-5}, {"lr": pytest.approx(1e-5)}]
    assert got(param_dict_type="ddetr_in_mmdet", lr_linear_proj_names=("sampling_offsets",), lr_linear_proj_mult=0.5)[2] == so
    assert got(param_dict_type="large_wd") == [
        ["encoder.proj.weight", "encoder.sampling_offsets.weight", "reference_points.weight"],
        ["backbone.0.conv.bias", "backbone.0.norm.bias", "backbone.0.norm.weight", "backbone.1.bias"],
        ["backbone.0.conv.weight", "backbone.1.weight"],
        ["encoder.norm.bias", "encoder.norm.weight", "encoder.proj.bias", "encoder.sampling_offsets.bias", "reference_points.bias"]]
    assert opts(param_dict_type="large_wd") == [{}, {"lr": 1e-5, "weight_decay": 0.0}, {"lr": 1e-5, "weight_decay": 1e-3},
                                                {"lr": 1e-4, "weight_decay": 0.0}]
    with pytest.raises(ValueError):
        param_groups(model, 1e-4, 1e-5, 1e-3, param_dict_type="other")
    assert not any("frozen" in n for grp in got() for n in grp)


def test_construction_refuses_what_the_kernels_do_not_do():
    from richsem_amd.optim import ClipAdamW
    ok = torch.nn.Parameter(torch.zeros(4, 3))
    ClipAdamW([ok], lr=1e-3)
    with pytest.raises(ValueError, match="amsgrad"):
        ClipAdamW([ok], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        ClipAdamW([ok], maximize=True)
    with pytest.raises(TypeError, match="float32"):
        ClipAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(TypeError, match="float32"):
        ClipAdamW([ok, torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        ClipAdamW([torch.nn.Parameter(torch.zeros(4, 3).t())])
    with pytest.raises(ValueError):
        ClipAdamW([ok], betas=(1.0, 0.9))
    opt = ClipAdamW([{"params": [ok], "lr": 5e-4}], lr=1e-3, weight_decay=0.2, max_norm=0.1)
    assert opt.param_groups[0]["lr"] == 5e-4 and opt.param_groups[0]["weight_decay"] == 0.2 and opt.max_norm == 0.1
    assert set(torch.optim.AdamW([ok]).param_groups[0]) == set(opt.param_groups[0])      # a state_dict moves both ways


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


CHUNK = _lib.OPTIM_CHUNK


@pytest.mark.parametrize("sizes", [[1], [CHUNK - 1], [CHUNK], [CHUNK + 1], [2 * CHUNK + 3], [1] * 300,
                                   [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3] + [1] * 300 + [5 * CHUNK]])
def test_chunk_planner_covers_every_element_once_in_order(lib, sizes):
    from richsem_amd.optim import plan_chunks
    chunks = plan_chunks(sizes)
    assert len(chunks) == sum(-(-s // CHUNK) for s in sizes)
    at = 0
    for t, size in enumerate(sizes):
        off = 0
        while off < size:
            c = chunks[at]
            assert (int(c["tensor"]), int(c["offset"])) == (t, off)            # in order, never spanning two tensors
            assert 1 <= int(c["count"]) <= CHUNK and off + int(c["count"]) <= size
            assert int(c["count"]) == CHUNK or off + int(c["count"]) == size   # only a tensor's last chunk is short
            off += int(c["count"])
            at += 1
        assert off == size
    assert at == len(chunks)


def test_header_constant_and_layouts_agree():
    import os
    import re
    from conftest import ROOT
    from richsem_amd import optim
    text = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    assert int(re.search(r"#define MSDA_OPTIM_CHUNK (\d+)", text).group(1)) == CHUNK == optim.CHUNK
    assert optim.TENSOR_DT.names == ("param", "grad", "exp_avg", "exp_avg_sq", "ema", "step", "numel", "group", "reserved")


def test_entry_points_check_their_arguments_on_the_host(lib):
    """null tables, non-positive counts and tables off their element alignment are refused before any launch (fake pointers: none is
    dereferenced), each with the usual code and the entry point's name in msda_last_error()"""
    p, n = 0x1000, ctypes.c_int64(0)
    nums = np.array([5, 0], dtype=np.int64)
    out = np.zeros(4, dtype=np.dtype([("offset", "<i8"), ("tensor", "<i4"), ("count", "<i4")]))
    assert lib.msda_optim_plan(None, 1, None, 0, ctypes.byref(n)) == -1
    assert lib.msda_optim_plan(nums.ctypes.data, 1, None, 0, None) == -1
    assert lib.msda_optim_plan(nums.ctypes.data, 0, None, 0, ctypes.byref(n)) == -2
    assert lib.msda_optim_plan(nums.ctypes.data, 2, None, 0, ctypes.byref(n)) == -2            # an empty tensor
    assert lib.msda_optim_plan(nums.ctypes.data, 1, out.ctypes.data, 0, ctypes.byref(n)) == -2  # no room
    assert lib.msda_optim_plan(nums.ctypes.data + 4, 1, None, 0, ctypes.byref(n)) == -5
    big = np.array([CHUNK * 3 + 1], dtype=np.int64)
    assert lib.msda_optim_plan(big.ctypes.data, 1, out.ctypes.data, 3, ctypes.byref(n)) == -2 and "msda_optim_plan" in _lib.last_error()
    assert lib.msda_optim_plan(big.ctypes.data, 1, out.ctypes.data, 4, ctypes.byref(n)) == 0 and n.value == 4
    huge = np.array([CHUNK << 31], dtype=np.int64)
    assert lib.msda_optim_plan(huge.ctypes.data, 1, None, 0, ctypes.byref(n)) == -4

    sumsq = lambda a=p, b=p, k=3, c=p: lib.msda_optim_sumsq(a, b, k, c, None)
    step = lambda a=p, b=p, k=3, c=p, d=p, e=p, f=p: lib.msda_optim_step(a, b, k, c, d, e, f, None)
    ema = lambda a=p, b=p, k=3, c=p: lib.msda_optim_ema(a, b, k, c, None)
    for name, fn, n_ptr in (("msda_optim_sumsq", sumsq, 3), ("msda_optim_step", step, 6), ("msda_optim_ema", ema, 3)):
        keys = "abcdef"[:n_ptr]
        for key in keys:
            assert fn(**{key: None}) == -1, (name, key)
            assert name in _lib.last_error() and "null pointer" in _lib.last_error()
            bad = p + (2 if (name, key) == ("msda_optim_step", "f") else 4)      # total_norm: a float; every table: 8 bytes
            assert fn(**{key: bad}) == -5, (name, key)
            assert name in _lib.last_error()
        for k in (0, -1):
            assert fn(k=k) == -2, (name, k)
    with pytest.raises(RuntimeError, match="msda_optim_step.*MSDA_ERR_MISALIGNED"):
        _lib.check(step(d=p + 4))
