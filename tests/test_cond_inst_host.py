"""The host layer of the dynamic mask head (richsem_amd/cond_inst.py) without a GPU: the torch composition and ``MaskBranch`` against the
reference's numbers in float64 (tests/golden/dynamic_masks/dynamic_masks_reference.npz), the capacity path against the list path, the dispatch rule
and the refusals, the workspace mirror, the C ABI's declarations, bindings and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dynamic_masks_ref as R
from richsem_amd import _build, _lib, cond_inst, masks

DYN, BRANCH = R.load_golden()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["msda_dynmask_workspace_bytes", "msda_dynmask_table", "msda_dynmask_forward_f32", "msda_dynmask_forward_bf16",
           "msda_dynmask_backward_f32", "msda_dynmask_backward_bf16"]


def tensors_of(case, device="cpu", dtype=torch.float64):
    """-> feats, params, ref (N, Q, 4), sizes (N, 2), inst (N, R) int64, gout as tensors"""
    t = lambda k, d: torch.from_numpy(np.ascontiguousarray(case[k])).to(device=device, dtype=d)      # noqa: E731
    return t("feats", dtype), t("params", dtype), t("ref", torch.float64 if dtype == torch.float64 else torch.float32), \
        t("sizes", torch.float32), t("inst", torch.int64), t("gout", dtype)


def branch_of(dtype=torch.float64):
    m = cond_inst.MaskBranch(32, channel_div=8)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.load_branch_weights().items()})
    return m.to(dtype)


def branch_inputs(case, dtype=torch.float64):
    hs, refs, sizes = (torch.from_numpy(case[k]).to(dtype) for k in ("hs", "references", "sizes"))
    memory = [torch.from_numpy(case[f"mem{i}"]).to(dtype) for i in range(3)]
    indices = [[(torch.from_numpy(case[f"idx_l{lvl}_i{n}"]), None) for n in range(hs.shape[1])] for lvl in range(hs.shape[0])]
    return hs, memory, refs, indices, [{"size": s} for s in sizes]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name", list(DYN))
def test_float64_path_matches_the_reference(name):
    case = DYN[name]
    feats, params, ref, sizes, inst, gout = tensors_of(case)
    for t in (feats, params, ref):
        t.requires_grad_(True)
    out = cond_inst._with_table(feats, params, ref, sizes, inst, rel_coord=bool(case["rel"]))      # (CPU float64 tensors: the composition)
    assert out.dtype == torch.float64 and tuple(out.shape) == case["out"].shape
    np.testing.assert_allclose(out.detach().numpy(), case["out"], rtol=1e-9, atol=1e-12)
    assert not out.detach()[inst < 0].any()
    (out * gout).sum().backward()
    np.testing.assert_allclose(feats.grad.numpy(), case["g_feats"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(params.grad.numpy(), case["g_params"], rtol=1e-9, atol=1e-11)
    if ref.grad is None:
        assert not int(case["rel"]) or not (inst >= 0).any()
    else:
        # the reference rounds the coordinates' gradient to float32 pixel by pixel (its .float()); the composition does not: they differ by
        # that rounding, which the restatement's fp32 bound of grad_ref contains
        assert not ref.grad[..., 2:].any()
        assert (np.abs(ref.grad[..., :2].numpy() - case["g_ref"]) <= R.dynamic_masks(case)["b_g_ref"]).all()


def test_all_queries_and_selected_rows():
    case = DYN["c8_rel_9x13"]
    feats, params, ref, sizes, inst, _ = tensors_of(case)
    every = cond_inst.dynamic_masks(feats, params, ref, sizes)
    assert tuple(every.shape) == (2, 4, 18, 26)
    listed = cond_inst.dynamic_masks(feats, params, ref, sizes, rows=inst)
    np.testing.assert_allclose(listed.numpy(), case["out"], rtol=1e-9, atol=1e-12)
    for n in range(2):
        for r in range(inst.shape[1]):
            if inst[n, r] >= 0:
                assert torch.equal(listed[n, r], every[n, inst[n, r]])
    with pytest.raises(RuntimeError, match="rows= is forward-only"):
        cond_inst.dynamic_masks(feats, params.clone().requires_grad_(True), ref, sizes, rows=inst)
    with torch.no_grad():
        cond_inst.dynamic_masks(feats, params.clone().requires_grad_(True), ref, sizes, rows=inst)
    one = cond_inst.dynamic_masks(feats, params, ref, sizes, mask_out_stride=8)
    assert tuple(one.shape) == (2, 4, 9, 13) and torch.equal(one, every[:, :, 1::2, 1::2])


def test_matched_table_follows_the_buffers():
    mt = masks.MaskTargets(2, 6, (32, 32), "cpu").update_([{"masks": torch.ones(1, 8, 8, dtype=torch.bool)},
                                                           {"masks": torch.ones(3, 8, 8, dtype=torch.bool)}])
    qot = torch.tensor([2, 0, 7, -1, 3, 1])      # slot 2: out of range, slot 3: unmatched, slots 4 and 5: dead
    inst = cond_inst.table_torch(2, 4, "cpu", mt, qot)
    assert inst.tolist() == [[-1, -1, 2, -1], [0, -1, -1, -1]]
    assert cond_inst.table_torch(2, 3, "cpu").tolist() == [[0, 1, 2], [0, 1, 2]]
    assert cond_inst.table_torch(1, 3, "cpu", rows=torch.tensor([[2, 3, -1, 0]])).tolist() == [[2, -1, -1, 0]]


@pytest.mark.parametrize("name", list(BRANCH))
def test_mask_branch_matches_the_reference(name):
    case = BRANCH[name]
    m = branch_of().train(bool(case["training"]))
    assert m.in_channels == 8 and m.num_gen_params == 169
    with torch.no_grad():
        out_masks, out_params = m(*branch_inputs(case))
    assert len(out_masks) == len(out_params) == 2
    for lvl in range(2):
        assert tuple(out_masks[lvl].shape) == case[f"masks{lvl}"].shape
        np.testing.assert_allclose(out_params[lvl].numpy(), case[f"params{lvl}"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(out_masks[lvl].numpy(), case[f"masks{lvl}"], rtol=1e-9, atol=1e-10)


def test_state_dict_keys_are_the_references():
    keys = set(cond_inst.MaskBranch(32, channel_div=8).state_dict())
    assert keys == set(R.load_branch_weights())
    assert keys == {f"controller.layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")} | \
        {f"mask_head.{lay}.{p}" for lay in ("lay1", "lay2", "lay3", "lay4", "dcn") for p in ("weight", "bias")}
    m = cond_inst.MaskBranch(256)      # the reference's defaults: channel_div 32, concatenated memory
    assert m.in_channels == 16 and m.num_gen_params == 233 and m.mask_head.lay3.in_channels == 512
    assert cond_inst.MaskBranch(256, is_concat=False).in_channels == 8
    assert {k for k in cond_inst.MaskHeadSmallConv(64, [8, 8, 8], 64).state_dict() if k.startswith("adapter")} == \
        {f"adapter{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")}
    with pytest.raises(ValueError, match="the dynamic width is 8"):
        cond_inst.MaskBranch(32, dy_mask_channel=16)


def test_forward_capacity_equals_forward_on_the_matched_rows():
    case = BRANCH["branch_train"]
    m = branch_of().train()
    hs, memory, refs, indices, targets = branch_inputs(case)
    lvl = 1
    counts = [int(i.numel()) for i, _ in indices[lvl]]
    mt = masks.MaskTargets(2, sum(counts) + 2, (32, 32), "cpu").update_([{"masks": torch.ones(c, 8, 8, dtype=torch.bool)} for c in counts])
    qot = torch.full((mt.capacity,), -1, dtype=torch.int64)
    qot[:sum(counts)] = torch.cat([i for i, _ in indices[lvl]])
    with torch.no_grad():
        listed = m(hs, memory, refs, indices, targets)[0][lvl]
        cap = m.forward_capacity(hs[lvl], memory, refs[lvl], torch.stack([t["size"] for t in targets]), mt, qot)
    assert tuple(cap.shape) == (2, 5, 18, 26)
    k = 0
    for n, (pred_i, _) in enumerate(indices[lvl]):
        for q in range(5):
            if q not in pred_i.tolist():
                assert not cap[n, q].any()
        for q in pred_i.tolist():
            assert torch.equal(cap[n, q], listed[k, 0])
            k += 1
    # ... and mask_losses takes it as it is
    out = masks.mask_losses(cap, mt, qot, float(sum(counts)))
    assert torch.isfinite(out["loss_mask"]) and torch.isfinite(out["loss_dice"])


def test_dispatch_rule():
    f32 = torch.zeros(1, 8, 2, 2)
    assert not cond_inst.on_kernels(f32) and not cond_inst.on_kernels(f32.double())      # CPU tensors: the composition
    fake = type("T", (), {"is_cuda": True, "dtype": torch.float32, "shape": (1, 8, 2, 2), "dim": lambda self: 4})()
    assert cond_inst.on_kernels(fake) and not cond_inst.on_kernels(fake, use_relative_hw=True)
    assert cond_inst.on_kernels(fake, rel_coord=False, use_relative_hw=True)      # (without coordinates the switch changes nothing)
    for dt, c, want in ((torch.bfloat16, 16, True), (torch.float64, 8, False), (torch.float16, 8, False), (torch.float32, 12, False)):
        fake.dtype, fake.shape = dt, (1, c, 2, 2)
        assert cond_inst.on_kernels(fake) is want, (dt, c)
    # an unsupported channel count and use_relative_hw take the composition on any device: here, the CPU's
    gen = torch.Generator().manual_seed(1)
    feats, params = torch.randn(1, 12, 3, 4, generator=gen), torch.randn(1, 2, cond_inst.num_params(12), generator=gen)
    ref, sizes = torch.rand(1, 2, 4, generator=gen) * 0.5 + 0.25, torch.tensor([[24.0, 32.0]])
    assert tuple(cond_inst.dynamic_masks(feats, params, ref, sizes).shape) == (1, 2, 6, 8)
    rel_hw = cond_inst.dynamic_masks(feats, params, ref, sizes, use_relative_hw=True)
    assert tuple(rel_hw.shape) == (1, 2, 6, 8) and not torch.equal(rel_hw, cond_inst.dynamic_masks(feats, params, ref, sizes))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        cond_inst.dynamic_masks_and_grads(f32, torch.zeros(1, 2, 169), torch.zeros(1, 2, 2), torch.ones(1, 2), torch.zeros(1, 2, 4, 4))


def test_use_relative_hw_is_the_references_formula():
    """1 - |1 - |2 d / (h, w)||, then 2 / (w, h): restated on one instance"""
    ref = torch.tensor([[0.5, 0.25, 0.5, 0.75]], dtype=torch.float64)
    rel = cond_inst._relative_coords(ref, torch.tensor([[16.0, 32.0]]), 2, 3, True, torch.float64)
    d = torch.tensor([16.0 - 12.0, 4.0 - 4.0], dtype=torch.float64)      # pixel (0, 1)
    wh = torch.tensor([16.0, 12.0], dtype=torch.float64)
    want = (1 - (1 - (d / wh.flip(0) * 2).abs()).abs()) / wh * 2
    assert torch.allclose(rel[0, :, 0, 1], want, rtol=0, atol=1e-15)


def test_argument_checks_name_the_shapes():
    feats, params, ref, sizes, inst, _ = tensors_of(DYN["c8_rel_9x13"])
    with pytest.raises(ValueError, match=r"params is \(N, Q, P\) with N = 2 and P = 169"):
        cond_inst.dynamic_masks(feats, params[:, :, :168], ref, sizes)
    with pytest.raises(ValueError, match=r"params is \(N, Q, P\) with N = 2 and P = 153"):
        cond_inst.dynamic_masks(feats, params, ref, sizes, rel_coord=False)
    with pytest.raises(ValueError, match=r"ref is \(N, Q, >= 2\)"):
        cond_inst.dynamic_masks(feats, params, ref[:, :3], sizes)
    with pytest.raises(ValueError, match=r"sizes is \(N, 2\)"):
        cond_inst.dynamic_masks(feats, params, ref, sizes[:1])
    with pytest.raises(ValueError, match="mask_out_stride is 4 or 8"):
        cond_inst.dynamic_masks(feats, params, ref, sizes, mask_out_stride=2)
    with pytest.raises(TypeError, match="rows is an int64"):
        cond_inst.dynamic_masks(feats, params, ref, sizes, rows=inst.int())
    with pytest.raises(TypeError, match="come together"):
        cond_inst.dynamic_masks(feats, params, ref, sizes, query_of_target=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError, match="share their type"):
        cond_inst.dynamic_masks(feats, params.float(), ref, sizes)


def test_symbols_declared_bound_and_exported(lib):
    import richsem_amd
    header = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    assert re.search(r"#define RICHSEM_MSDA_ABI_VERSION 13\b", header) and _lib.ABI_VERSION == 13 and lib.msda_abi_version() == 13
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert _build.SOURCES[_build.SOURCES.index("dynamic_masks.hip") - 1] == "mask_terms.hip"
    for name in ("dynamic_masks", "dynamic_masks_torch", "dynamic_masks_and_grads", "MaskBranch", "MaskHeadSmallConv"):
        assert getattr(richsem_amd, name) is getattr(cond_inst, name)


def test_workspace_bytes_mirror(lib):
    for dims in ((2, 8, 9, 13, 4, 4), (2, 16, 100, 168, 900, 900), (1, 8, 1, 1, 1, 1), (2, 16, 25, 42, 64, 64), (3, 8, 8, 32, 5, 17),
                 (1, 16, 9, 33, 2, 300)):
        assert cond_inst.workspace_bytes(*dims) == cond_inst.workspace_bytes_host(*dims), dims


def test_entry_points_refuse_before_any_launch(lib):
    n = ctypes.c_int64(0)
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf) // 16 * 16 + 16
    for dims, code in (((2, 8, 9, 13, 4, 4), 0), ((2, 16, 9, 13, 4, 4), 0), ((2, 12, 9, 13, 4, 4), -2), ((2, 32, 9, 13, 4, 4), -2),
                       ((0, 8, 9, 13, 4, 4), -2), ((2, 8, 9, 13, 0, 4), -2), ((2, 8, 9, 13, 4, 0), -2), ((2, 8, 1 << 15, 13, 4, 4), -4),
                       ((70000, 8, 9, 13, 4, 4), -4), ((2, 8, 9, 13, 4, (1 << 20) + 1), -4)):
        assert lib.msda_dynmask_workspace_bytes(*dims, ctypes.byref(n)) == code, dims
        if code:
            assert _lib.last_error().startswith("msda_dynmask_workspace_bytes: "), _lib.last_error()
    assert lib.msda_dynmask_workspace_bytes(2, 8, 9, 13, 4, 4, None) == -1
    assert lib.msda_dynmask_table(None, None, None, 2, 4, 4, 1, None, None) == -1 and _lib.last_error().startswith("msda_dynmask_table: ")
    assert lib.msda_dynmask_table(None, p, None, 2, 4, 4, 1, p, None) == -1      # offsets without query_of_target
    assert lib.msda_dynmask_table(None, None, None, 2, 3, 4, 1, p, None) == -2      # the identity needs R = Q
    assert lib.msda_dynmask_table(p + 4, None, None, 2, 3, 4, 1, p, None) == -5
    for sfx in ("f32", "bf16"):
        fwd, bwd = (getattr(lib, f"msda_dynmask_{k}_{sfx}") for k in ("forward", "backward"))
        dims = (2, 8, 9, 13, 4, 4)
        assert fwd(None, p, p, p, p, *dims, 1, 2, p, None) == -1 and _lib.last_error().startswith(f"msda_dynmask_forward_{sfx}: ")
        assert fwd(p, p, None, p, p, *dims, 1, 2, p, None) == -1      # the coordinates need ref and sizes
        assert fwd(p, p, p, p, p, 2, 24, 9, 13, 4, 4, 1, 2, p, None) == -2
        assert fwd(p, p, p, p, p, *dims, 1, 3, p, None) == -2      # factor 1 or 2
        assert fwd(p, p, p, p, p, *dims, 2, 2, p, None) == -2      # rel_coord 0 or 1
        assert fwd(p, p, p, p, p + 2, *dims, 1, 2, p, None) == -5
        assert bwd(p, p, p, p, p, p, *dims, 1, 2, p, p, p, None, None) == -1 and _lib.last_error().startswith(f"msda_dynmask_backward_{sfx}: ")
        assert bwd(p, p, p, p, p, p, *dims, 1, 2, p, p, p, p + 4, None) == -5
        assert bwd(p, p, p, p, p, p, 2, 8, 9, 13, 4, 4, 1, 4, p, p, None, p, None) == -2
