"""GPU (-m gpu): the bf16 entry points (msda_forward_bf16 / msda_backward_bf16, row "dagger" of VERDICT round 1) -- value,
out, grad_output, grad_value in bfloat16; sampling locations, attention weights and their gradients in float32; all
accumulation in fp32.  The reference has no half path (ms_deform_attn_cuda.cu:64,134), so parity is defined against the
oracle run (in float32) on the SAME bf16-rounded inputs:
  * out and grad_value are rounded to bf16 once at the store: |err| <= 2^-9 |x| per element (round to nearest, 8
    significant bits) plus the fp32 accumulation error (~1e-6) -> tolerance 4e-3 of the tensor's largest magnitude,
    AND -- the stronger statement -- the result must equal the correctly rounded oracle value up to ONE bf16 ulp
    almost everywhere (sums are formed in fp32, never in bf16; a bf16 running sum would be off by many ulps);
  * grad_sampling_loc / grad_attn_weight are float32 outputs of exact (bf16-valued) inputs: the fp32 tolerance 2e-4.
The element-wise statement -- every stored element between the bf16 roundings of the float64 reference -+ the fp32 sum's bound (a bf16
store is off by up to 2^-8 of the number, 8 significant bits), no share of elements exempt, none skipped for being small -- lives in
tests/test_gpu_msda_bounds.py (comparator: tests/msda_ref.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import msda_oracle as O
from richsem_amd import _lib, workload as W
from richsem_amd import MultiScaleDeformableAttention as MSDA
from richsem_amd.functions import MSDeformAttnFunction

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    yield
    _lib.set_option("fwd_variant", 0)
    _lib.set_option("bwd_variant", 0)


def rel_err(a, b):
    a = a.detach().float().cpu().numpy().astype(np.float64) if hasattr(a, "detach") else a
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def ulp_share(a_bf16, ref64):
    """share of elements further than one bf16 ulp from the correctly rounded reference"""
    ref = torch.from_numpy(ref64).float().to(torch.bfloat16)
    ai = a_bf16.detach().cpu().view(torch.int16).to(torch.int32)
    ri = ref.view(torch.int16).to(torch.int32)
    # compare in the ordered-integer domain of bf16 bit patterns (sign-magnitude -> monotone)
    ai = torch.where(ai < 0, -(ai & 0x7FFF), ai)
    ri = torch.where(ri < 0, -(ri & 0x7FFF), ri)
    big = (ai - ri).abs() > 1
    # cancellation: elements tiny against the tensor's scale carry no relative information
    big &= torch.from_numpy(np.abs(ref64) > 1e-3 * np.abs(ref64).max())
    return float(big.float().mean())


def run_bf16(z, variant):
    """variant: 1 direct kernels; 2 window forward + routed backward; 4 direct forward + routed backward; 5 direct forward + row-band backward"""
    _lib.set_option("fwd_variant", {1: 1, 2: 2, 4: 1, 5: 1}[variant])
    _lib.set_option("bwd_variant", {1: 1, 2: 4, 4: 4, 5: 5}[variant])
    v = torch.from_numpy(z["value"]).float().to(torch.bfloat16).cuda()
    go = torch.from_numpy(z["grad_out"]).float().to(torch.bfloat16).cuda().contiguous()
    sh, ls = torch.from_numpy(z["shapes"]).cuda(), torch.from_numpy(z["lsi"]).cuda()
    loc, aw = torch.from_numpy(z["loc"]).float().cuda(), torch.from_numpy(z["aw"]).float().cuda()
    out = MSDA.ms_deform_attn_forward(v, sh, ls, loc, aw, 64)
    gv, gl, ga = MSDA.ms_deform_attn_backward(v, sh, ls, loc, aw, go, 64)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and gv.dtype == torch.bfloat16 and gl.dtype == torch.float32 and ga.dtype == torch.float32
    # the oracle on the bf16-rounded inputs, in float32 like the kernels (the same floor() decisions for samples that sit
    # within rounding of a pixel boundary; its own accumulation error, ~1e-6, is far below the bf16 output rounding)
    v32, go32 = v.float().cpu().numpy(), go.float().cpu().numpy()
    loc32, aw32 = loc.cpu().numpy(), aw.cpu().numpy()
    oo = O.forward(v32, z["shapes"], z["lsi"], loc32, aw32).astype(np.float64)
    ogv, ogl, oga = (a.astype(np.float64) for a in O.backward(v32, z["shapes"], z["lsi"], loc32, aw32, go32))
    return (out, gv, gl, ga), (oo, ogv, ogl, oga)


def check(got, want, loc64=None):
    out, gv, gl, ga = got
    oo, ogv, ogl, oga = want
    assert rel_err(out, oo) < 4e-3 and rel_err(gv, ogv) < 4e-3
    assert ulp_share(out, oo) < 1e-3, "out is not the once-rounded fp32 sum"
    assert ulp_share(gv, ogv) < 1e-3, "grad_value is not the once-rounded fp32 sum (was it accumulated in bf16?)"
    assert rel_err(ga, oga) < 2e-4
    assert rel_err(gl, ogl) < 2e-4


@pytest.mark.parametrize("variant", [1, 2, 4])
@pytest.mark.parametrize("case", ["pyramid_encoder_f32", "decoder_n2m8_f64", "ref_test_grad_D32", "ref_test_grad_D30",
                                  "border_bands_grad"])
def test_bf16_golden_inputs(case, variant):
    z = dict(np.load(os.path.join(GOLDEN, case + ".npz")))
    got, want = run_bf16(z, variant)
    if case == "border_bands_grad":   # exact-border samples: grid_sample vs kernel convention, see test_oracle_golden.py
        pass
    check(got, want)


@pytest.mark.parametrize("variant", [1, 2, 4, 5])   # direct; window forward + routed backward; direct forward + routed backward; + row-band backward
@pytest.mark.parametrize("loc_mode", ["init", "sigma4", "uniform"])
@pytest.mark.parametrize("which", ["E", "Dd", "Em"])
def test_bf16_shrunk_baseline_calls(which, loc_mode, variant):
    call = W.shrunk({"E": W.call_E, "Dd": W.call_Dd, "Em": W.call_Em}[which](2), 4)
    z = {k: v.numpy() for k, v in W.make_inputs(call, loc_mode, seed=13).items()}
    got, want = run_bf16(z, variant)
    check(got, want)


@pytest.mark.parametrize("dims", [
    dict(N=1, M=2, D=30, P=3, shapes=[(9, 7), (3, 2)], Lq=40),        # two channels per lane
    dict(N=2, M=3, D=7, P=2, shapes=[(5, 5)], Lq=9),                  # one channel per lane, odd value count: scratch + rounding
    dict(N=1, M=1, D=64, P=4, shapes=[(300, 300), (9, 9)], Lq=64),    # level too large for the LDS windows: fp32 scratch
    dict(N=1, M=1, D=3, P=2, shapes=[(301, 301)], Lq=50),             # scratch, value count not a multiple of 4
])
def test_bf16_odd_shapes(dims):
    call = W.Call("o", dims["N"], dims["M"], dims["D"], dims["P"], dims["shapes"], dims["Lq"], False)
    z = {k: v.numpy() for k, v in W.make_inputs(call, "uniform", seed=3).items()}
    got, want = run_bf16(z, 1)
    check(got, want)


@pytest.mark.parametrize("opts", [{}, {"band_hits": 200}, {"band_lds_kb": 150}])
def test_bf16_band_backward_full_size_decoder_call(opts):
    """the decoder call Dd at full size in bf16 storage: the row-band kernel (bwd_variant 5); slabbed levels go through the fp32
    scratch image and one rounding (band_hits = 200: levels 1-3)"""
    from test_gpu_parity import _profiled_variants
    call = W.call_Dd(2)
    z = {k: v.numpy() for k, v in W.make_inputs(call, "init", seed=17).items()}
    defaults = {k: _lib.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        got, want = run_bf16(z, 5)
        check(got, want)
        v = torch.from_numpy(z["value"]).to(torch.bfloat16).cuda()
        go = torch.from_numpy(z["grad_out"]).to(torch.bfloat16).cuda()
        args = [torch.from_numpy(z[k]).cuda() for k in ("shapes", "lsi", "loc", "aw")]
        assert _profiled_variants(lambda: MSDA.ms_deform_attn_backward(v, *args, go, 64)) == [("bwd", 5)]
    finally:
        for k, v in defaults.items():
            _lib.set_option(k, v)


def test_bf16_autograd_function_and_full_size_adjoint():
    """Through the autograd binding at BASELINE's full E size: <out, g> == <value, grad_value> within bf16 rounding."""
    call = W.call_E(2)
    t = W.make_inputs(call, "init", seed=0, device="cuda")
    v = t["value"].to(torch.bfloat16).requires_grad_(True)
    loc, aw = t["loc"].clone().requires_grad_(True), t["aw"].clone().requires_grad_(True)
    out = MSDeformAttnFunction.apply(v, t["shapes"], t["lsi"], loc, aw, 64)
    g = t["grad_out"].to(torch.bfloat16)
    out.backward(g)
    assert v.grad.dtype == torch.bfloat16 and loc.grad.dtype == torch.float32
    a, b_ = out.detach().double() * g.double(), v.detach().double() * v.grad.double()
    lhs, rhs = a.sum(), b_.sum()
    # both sides are sums of ~1e7 terms whose factors carry an independent bf16 rounding (relative 2^-9, random sign)
    noise = 2.0 ** -9 * float((a.pow(2).sum() + b_.pow(2).sum()).sqrt())
    assert abs(float(lhs - rhs)) < 4 * noise + 1e-6 * abs(float(lhs))
    # against the fp32 path on the same (bf16-valued) inputs
    out32 = MSDA.ms_deform_attn_forward(v.detach().float(), t["shapes"], t["lsi"], loc.detach(), aw.detach(), 64)
    assert float((out.float() - out32).abs().max()) <= 2 ** -8 * float(out32.abs().max()) + 1e-5
