"""GPU (-m gpu): the routed backward (msda_rps.h) after its LDS re-cut -- tile grids of up to 312 pixels (a 9-bit base-grid index in
the record code and in the walk units), chunks of 1536 records whose gradient stage reads the records from the pool a second time
instead of keeping them in LDS, and a planner that chooses the tiles from those limits.

Every case is compared with the C oracle (oracle/msda_oracle.c) on seeded inputs, the routed path forced with bwd_variant 4 and
checked to be the one that ran.  The bounds are those tests/test_gpu_parity.py applies to the routed backward (fp32: 2e-4 of the
tensor's largest magnitude for the three gradients) and tests/test_gpu_bf16.py to bf16 storage (grad_value 4e-3: rounded once at the
store; grad_sampling_loc / grad_attn_weight 2e-4).  N = 1 or 2, M = 2, D = 32."""
import numpy as np
import pytest
import torch

from oracle import msda_oracle as O
from richsem_amd import _lib, workload as W
from richsem_amd import MultiScaleDeformableAttention as MSDA

pytestmark = pytest.mark.gpu

TG = 2e-4            # tests/test_gpu_parity.py: tols(np.float32)[1]
TG_BF16_GV = 4e-3    # tests/test_gpu_bf16.py: check()
CHUNK = 1536         # kRpsChunk
GRID = 312           # kRpsMaxPx
M, D = 2, 32


@pytest.fixture(autouse=True)
def _restore():
    yield
    _lib.set_option("fwd_variant", 0)
    _lib.set_option("bwd_variant", 0)


def rel_err(a, b):
    a = a.detach().float().cpu().numpy().astype(np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def make(shapes, Lq, P, N=1, seed=0, spread=1.0):
    """seeded inputs; locations U(0, 1) * spread - (spread - 1) / 2 (spread > 1: samples outside the map)"""
    g = torch.Generator().manual_seed(seed)
    L, S = len(shapes), sum(h * w for h, w in shapes)
    call = W.Call("recut", N, M, D, P, list(shapes), Lq, False)
    sh, lsi = W.level_tensors(call)
    return dict(value=torch.randn(N, S, M, D, generator=g), shapes=sh, lsi=lsi,
                loc=(torch.rand(N, Lq, M, L, P, 2, generator=g) * spread - (spread - 1.0) / 2).contiguous(),
                aw=torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P).contiguous(),
                grad_out=torch.randn(N, Lq, M * D, generator=g))


def routed(t, bf16=False):
    """the routed backward of inputs t -> (grad_value, grad_loc, grad_aw); fails unless the routed kernels are what ran"""
    _lib.set_option("bwd_variant", 4)
    dt = torch.bfloat16 if bf16 else torch.float32
    v, go = t["value"].to(dt).cuda(), t["grad_out"].to(dt).cuda().contiguous()
    sh, ls, loc, aw = (t[k].cuda() for k in ("shapes", "lsi", "loc", "aw"))
    _lib.profile_enable(8)
    res = MSDA.ms_deform_attn_backward(v, sh, ls, loc, aw, go, 64)
    torch.cuda.synchronize()
    ran = [(r["kind"], r["variant"]) for r in _lib.profile_collect()]
    _lib.profile_enable(0)
    assert ran == [("bwd", 4)], ran
    return res


def oracle(t, bf16=False):
    v, go = t["value"], t["grad_out"]
    if bf16:      # (the oracle on the bf16-rounded operands, as in tests/test_gpu_bf16.py)
        v, go = v.bfloat16().float(), go.bfloat16().float()
    return O.backward(v.numpy(), t["shapes"].numpy(), t["lsi"].numpy(), t["loc"].numpy(), t["aw"].numpy(), go.numpy())


def check(t, bf16=False, tag=None):
    gv, gl, ga = routed(t, bf16)
    ogv, ogl, oga = oracle(t, bf16)
    errs = (rel_err(gv, ogv), rel_err(gl, ogl), rel_err(ga, oga))
    print("rel_err grad_value / grad_loc / grad_aw:", errs, tag)
    assert errs[0] < (TG_BF16_GV if bf16 else TG) and errs[1] < TG and errs[2] < TG, (errs, tag)
    return (gv, gl, ga), (ogv, ogl, oga)


def on_every_pixel(t, H, W_, level=0):
    """place by hand: point 0 of query r * W + c has pixel (r, c) of `level` under its upper-left corner (fractions 0.3), point 1 has
    it under its lower-right corner -- every cell of every tile's base grid gets a point, the last one included"""
    n = min(t["loc"].shape[1], H * W_)
    r, c = torch.arange(n) // W_, torch.arange(n) % W_
    for p, d in ((0, 0.8), (1, -0.2)):      # h_im = r + 0.3 / r - 0.7  <=>  y = (h_im + 0.5) / H
        t["loc"][:, :n, :, level, p, 0] = ((c + d) / W_)[None, :, None]
        t["loc"][:, :n, :, level, p, 1] = ((r + d) / H)[None, :, None]


# ---- grid-limit edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [
    (13, 21),      # grid 14 x 22 = 308 pixels: one tile, between the old limit (256) and the new one
    (11, 25),      # grid 12 x 26 = 312: exactly the limit
    (14, 21),      # one row more than the limit allows (15 x 22 = 330): must split
    (12, 25),      # likewise (13 x 26 = 338)
    (1, 1),
    (30, 9),       # a grid side of 31: the widest the route pass's tables hold
    (31, 9),       # ... and one more: must split
])
def test_grid_limit_edges(shape):
    H, W_ = shape
    assert ((H + 1) * (W_ + 1) <= GRID) == (shape in [(13, 21), (11, 25), (1, 1), (30, 9)])
    t = make([shape], Lq=max(H * W_, 40), P=4, seed=H * 100 + W_)
    on_every_pixel(t, H, W_)
    check(t, tag=shape)


def test_nine_bit_base_index():
    """13 x 21, one tile: the base pixels of its last grid row / column have indices up to 307 (> 255).  A point by hand on the
    bottom-right pixel (only its upper-left corner is inside the map) and one a pixel further in (all four corners inside): the four
    corners' grad_value rows and the points' grad_loc / grad_aw, element by element."""
    H, W_ = 13, 21
    t = make([(H, W_)], Lq=8, P=4, seed=5)
    t["loc"][:] = 0.25      # everybody else far away, on base index (3 + 1) * 22 + 5
    t["loc"][0, 0, :, 0, 0] = torch.tensor([(W_ - 1 + 0.3 + 0.5) / W_, (H - 1 + 0.3 + 0.5) / H])      # base index 13 * 22 + 21 = 307
    t["loc"][0, 1, :, 0, 2] = torch.tensor([(W_ - 2 + 0.6 + 0.5) / W_, (H - 2 + 0.7 + 0.5) / H])      # base index 12 * 22 + 20 = 284
    (gv, gl, ga), (ogv, ogl, oga) = check(t)
    scale = np.abs(ogv).max()
    for r, c in ((H - 1, W_ - 1), (H - 2, W_ - 2), (H - 2, W_ - 1), (H - 1, W_ - 2)):
        got, want = gv[0, r * W_ + c].cpu().numpy(), ogv[0, r * W_ + c]
        assert np.abs(want).max() > 1e-3 * scale, "the probe must reach this corner"
        assert np.abs(got - want).max() < TG * scale, (r, c)
    for q, p in ((0, 0), (1, 2)):
        assert np.abs(gl[0, q, :, 0, p].cpu().numpy() - ogl[0, q, :, 0, p]).max() < TG * np.abs(ogl).max()
        assert np.abs(ga[0, q, :, 0, p].cpu().numpy() - oga[0, q, :, 0, p]).max() < TG * np.abs(oga).max()
        assert np.abs(oga[0, q, :, 0, p]).max() > 0


# ---- chunk edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_edges(records):
    """one level, one tile (8 x 8), P = 1: every (image, head) bin holds exactly Lq records"""
    t = make([(8, 8)], Lq=records, P=1, seed=records)
    check(t, tag=records)


# ---- planning over several levels, other instances -------------------------------------------------------------------------------
SHRUNK_E = [(20, 34), (10, 17), (5, 9), (3, 5)]      # tiles, slabs and apron atomics all occur


@pytest.fixture(scope="module")
def shrunk_e():
    S = sum(h * w for h, w in SHRUNK_E)
    t = make(SHRUNK_E, Lq=S, P=4, N=2, seed=21)
    on_every_pixel(t, 20, 34)
    return t, oracle(t)


def test_multi_level_planning(shrunk_e):
    t, (ogv, ogl, oga) = shrunk_e
    gv, gl, ga = routed(t)
    errs = (rel_err(gv, ogv), rel_err(gl, ogl), rel_err(ga, oga))
    print("rel_err:", errs)
    assert max(errs) < TG, errs


def test_arrival_order_with_poisoned_outputs(shrunk_e):
    """the gradient stage reads a chunk's records from the pool a second time: every element of grad_sampling_loc / grad_attn_weight is
    written (NaN-filled caller buffers, C ABI) and is the oracle's -- a record re-read from the wrong place would write another point's"""
    t, (ogv, ogl, oga) = shrunk_e
    lib = _lib.load()
    c = {k: v.cuda() for k, v in t.items()}
    N, Lq, L, P = c["loc"].shape[0], c["loc"].shape[1], len(SHRUNK_E), 4
    S = c["value"].shape[1]
    sh, ls = t["shapes"].numpy(), t["lsi"].numpy()
    gv, gl, ga = (torch.full_like(c[k], float("nan")) for k in ("value", "loc", "aw"))
    _lib.set_option("bwd_variant", 4)
    _lib.profile_enable(8)
    _lib.check(lib.msda_backward_f32(c["value"].data_ptr(), c["shapes"].data_ptr(), c["lsi"].data_ptr(), c["loc"].data_ptr(),
                                     c["aw"].data_ptr(), c["grad_out"].data_ptr(), N, S, M, D, L, Lq, P, 64, gv.data_ptr(),
                                     gl.data_ptr(), ga.data_ptr(), sh.ctypes.data, ls.ctypes.data,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ran = [(r["kind"], r["variant"]) for r in _lib.profile_collect()]
    _lib.profile_enable(0)
    assert ran == [("bwd", 4)], ran
    for a in (gv, gl, ga):
        assert torch.isfinite(a).all()
    errs = (rel_err(gv, ogv), rel_err(gl, ogl), rel_err(ga, oga))
    print("rel_err:", errs)
    assert max(errs) < TG, errs


def test_generic_route_instance_p3():
    S = sum(h * w for h, w in SHRUNK_E[:3])
    check(make(SHRUNK_E[:3], Lq=S, P=3, N=2, seed=33))


def test_samples_outside_the_map():
    """a third of the samples fall outside: the reference drops them, their gradients are zero (and written)"""
    t = make(SHRUNK_E, Lq=700, P=4, seed=44, spread=1.5)
    (gv, gl, ga), (ogv, ogl, oga) = check(t)
    dropped = (ogl == 0).all(-1) & (oga == 0)
    assert dropped.mean() > 0.1
    assert (gl.cpu().numpy()[dropped] == 0).all() and (ga.cpu().numpy()[dropped] == 0).all()


def test_bf16_storage():
    S = sum(h * w for h, w in SHRUNK_E)
    t = make(SHRUNK_E, Lq=S, P=4, seed=55)
    on_every_pixel(t, 20, 34)
    check(t, bf16=True)
