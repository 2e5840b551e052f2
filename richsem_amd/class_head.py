"""The CLIP-text class head with its gradient: the logits of ``CLIPAlign.forward`` / ``forward_hs`` from the 256-wide rows.

Reference: models/richsem/richsem.py:182-205 in its shipped configuration (``dino_visual_proj`` = bias-free ``nn.Linear(256, 1024)``,
frozen text side and ``logit_scale``): ``f = Wp x; logits_c = exp(logit_scale) (f / |f|) . (t_c / |t_c|)``.  :class:`ClassHead` computes
them from the collapsed operands of :mod:`richsem_amd.two_stage` -- ``G = T^ Wp``, ``A = Wp^T Wp`` -- with three MFMA kernels
(csrc/cls_head_mfma.hip; C ABI ``msda_cls_head_*``): the forward writes the fp32 logits and ``n2 = x . (A x)``, the backward the gradient
of the rows and ``[dG; dA]``, from which ``dWp = T^^T dG + Wp (dA + dA^T)`` follows by two small fp32 products here.  The 1024-wide
feature is never written and autograd keeps ``x``, the logits and one float per row.
"""
import ctypes

import torch

from . import _lib
from .param_cache import VersionCache


def _stream(dev):
    return _lib.raw_stream(dev)


def collapsed_operands(proj_weight, text_embed):
    """-> (G, A, t_hat): G = T^ Wp (classes, 256) and A = Wp^T Wp (256, 256), formed in fp64 and rounded once to fp32 exactly as
    ``ClassScorer._pack`` (richsem_amd/two_stage.py) forms them, and the normalised text side T^ (classes, proj) in fp32, which the weight
    gradient needs"""
    dev = proj_weight.device
    wp = proj_weight.detach().double()
    te = text_embed.detach().to(dev).double()
    te = te / te.norm(dim=-1, keepdim=True)                           # richsem.py:180
    G = (te @ wp).float().contiguous()                                # (classes, 256): t^_c . (Wp x) = (G x)_c
    A = (wp.t() @ wp).float().contiguous()                            # (256, 256):  |Wp x|^2 = x . (A x)
    return G, A, te.float().contiguous()


def _forward(x, packed, classes, scale, parts):
    """x (R, 256) contiguous -> (logits (R, classes), n2 (R)) fp32"""
    R = x.shape[0]
    logits = torch.empty(R, classes, dtype=torch.float32, device=x.device)
    n2 = torch.empty(R, dtype=torch.float32, device=x.device)
    if R:
        with _lib.on_device(x.device):
            _lib.check(_lib.load().msda_cls_head_forward(x.data_ptr(), int(x.dtype == torch.bfloat16), packed.data_ptr(), R, 256, classes,
                                                         scale, parts, logits.data_ptr(), n2.data_ptr(), _stream(x.device)))
    return logits, n2


def _backward_rows(g, logits, n2, x, packed, classes, scale, parts):
    """-> (dx (R, 256) in x's dtype, beta (R) fp32 = sum_c g_c logits_c)"""
    R = x.shape[0]
    dx = torch.empty_like(x)
    beta = torch.empty(R, dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_cls_head_backward_rows(g.data_ptr(), logits.data_ptr(), n2.data_ptr(), x.data_ptr(),
                                                           int(x.dtype == torch.bfloat16), packed.data_ptr(), R, 256, classes, scale, parts,
                                                           dx.data_ptr(), beta.data_ptr(), _stream(x.device)))
    return dx, beta


def workspace_bytes(rows, classes):
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_cls_head_workspace_bytes(rows, classes, ctypes.byref(n)))
    return n.value


def _backward_weights(g, n2, beta, x, classes, scale, parts):
    """-> [dG; dA] (classes + 256, 256) fp32: the splits over the rows added in a fixed order (the same bits on every run)"""
    R = x.shape[0]
    ws = torch.empty(workspace_bytes(R, classes) // 4, dtype=torch.float32, device=x.device)
    dGA = torch.empty(classes + 256, 256, dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_cls_head_backward_weights(g.data_ptr(), n2.data_ptr(), beta.data_ptr(), x.data_ptr(),
                                                              int(x.dtype == torch.bfloat16), R, 256, classes, scale, parts, ws.data_ptr(),
                                                              dGA.data_ptr(), _stream(x.device)))
    return dGA


class _HeadFunction(torch.autograd.Function):
    """(x (R, 256), proj_weight, head) -> logits (R, classes); gradients for x and proj_weight"""

    @staticmethod
    def forward(ctx, x, proj_weight, head, operand):
        packed, t_hat = operand
        logits, n2 = _forward(x, packed, head.classes, head.scale, head.parts)
        ctx.save_for_backward(x, logits, n2, packed, t_hat, proj_weight)
        ctx.head = head
        return logits

    @staticmethod
    def backward(ctx, g):
        x, logits, n2, packed, t_hat, proj_weight = ctx.saved_tensors
        head = ctx.head
        if x.shape[0] == 0:
            return torch.zeros_like(x), torch.zeros_like(proj_weight), None, None
        g = g.contiguous().float()
        dx, beta = _backward_rows(g, logits, n2, x, packed, head.classes, head.scale, head.parts)
        dwp = None
        if ctx.needs_input_grad[1]:
            dGA = _backward_weights(g, n2, beta, x, head.classes, head.scale, head.parts)
            dG, dA = dGA[:head.classes], dGA[head.classes:]
            wp = proj_weight.detach().float()
            dwp = (t_hat.t() @ dG + wp @ (dA + dA.t())).to(proj_weight.dtype)
        return (dx if ctx.needs_input_grad[0] else None), dwp, None, None


class ClassHead:
    """``prepare`` once, ``head(x)`` per forward: x (..., 256) float32 or bfloat16 on the GPU -> logits (..., classes) float32, with
    gradients for ``x`` and for ``proj_weight``.

    proj_weight (proj_dim, 256) = ``class_embed.dino_visual_proj.weight``; text_embed (classes, proj_dim) as stored; logit_scale = the CLIP
    parameter (frozen: read once).  ``parts`` = 2: operands as bf16 hi + lo parts (fp32-level logits and gradients from fp32 rows); 1: plain
    bf16 products.  The packed operand is kept in a VersionCache keyed on the projection: it follows optimizer steps and
    ``load_state_dict`` and is rebuilt inside a graph capture."""

    def __init__(self, parts=2):
        assert parts in (1, 2)
        self.parts = parts
        self._src = None
        self._cache = VersionCache()
        self.classes = 0
        self.scale = 1.0

    @torch.no_grad()
    def prepare(self, proj_weight, text_embed, logit_scale, parts=None):
        if not proj_weight.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        assert proj_weight.dim() == 2 and proj_weight.shape[1] == 256, "the rows must be 256 wide"
        assert text_embed.dim() == 2 and text_embed.shape[1] == proj_weight.shape[0]
        if parts is not None:
            assert parts in (1, 2)
            self.parts = parts
        self.classes = text_embed.shape[0]
        self.scale = float(torch.as_tensor(logit_scale).detach().double().exp())      # richsem.py:181
        self._src = (proj_weight, text_embed)
        self._cache.clear()
        self.packed      # (built now: a bad operand raises here)
        return self

    @property
    def packed(self):
        """(the kernels' operand, T^ fp32) from the current projection / text embeddings (None before :meth:`prepare`)"""
        if self._src is None:
            return None
        return self._cache.get(self._src, lambda: self._pack(*self._src))

    def _pack(self, proj_weight, text_embed):
        dev = proj_weight.device
        G, A, t_hat = collapsed_operands(proj_weight, text_embed)
        L = _lib.load()
        n = ctypes.c_int64(0)
        _lib.check(L.msda_cls_head_packed_elems(self.classes, ctypes.byref(n)))
        packed = torch.empty(n.value, dtype=torch.int16, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.msda_cls_head_pack(G.data_ptr(), self.classes, A.data_ptr(), 256, packed.data_ptr(), _stream(dev)))
        return packed, t_hat

    def __call__(self, x, packed=None):
        """``packed``: what :attr:`packed` returned earlier in the SAME forward (a caller with several call sites fetches it once: inside a
        capture every fetch builds the operand anew)"""
        if self._src is None:
            raise RuntimeError("ClassHead.prepare has not been called")
        if not x.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f"ClassHead: float32 / bfloat16 rows, got {x.dtype}")
        assert x.shape[-1] == 256
        rows = x.contiguous().view(-1, 256)
        return _HeadFunction.apply(rows, self._src[0], self, packed if packed is not None else self.packed).view(*x.shape[:-1], self.classes)
