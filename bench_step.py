"""A composed RichSem training step on richsem_amd's rows, for bench.py's ``full_step`` line.

NOT a model framework: the tier this repository is built to covers the operator and the rows around it, not RichSem's model assembly
(out of scope).  This file chains those rows the way the reference chains them --
``engine.py:44-114`` -> ``models/richsem/richsem.py:581-774`` -> ``deformable_transformer.py:273-463`` -- at the tensor sizes of
BASELINE.json configs[1] (2 x 800 x 1333 images padded to 1344, R50 4-scale, 900 queries + denoising groups of 12 boxes, 1204 classes,
frozen CLIP-RN50 teacher), with synthetic seeded weights and a compact criterion (the reference's SetCriterion stays host Python by
``north_star``; what is here reproduces its tensor work: Hungarian matching of 6 decoder outputs + the two-stage output, sigmoid focal
classification loss, L1 + GIoU box losses on the matched pairs and on the denoising queries, KL distillation against the teacher's
box logits), so that ONE number covers a whole forward + backward of the path:

    ResNet-50 (layer2-4 trained) -> input projections -> 6 encoder layers -> two-stage class score + top-900 -> denoising layout ->
    6 decoder layers (+ box refinement) -> class / box / distillation heads -> frozen teacher -> ROIAlign -> attention pool ->
    matcher -> losses -> backward through all of it.

bf16 activations wherever the library has a bf16 path (backbone, encoder, decoder), fp32 master parameters.  The timed step of ``run``,
``run_graphed``, ``run_graphed_device`` and ``run_ddp`` ends with gradient clipping and the AdamW step (reference engine.py:105-113); only
``run``'s ``graph_replay`` diagnostic is forward + backward alone.  The data pipeline is not part of it (nor of this repository's scope).
Layout: ``SECTIONS`` under one driver, one ``TrainLoop``, the command line through ``cli_kwargs``.
"""
import contextlib
import functools
import inspect
import math
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

from richsem_amd import workload as W
from richsem_amd.backbone import InputProjection, ResNet50
from richsem_amd.capture import capture, capture_stream, graphed_callables, pin_grad_accumulators      # noqa: F401  (bench_step.pin_grad_accumulators: its old home)
from richsem_amd.clip_resnet import ModifiedResNetTeacher
from richsem_amd.dn import denoising_queries, dn_buffers, prepare_dn_layout
from richsem_amd.distill import DistillKL
from richsem_amd.geometry import batch_geometry, sizes_from_targets
from richsem_amd.fed_loss import FedClassSampler, MaskedFocalNegativeSum, class_weights_from_image_counts
from richsem_amd.functions.linear import Lin256Function, VersionCache, pack_linear256
from richsem_amd.matcher import (BoxPairLoss, CostPlan, FocalNegativeSum, FocalPositiveSum, HungarianMatcher, LateStatus,
                                 pairs_from_query_of_target)
from richsem_amd.optim import ClipAdamW
from richsem_amd.repack import RepackPlan
from richsem_amd.modules import (MLP, refine_boxes, DeformableTransformerDecoderLayer, DeformableTransformerEncoderLayer, TransformerDecoder,
                                 clip_box_targets, get_reference_points, inverse_sigmoid)
from richsem_amd.two_stage import ClassScorer

NUM_CLASSES, NUM_QUERIES, DN_NUMBER, PROJ = 1204, 900, 100, 1024
# the model part in order: section ``name`` is the method ``Step.<name>_section`` (four bare names are sub-modules, so state dict keys)
SECTIONS = ("backbone", "input_proj", "encoder", "two_stage", "dn", "decoder", "heads")


# ---- small helpers of the reference, restated (host-side torch ops) -----------------------------------------------------------------
def box_cxcywh_to_xyxy(x):
    cx, cy, w, h = x.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou_pairs(a, b):
    """generalised IoU of matched pairs (util/box_ops.py:41-64 on the diagonal), xyxy boxes"""
    area = lambda t: (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    lt, rb = torch.max(a[:, :2], b[:, :2]), torch.min(a[:, 2:], b[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]                 # (not .prod(-1): its backward reads a zero count back to the host)
    union = area(a) + area(b) - inter
    iou = inter / (union + 1e-6)
    hw = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
    hull = hw[:, 0] * hw[:, 1]
    return iou - (hull - union) / (hull + 1e-6)


def sine_position(mask, num_pos_feats=128, temperature=20.0):
    """PositionEmbeddingSineHW (models/richsem/position_encoding.py:46-92, temperatureH = temperatureW = 20, normalize): (N, H, W) bool
    padding mask -> (N, H * W, 256)"""
    not_mask = ~mask
    y_embed, x_embed = not_mask.cumsum(1, dtype=torch.float32), not_mask.cumsum(2, dtype=torch.float32)
    eps, scale = 1e-6, 2 * math.pi
    y_embed = y_embed / (y_embed[:, -1:, :] + eps) * scale
    x_embed = x_embed / (x_embed[:, :, -1:] + eps) * scale
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=mask.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    px, py = x_embed[:, :, :, None] / dim_t, y_embed[:, :, :, None] / dim_t
    px = torch.stack((px[:, :, :, 0::2].sin(), px[:, :, :, 1::2].cos()), dim=4).flatten(3)
    py = torch.stack((py[:, :, :, 0::2].sin(), py[:, :, :, 1::2].cos()), dim=4).flatten(3)
    return torch.cat((py, px), dim=3).flatten(1, 2)


def encoder_output_proposals(memory_padding_mask, shapes):
    """models/richsem/utils.py:10-65, the part that depends on the batch's geometry only: per-pixel anchor boxes (unsigmoided, +inf at
    padded / out-of-range positions) and the (N, S, 1) mask of the positions whose memory is zeroed"""
    N, dev = memory_padding_mask.shape[0], memory_padding_mask.device
    proposals, cur = [], 0
    for lvl, (H_, W_) in enumerate(shapes):
        m = memory_padding_mask[:, cur:cur + H_ * W_].view(N, H_, W_, 1)
        valid_H, valid_W = (~m[:, :, 0, 0]).sum(1), (~m[:, 0, :, 0]).sum(1)
        gy, gx = torch.meshgrid(torch.linspace(0, H_ - 1, H_, dtype=torch.float32, device=dev),
                                torch.linspace(0, W_ - 1, W_, dtype=torch.float32, device=dev), indexing="ij")
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.cat([valid_W.unsqueeze(-1), valid_H.unsqueeze(-1)], 1).view(N, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(N, -1, -1, -1) + 0.5) / scale
        wh = torch.ones_like(grid) * 0.05 * (2.0 ** lvl)
        proposals.append(torch.cat((grid, wh), -1).view(N, -1, 4))
        cur += H_ * W_
    out = torch.cat(proposals, 1)
    valid = ((out > 0.01) & (out < 0.99)).all(-1, keepdim=True)
    out = torch.log(out / (1 - out))
    zeroed = memory_padding_mask.unsqueeze(-1) | ~valid
    return out.masked_fill(zeroed, float("inf")), zeroed


class Step(nn.Module):
    """the rows with their (synthetic) parameters; ``forward`` = model forward + criterion, returns the loss and section times"""

    def __init__(self, n_img=2, height=800, width=1333, boxes_per_image=12, seed=0, dev="cuda", fed_loss=False, fed_num_sample_cats=50,
                 class_image_counts=None, device_matcher=False, keep_match_outputs=False, device_distill=False, device_geometry=False, device_dn=False):
        super().__init__()
        torch.manual_seed(seed)
        self.n_img, self.H, self.Wimg, self.K = n_img, height, width, boxes_per_image
        self.Wpad = (width + 31) // 32 * 32
        self.backbone = ResNet50()
        self.backbone.load_state_dict(W.resnet50_state_dict(seed=seed + 1))
        self.input_proj = InputProjection()
        enc = DeformableTransformerEncoderLayer(256, 2048, dropout=0.0, n_levels=4, n_heads=8, n_points=4)
        self.encoder = nn.ModuleList([enc] + [type(enc)(256, 2048, dropout=0.0, n_levels=4, n_heads=8, n_points=4) for _ in range(5)])
        self.level_embed = nn.Parameter(torch.randn(4, 256))
        self.enc_output, self.enc_output_norm = nn.Linear(256, 256), nn.LayerNorm(256)
        self.enc_out_bbox_embed = MLP(256, 256, 4, 3)
        self.tgt_embed = nn.Embedding(NUM_QUERIES, 256)
        self.label_enc = nn.Embedding(NUM_CLASSES + 1, 256)
        dec = DeformableTransformerDecoderLayer(256, 2048, dropout=0.0, n_levels=4, n_heads=8, n_points=4)
        self.decoder = TransformerDecoder(dec, 6, nn.LayerNorm(256), d_model=256)
        self.decoder.bbox_embed = nn.ModuleList([MLP(256, 256, 4, 3) for _ in range(6)])
        # the CLIP-space classifier (richsem.py:38-205): visual projection (trained), distillation projection (trained), frozen text side
        self.dino_visual_proj = nn.Linear(256, PROJ, bias=False)
        self.proj_dino_hs = nn.Linear(256, PROJ)
        self.register_buffer("text_embed", torch.randn(NUM_CLASSES, PROJ))
        self.register_buffer("logit_scale", torch.tensor(math.log(1 / 0.07)))
        for m in list(self.encoder) + list(self.decoder.layers):
            att = m.self_attn if hasattr(m.self_attn, "sampling_offsets") else m.cross_attn
            with torch.no_grad():
                att.sampling_offsets.weight.normal_(0, 0.01)
                att.attention_weights.weight.normal_(0, 0.05)
        self.to(dev)
        self.teacher = ModifiedResNetTeacher(W.clip_rn50_state_dict(seed=seed + 2), heads=32)      # frozen: not a sub-module
        self.matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
        self.scorer = ClassScorer(2)
        self._eo_pack = VersionCache()
        self.timing = True
        self.stop_at = None       # (tools/capture_probe.py: end the step after this section with a surrogate loss)
        # bfloat16: the library's bf16 rows (the step bench.py times).  float32: the SAME parameters through the reference's op sequence in
        # fp32 from the input projections on (PyTorch ops around the operator's fp32 entry points; the backbone stays on the bf16
        # convolution kernels, its output is cast) -- the yardstick of tests/test_gpu_step.py
        self.act_dtype = torch.bfloat16
        # the federated loss (reference use_fed_loss / fed_num_sample_cats, richsem.py:956-961): opt-in, see loss_part.  Without
        # class_image_counts the class weights come from synthetic_image_counts() -- a made-up long tail, NOT LVIS's counts
        self.fed_loss = bool(fed_loss)
        self.fed_sampler = None
        if self.fed_loss:
            counts = synthetic_image_counts(NUM_CLASSES) if class_image_counts is None else class_image_counts
            self.fed_sampler = FedClassSampler(fed_num_sample_cats, class_weights_from_image_counts(counts, NUM_CLASSES))
        self.last_fed_mask = None
        # the distillation term as one row kernel (richsem_amd/distill.py) instead of gathers + softmaxes + kl_div: opt-in, see loss_part
        self.device_distill = bool(device_distill)
        # the Hungarian assignment on the device (msda_lsap_*, richsem_amd/matcher.py) instead of scipy on the host: opt-in.  The step then
        # has no host wait between its first and last kernel and captures whole (run_graphed(device_matcher=True)); the solver's status is
        # read one step late (matcher.LateStatus), the way AsyncLossLog reads the losses
        self.device_matcher = bool(device_matcher)
        self.cost_plan = None
        self.late_status = LateStatus()
        self.last_qot = self.last_status = None
        self.keep_match_outputs = bool(keep_match_outputs)      # (tests: the logits / boxes the solver saw stay referenced as last_match_outputs)
        self.last_match_outputs = None
        # the batch's geometry tensors (level masks, valid ratios, reference points, sine position, anchors) from ONE kernel inside the step
        # (richsem_amd/geometry.py) instead of torch ops in prepare(): opt-in.  They are then part of every captured form of the step and
        # follow the static ``sizes`` tensor at each replay, instead of staying those of the batch the graph was captured on
        self.device_geometry = bool(device_geometry)
        self.sizes = self._geometry = self.last_geometry = None      # (N, 2) int32 (h, w); the static buffers; the dict of the last forward
        # the denoising queries -- label / box noise, label embedding, padded query block, mask -- from ONE kernel that reads the target
        # counts on the device (richsem_amd/dn.py denoising_queries) instead of ~25 torch ops on the host's layout: opt-in.  The buffers
        # have the exact capacity of the batch prepare() saw (the criterion still indexes the layout on the host)
        self.device_dn = bool(device_dn)
        self._dn = self.last_dn = None      # the static inputs / buffers; what the last forward's denoising part produced (tests)

    # synthetic LVIS-shaped batch
    def batch(self, seed=0):
        g = torch.Generator().manual_seed(42 + seed)
        N, dev = self.n_img, self.level_embed.device
        images = torch.zeros(N, 3, self.H, self.Wpad)
        images[..., :self.Wimg] = torch.randn(N, 3, self.H, self.Wimg, generator=g)
        mask = torch.zeros(N, self.H, self.Wpad, dtype=torch.bool)
        mask[..., self.Wimg:] = True
        targets = []
        for _ in range(N):
            cxcy, wh = torch.rand(self.K, 2, generator=g) * 0.6 + 0.2, torch.rand(self.K, 2, generator=g) * 0.35 + 0.05
            targets.append({"boxes": torch.cat((cxcy, wh), 1).to(dev), "labels": torch.randint(1, 1204, (self.K,), generator=g).to(dev),
                            "size": torch.tensor([float(self.H), float(self.Wimg)], device=dev)})
        return images.to(dev), mask.to(dev), targets

    def _mark(self, name):
        if self.timing:       # (timing events cannot be recorded while the stream is being captured)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._events.append((name, ev))

    def class_logits(self, hs):
        return self.text_logits(F.linear(hs, self.dino_visual_proj.weight.to(hs.dtype)))

    def text_logits(self, f):
        """scaled cosine of ``f`` against the frozen text side (CLIPAlign.forward / forward_hs, richsem.py:182-205)"""
        f = f / f.norm(dim=-1, keepdim=True)
        t = self.text_embed / self.text_embed.norm(dim=-1, keepdim=True)
        return (self.logit_scale.exp() * (f @ t.to(f.dtype).t())).float()

    @torch.no_grad()
    def prepare(self, mask, targets):
        """what depends on the batch's geometry only (level shapes, padding masks, valid ratios, encoder reference points, denoising
        layout) and the two-stage scorer's binding to the projection and the frozen text side: built once per batch shape -- a few small
        launches and host -> device copies a trainer repeats per step; kept out of the step so that it can be captured into a graph.
        With ``device_geometry`` only what the canvas and the targets fix is built here; the image sizes go into the static ``self.sizes``
        and ``forward`` derives the geometry from them on the device (``mask`` is then not read)"""
        dev = mask.device
        shapes = list(W.pyramid_shapes(self.H, self.Wpad))
        spatial = torch.tensor(shapes, dtype=torch.int64, device=dev)
        st = {"shapes": shapes, "spatial": spatial, "lsi": torch.cat((spatial.new_zeros(1), spatial.prod(1).cumsum(0)[:-1]))}
        if self.device_geometry:
            sizes = sizes_from_targets(targets, dev)
            if self.sizes is None or self.sizes.shape != sizes.shape:
                self.sizes, self._geometry = sizes, None
            else:
                self.sizes.copy_(sizes)
            if self._geometry is None:      # the buffers every forward writes again: allocated once
                self._geometry = batch_geometry(self.sizes, (self.H, self.Wpad), shapes)
        else:
            masks = [F.interpolate(mask[None].float(), size=s).to(torch.bool)[0] for s in shapes]
            st.update({"masks": masks, "mask_flat": torch.cat([m.flatten(1) for m in masks], 1),
                       "valid_ratios": torch.stack([torch.stack([(~m[:, 0, :]).sum(1) / m.shape[2], (~m[:, :, 0]).sum(1) / m.shape[1]], -1)
                                                    for m in masks], 1).float()})
            st["ref"] = get_reference_points(shapes, st["valid_ratios"], dev)
            st["pos_sine"] = torch.cat([sine_position(m) for m in masks], 1)                           # (N, S, 256): the masks' part of pos
            st["proposals"], st["zeroed"] = encoder_output_proposals(st["mask_flat"], shapes)
        level_of = torch.cat([torch.full((h * w,), l, dtype=torch.int64, device=dev) for l, (h, w) in enumerate(shapes)])
        st["level_onehot"] = F.one_hot(level_of, len(shapes)).float()      # (S, L): the level embedding as a product (its backward a 4-row GEMM, not 22 k serialised row adds)
        st["known_num"] = [len(t["labels"]) for t in targets]
        st["lay"] = prepare_dn_layout(st["known_num"], DN_NUMBER, NUM_QUERIES, use_cdn=True)
        if self.device_dn:      # (host -> device copies: here, not in the step)
            cum = torch.tensor([0] + list(torch.tensor(st["known_num"]).cumsum(0).tolist()), dtype=torch.int64, device=dev)
            self._dn = {"cum": cum, "labels": torch.cat([t["labels"] for t in targets]).to(torch.int64).contiguous(),
                        "boxes": torch.cat([t["boxes"] for t in targets]).float().contiguous(),
                        "out": dn_buffers(len(targets), st["lay"]["pad_size"], NUM_QUERIES, 256, dev)}
        st["scale"] = self.logit_scale.detach().clone()
        self.scorer.prepare(self.dino_visual_proj.weight, self.text_embed, self.logit_scale)      # (its operand follows the weight's updates)
        self.static = st
        self._targets = targets
        if self.device_matcher:      # (host -> device copies: here, not in the step)
            if max(st["known_num"]) > NUM_QUERIES:
                raise ValueError(f"device_matcher: an image with {max(st['known_num'])} targets against {NUM_QUERIES} queries")
            self.cost_plan = CostPlan(targets, dev, torch.float32)
        return st

    # ---- the sections: ``s`` is the state of ONE call (run_sections makes it); each returns the terms of its surrogate loss ------------
    def backbone_section(self, s):      # backbone (richsem.py:581-595)
        s.feats = self.backbone(s.images)
        return (s.feats,)

    def input_proj_section(self, s):      # input projections, sine part + level embedding of the position (:596-612)
        srcs, got_shapes = self.input_proj(s.feats, out_dtype=self.act_dtype)
        assert got_shapes == s.st["shapes"]
        s.src = torch.cat(srcs, 1)
        s.pos_flat = (s.geo["pos_sine"] + s.st["level_onehot"] @ self.level_embed).to(self.act_dtype)
        return s.src, s.pos_flat

    def encoder_section(self, s):      # encoder (deformable_transformer.py:319)
        s.memory = s.src
        for layer in self.encoder:
            s.memory = layer(s.memory, s.pos_flat, s.geo["ref"], s.st["spatial"], s.st["lsi"], s.geo["mask_flat"])
        return (s.memory,)

    def two_stage_section(self, s):
        """two-stage query selection (:352-380); ``s.topk``: the selection held fixed.  Its two outputs reach the loss past the decoder (the
        decoder's reference points are detached), so they stay in every later surrogate: ``s.carried``"""
        adt, geo, eo = self.act_dtype, s.geo, self.enc_output
        if adt == torch.bfloat16:
            pk = self._eo_pack.get((eo.weight, eo.bias), lambda: pack_linear256([eo.weight], [eo.bias]))
            output_memory = Lin256Function.apply(s.memory.masked_fill(geo["zeroed"], 0.0), pk, None, False, eo.weight, eo.bias)   # bf16, lin256
        else:
            output_memory = eo(s.memory.masked_fill(geo["zeroed"], 0.0))
        output_memory = F.layer_norm(output_memory, (256,), self.enc_output_norm.weight.to(adt), self.enc_output_norm.bias.to(adt),
                                     self.enc_output_norm.eps)
        if s.topk is None:
            s.topk = self.scorer.topk_proposals(output_memory, NUM_QUERIES)                            # no logit tensor (two_stage.py)
        self.last_topk = s.topk
        coord_unselected = self.enc_out_bbox_embed(output_memory).float() + geo["proposals"]
        s.refpoint_undetach = torch.gather(coord_unselected, 1, s.topk[..., None].expand(-1, -1, 4))
        tgt_undetach = torch.gather(output_memory, 1, s.topk[..., None].expand(-1, -1, 256)).float()
        s.carried = (self.class_logits(tgt_undetach), s.refpoint_undetach.sigmoid())      # the two-stage logits and boxes
        return ()

    def dn_section(self, s):      # denoising queries (dn_components.py:11-193): layout on the library's kernels, noise as torch ops
        N, dev, lay = s.images.shape[0], s.images.device, s.st["lay"]
        if self.device_dn:      # (one launch: noise, embedding, block and mask)
            q_label, q_bbox, s.tgt_mask = self._device_dn_queries(N, lay["pad_size"], dev)
        else:
            (q_label, q_bbox), s.tgt_mask = self._torch_dn_queries(N, lay["pad_size"], lay["num_dn_group"], s.targets, dev), lay["attn_mask"]
        s.tgt = torch.cat((q_label, self.tgt_embed.weight[None].expand(N, -1, -1)), 1)                 # embed_init_tgt
        s.refpoints = torch.cat((q_bbox, s.refpoint_undetach.detach()), 1)
        return s.tgt, s.refpoints

    def decoder_section(self, s):      # decoder (:427)
        s.hs, s.refs = self.decoder(tgt=s.tgt.transpose(0, 1).to(self.act_dtype), memory=s.memory.transpose(0, 1), tgt_mask=s.tgt_mask,
                                    memory_key_padding_mask=s.geo["mask_flat"], refpoints_unsigmoid=s.refpoints.transpose(0, 1),
                                    level_start_index=s.st["lsi"], spatial_shapes=s.st["spatial"], valid_ratios=s.geo["valid_ratios"])
        return s.hs, s.refs

    def heads_section(self, s):      # heads (richsem.py:705-733)
        hs, refs = s.hs, s.refs
        s.coords = torch.stack([refine_boxes(self.decoder.bbox_embed[l](hs[l]), refs[l]) for l in range(6)])      # richsem.py:705-715
        s.logits = self.class_logits(torch.stack(hs))                                 # (6, N, pad + 900, 256) -> (6, N, 1092, 1204)
        s.clip_logits = self.text_logits(F.linear(hs[-1], self.proj_dino_hs.weight.to(hs[-1].dtype), self.proj_dino_hs.bias.to(hs[-1].dtype)))
        return s.coords, s.logits, s.clip_logits      # (the last: (N, 1092, 1204))

    def run_sections(self, images, targets, topk=None):
        """the one driver: every section of ``SECTIONS`` on a fresh state, a timing mark after each -> (state, None); or, where ``stop_at``
        names a section, (state, its surrogate loss) with the later sections not run.  The surrogate sums the section's terms and the
        carried ones -- a list among them summed on its own first --, so its backward reaches all the work up to there"""
        self._events = []
        self._mark("start")
        s = SimpleNamespace(images=images, targets=targets, topk=topk, st=self.static, geo=self.static, carried=())
        if self.device_geometry:      # the step's first device work: the geometry of the batch whose sizes ``self.sizes`` holds NOW
            s.geo = self.last_geometry = batch_geometry(self.sizes, (self.H, self.Wpad), s.st["shapes"], out=self._geometry)
        for name in SECTIONS:
            terms = getattr(self, name + "_section")(s)
            self._mark(name)
            if self.stop_at == name:
                sums = [sum(x.float().sum() for x in t) if isinstance(t, (list, tuple)) else t.float().sum() for t in (*terms, *s.carried)]
                return s, sum(sums[1:], sums[0])
        return s, None

    def forward(self, images, mask, targets, indices=None, topk=None):
        """``model_part``, matcher, ``loss_part`` -> the loss (with ``stop_at``: the section's surrogate).  ``indices``: the matcher's
        assignment held fixed (graph capture, A/B tests); ``topk``: the two-stage selection held fixed"""
        out = self.model_part(images, mask, targets, topk=topk)
        if torch.is_tensor(out):
            return out
        # ---- matcher (matcher.py:30-78, one host copy for the 7 outputs) -------------------------------------------------------------------
        if indices is None:
            indices = (self.match_device if self.device_matcher else self.match)(*out[:4], targets)
        packed = indices if (isinstance(indices, tuple) and torch.is_tensor(indices[0])) else self.pack_indices(indices, targets)
        if packed is not indices:
            self.last_indices = indices
        self._mark("matcher")
        loss = self.loss_part(*out, *packed)
        self._mark("criterion")
        return loss

    def _torch_dn_queries(self, N, pad, groups, targets, dev):
        """the noise, the embedding and the scatter as torch ops on the host's layout (the default)"""
        lay = self.static["lay"]
        fz = self.frozen_noise      # (tests: the same draws in every step and in every form of the step -- see freeze_noise)
        labels, boxes = torch.cat([t["labels"] for t in targets]), torch.cat([t["boxes"] for t in targets])
        known_labels, known_boxes = labels.repeat(2 * groups), boxes.repeat(2 * groups, 1)
        p = torch.rand(known_labels.shape, device=dev) if fz is None else fz["p"]
        rnd_lab = torch.randint(0, NUM_CLASSES, known_labels.shape, device=dev) if fz is None else fz["labels"]
        noised = torch.where(p < 0.25, rnd_lab, known_labels)
        xyxy = box_cxcywh_to_xyxy(known_boxes)
        diff = torch.cat((known_boxes[:, 2:] / 2, known_boxes[:, 2:] / 2), 1)
        sign = (torch.randint(0, 2, xyxy.shape, device=dev).float() * 2 - 1) if fz is None else fz["sign"]
        rand_part = torch.rand(xyxy.shape, device=dev) if fz is None else fz["rand"]
        neg = (torch.arange(known_labels.numel(), device=dev) // labels.numel()) % 2 == 1
        rand_part = torch.where(neg[:, None], rand_part + 1.0, rand_part) * sign
        xyxy = (xyxy + rand_part * diff).clamp(0.0, 1.0)
        nb = torch.cat(((xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]), 1)
        q_label = torch.zeros(N, pad, 256, device=dev)
        q_bbox = torch.zeros(N, pad, 4, device=dev)
        q_label[lay["known_bid"], lay["map_known_indice"]] = self.label_enc(noised)
        q_bbox[lay["known_bid"], lay["map_known_indice"]] = inverse_sigmoid(nb)
        self.last_dn = {"noised_label": noised, "noised_box": nb}
        return q_label, q_bbox

    def _device_dn_queries(self, N, pad, dev):
        """the same from one launch that reads the counts on the device (richsem_amd/dn.py); fresh uniforms every step -- drawn here, so a
        replay of a captured step draws anew --, or the frozen draws in the kernel's encoding"""
        d, fz = self._dn, self.frozen_noise
        uniform = torch.rand((N, pad, 10), device=dev) if fz is None else fz["uniform"]
        q_label, q_bbox, tgt_mask, noised_label, meta = denoising_queries(
            d["cum"], d["labels"], d["boxes"], self.label_enc.weight, uniform, pad_cap=pad, num_queries=NUM_QUERIES, num_classes=NUM_CLASSES,
            dn_number=DN_NUMBER, label_noise_ratio=0.5, box_noise_scale=1.0, use_cdn=True, out=d["out"])
        self.last_dn = {"noised_label": noised_label, "noised_box": d["out"]["noised_box"], "meta": meta}
        return q_label, q_bbox, tgt_mask

    frozen_noise = None
    frozen_fed = None

    def freeze_noise(self, seed):
        """draw the denoising noise ONCE from ``seed`` and use it in every later step (a training step draws it anew each time,
        dn_components.py:72-110): eager, captured and graphed forms of the step can then be compared parameter by parameter"""
        st = self.static
        n = 2 * st["lay"]["num_dn_group"] * sum(st["known_num"])
        g = torch.Generator(device=self.level_embed.device).manual_seed(seed)
        dev = self.level_embed.device
        self.frozen_noise = {"p": torch.rand(n, device=dev, generator=g), "labels": torch.randint(0, NUM_CLASSES, (n,), device=dev, generator=g),
                             "sign": torch.randint(0, 2, (n, 4), device=dev, generator=g).float() * 2 - 1,
                             "rand": torch.rand((n, 4), device=dev, generator=g)}
        if self.device_dn:
            # the same draws as the kernel takes them: row g * total + cum[b] + j of the reference's order is slot (b, g * single_pad + j) --
            # the pair (known_bid, map_known_indice) --, sign -1 / +1 is 0.25 / 0.75 and class k is (k + 0.5) / num_classes, which floors back to k
            fz, lay = self.frozen_noise, st["lay"]
            u = torch.zeros((len(st["known_num"]), lay["pad_size"], 10), device=dev)
            rows = torch.cat((fz["p"][:, None], ((fz["labels"].float() + 0.5) / NUM_CLASSES)[:, None],
                              torch.where(fz["sign"] > 0, 0.75, 0.25).float(), fz["rand"]), 1)
            u[lay["known_bid"], lay["map_known_indice"]] = rows
            fz["uniform"] = u

    def fed_groups(self):
        """how many class draws a step of the federated loss makes: one per reference loss_labels call -- the matching part of every
        decoder layer, their denoising parts, the two-stage output"""
        return 2 * len(self.decoder.layers) + 1

    def freeze_fed(self, seed):
        """draw the federated loss's class masks ONCE from ``seed`` (for the batch ``prepare`` saw) and use them in every later step (a
        training step draws them anew each time): eager and graphed forms of the step can then be compared on the same draws"""
        dev = self.level_embed.device
        labels = torch.cat([t["labels"] for t in self._targets])
        g = torch.Generator(device=dev).manual_seed(seed)
        self.frozen_fed, _ = self.fed_sampler.sample(labels, self.fed_groups(), generator=g)

    def model_part(self, images, mask=None, targets=None, teacher=True, topk=None):
        """the step up to the matcher: -> (logits (6, N, Q, C), boxes (6, N, Q, 4), two-stage logits (N, 900, C), two-stage boxes
        (N, 900, 4), distillation logits (N, Q, C), the teacher's box logits (targets, C) -- unless ``teacher`` is False: ``run_graphed``
        launches the frozen teacher beside the host's matching): tensors in, tensors out, nothing read back to the host -- the part
        ``run_graphed`` captures.  ``topk``: the two-stage selection held fixed; ``mask`` is not read (``prepare`` was); with ``stop_at`` the
        section's surrogate loss, a scalar, instead"""
        targets = self._targets if targets is None else targets
        s, surrogate = self.run_sections(images, targets, topk)
        if surrogate is not None:
            return surrogate
        out = (s.logits, s.coords, *s.carried, s.clip_logits)
        if not teacher:
            return out
        # ---- frozen teacher -> ROIAlign -> attention pool -> text logits (richsem.py:614-629, :741-768) ----------------------------------
        t_logits = self.teacher_part(images, targets)
        self._mark("teacher")
        return out + (t_logits,)

    @torch.no_grad()
    def teacher_part(self, images, targets=None):
        """frozen CLIP-RN50 teacher -> ROIAlign -> attention pool -> text logits of the target boxes (richsem.py:614-629, :741-768): no
        gradient, no dependence on the student"""
        targets = self._targets if targets is None else targets
        _, fmap = self.teacher(images, ret_sp=True)
        _, t_logits = clip_box_targets(fmap, targets, self.teacher.attnpool, self.text_embed, self.static["scale"])
        return torch.cat(t_logits).float()

    def _match_outputs(self, logits, coords, il, ib):
        pad = self.static["lay"]["pad_size"]
        return [{"pred_logits": logits[l][:, pad:], "pred_boxes": coords[l][:, pad:]} for l in range(logits.shape[0])] + \
            [{"pred_logits": il, "pred_boxes": ib}]

    def match(self, logits, coords, il, ib, targets):
        return self.matcher.match_many(self._match_outputs(logits, coords, il, ib), targets)

    @torch.no_grad()
    def match_device(self, logits, coords, il, ib, targets):
        """the assignment of the 6 + 1 outputs solved on the device, as the packed tensors :meth:`pack_indices` builds from the host's: cost
        blocks -> ``msda_lsap_*`` -> index tensors, all enqueued, nothing read back (``last_qot`` (7, targets) / ``last_status`` (7, images)
        keep the solver's result; outside a capture the status goes to ``late_status``, which raises one step late)"""
        outs = [{"pred_logits": o["pred_logits"].float(), "pred_boxes": o["pred_boxes"].float()} for o in self._match_outputs(logits, coords, il, ib)]
        self.last_qot, self.last_status = self.matcher.match_many_device(outs, self.cost_plan)
        if self.keep_match_outputs:
            self.last_match_outputs = outs
        if not torch.cuda.is_current_stream_capturing():
            self.late_status.push(self.last_status)
        labels, boxes = torch.cat([t["labels"] for t in targets]), torch.cat([t["boxes"] for t in targets])
        return (labels, boxes) + pairs_from_query_of_target(self.last_qot, self.cost_plan, NUM_QUERIES)

    def match_begin(self, logits, coords, il, ib, targets):
        """the device half of :meth:`match` (cost blocks + copy to the host enqueued, nothing waits); :meth:`match_end` the host half"""
        return self.matcher.match_many_begin(self._match_outputs(logits, coords, il, ib), targets)

    def match_end(self, pending):
        return self.matcher.match_many_end(pending)

    def pack_indices(self, indices, targets):
        """the Hungarian assignment of the 6 + 1 outputs as flat device tensors of a size the batch fixes (every target is matched once per
        output): (labels, boxes) of all targets, (layer, image, query, target) of the decoder outputs' pairs, (image, query, target) of the
        two-stage output's and of the last layer's (the distillation pairs)"""
        dev = self.level_embed.device
        off = [0]
        for t in targets:
            off.append(off[-1] + len(t["labels"]))
        labels, boxes = torch.cat([t["labels"] for t in targets]), torch.cat([t["boxes"] for t in targets])

        def flat(idx_list):
            li = torch.cat([torch.full((len(s),), k, dtype=torch.int64) for k, idx in enumerate(idx_list) for s, _ in idx])
            bi = torch.cat([torch.full((len(s),), b, dtype=torch.int64) for idx in idx_list for b, (s, _) in enumerate(idx)])
            si = torch.cat([s.cpu() for idx in idx_list for s, _ in idx])
            tj = torch.cat([j.cpu() + off[b] for idx in idx_list for b, (_, j) in enumerate(idx)])
            return torch.stack((li, bi, si, tj)).to(dev, non_blocking=True)
        nl = len(indices) - 1
        return labels, boxes, flat(indices[:nl]), flat(indices[nl:]), flat(indices[nl - 1:nl])

    def loss_part(self, logits, coords, il, ib, clip_logits, t_logits, labels, boxes, m_dec, m_int, m_dis):
        """criterion (richsem.py:1124-1306, compact): the same per-output sums as the reference's loop over the 6 + 1 outputs -- sigmoid focal
        loss (over every query incl. the denoising part's negative slots, whose target is no-object), L1 + GIoU on the matched pairs and on
        the denoising queries' positive slots, KL distillation -- formed in ONE pass per kind over
        the stacked outputs: the all-negative focal term of a whole logit tensor is one kernel each way (matcher.FocalNegativeSum), and the
        positive entries / box pairs of the matched, two-stage and denoising parts are concatenated with a weight each (1 / num_boxes, or
        1 / (num_boxes x groups)) so that every loss formula runs once -- as one kernel each (matcher.FocalPositiveSum, matcher.BoxPairLoss:
        value and gradient in one launch; a loop over the outputs is ~40 small launches per output and kind).
        By default every class counts in the focal loss.  With ``fed_loss`` (the reference's use_fed_loss, richsem.py:956-961) each of the
        13 reference loss_labels calls -- the matching part of decoder layers 0-5, their denoising parts, the two-stage output, in that
        order -- takes it over a class subset of its own: the batch's target classes (what every one of those calls passes to
        get_fed_loss_inds: the Hungarian matching assigns every target, the denoising targets repeat the same labels) topped up to
        fed_num_sample_cats by weighted draws without replacement, drawn afresh every step on the device (fed_loss.FedClassSampler, no host
        sync: the draw is captured and replayed with the rest) -- or the masks of ``freeze_fed``.  The all-negative term then runs
        with a class mask per row (fed_loss.MaskedFocalNegativeSum); the positive entries are appeared classes, always in the mask.
        The last masks are kept as ``last_fed_mask`` (13, C).  With ``device_distill`` the KL term is one ``distill.DistillKL`` call on the same
        rows (value and gradient rows from one kernel, the gather inside it) instead of two gathers, two softmaxes and ``kl_div``.
        Tensors in, the loss out."""
        st = self.static
        dev = logits.device
        lay = st["lay"]
        pad, groups, single = lay["pad_size"], lay["num_dn_group"], lay["single_pad"]
        num_boxes = float(max(sum(st["known_num"]), 1))
        nbx = num_boxes * groups
        nl, N, Q = logits.shape[0], logits.shape[1], logits.shape[2]
        alpha = 0.25
        cst = st.get("loss_static")
        if cst is None or cst["key"] != (nl, N, Q, pad, groups, single):      # index / weight tensors the batch's geometry fixes
            pos_slots = (torch.arange(groups, device=dev)[:, None] * 2 * single + torch.arange(single, device=dev)[None]).flatten()
            # (reference richsem.py:938-964: loss_labels of the denoising part runs the focal loss over ALL pad_size denoising queries --
            # the negative slots with the no-object target -- normalised by num_boxes x groups, :1180 / :1227; the matching part by num_boxes)
            w_q = torch.empty(Q, dtype=torch.float32, device=dev)
            w_q[:pad] = 1.0 / nbx
            w_q[pad:] = 1.0 / num_boxes
            n_dn = nl * N * pos_slots.numel()
            cst = {"key": (nl, N, Q, pad, groups, single), "pos_slots": pos_slots,
                   "w_rows": w_q[None, None, :].expand(nl, N, Q).contiguous(),
                   "w_int": torch.full(il.shape[:2], 1.0 / num_boxes, dtype=torch.float32, device=dev),
                   "dn_l": torch.arange(nl, device=dev)[:, None, None].expand(nl, N, pos_slots.numel()).reshape(-1),
                   "dn_n": torch.arange(N, device=dev)[None, :, None].expand(nl, N, pos_slots.numel()).reshape(-1),
                   "dn_q": pos_slots[None, None, :].expand(nl, N, -1).reshape(-1),
                   "w_dn": torch.full((n_dn,), 1.0 / nbx, dtype=torch.float32, device=dev)}
            if self.fed_loss:      # the class draw each row's focal term uses: layer l's matching part -> l, its denoising part -> nl + l; two-stage -> 2 nl
                g_q = torch.arange(nl, dtype=torch.int32, device=dev)[:, None, None].expand(nl, N, Q).clone()
                g_q[:, :, :pad] += nl
                cst["g_rows"] = g_q.contiguous()
                cst["g_int"] = torch.full(il.shape[:2], 2 * nl, dtype=torch.int32, device=dev)
            st["loss_static"] = cst
        # ---- classification: all-negative term of every entry, then what the positive entries contribute instead ------------------------
        if self.fed_loss:
            fed = self.frozen_fed if self.frozen_fed is not None else self.fed_sampler.sample(labels, 2 * nl + 1)[0]
            self.last_fed_mask = fed
            loss = MaskedFocalNegativeSum.apply(logits, cst["w_rows"], cst["g_rows"], fed, alpha) + \
                MaskedFocalNegativeSum.apply(il, cst["w_int"], cst["g_int"], fed, alpha)
        else:
            loss = FocalNegativeSum.apply(logits, cst["w_rows"], alpha) + FocalNegativeSum.apply(il, cst["w_int"], alpha)
        li, bi, si, tj = m_dec
        _, ibi, isi, itj = m_int
        dn_lab = labels.view(N, -1).repeat(1, groups)[None].expand(nl, -1, -1).reshape(-1)      # every image has `single` boxes here
        x_pos = torch.cat((logits[li, bi, si + pad, labels[tj]], il[ibi, isi, labels[itj]], logits[cst["dn_l"], cst["dn_n"], cst["dn_q"], dn_lab]))
        w_pair = torch.cat((torch.full((li.numel() + ibi.numel(),), 1.0 / num_boxes, dtype=torch.float32, device=dev), cst["w_dn"]))
        loss = loss + FocalPositiveSum.apply(x_pos, w_pair, alpha)
        # ---- boxes: L1 + GIoU of all pairs at once -------------------------------------------------------------------------------------------
        pb = torch.cat((coords[li, bi, si + pad], ib[ibi, isi], coords[cst["dn_l"], cst["dn_n"], cst["dn_q"]]))
        tb = torch.cat((boxes[tj], boxes[itj], boxes.view(N, -1, 4).repeat(1, groups, 1)[None].expand(nl, -1, -1, -1).reshape(-1, 4)))
        loss = loss + BoxPairLoss.apply(pb, tb, w_pair, 5.0, 2.0)
        # ---- distillation: KL of the matched queries' CLIP logits against the teacher's box logits (richsem.py:1255-1300) -------------------
        _, bi, si, tj = m_dis
        if self.device_distill:      # the same rows, each with the weight 0.5 / K ("batchmean" over K rows), gathered inside one kernel
            K = bi.numel()
            w_dis = cst.get("w_dis")
            if w_dis is None or w_dis.numel() != K:
                w_dis = cst["w_dis"] = torch.full((K,), 0.5 / max(K, 1), dtype=torch.float32, device=dev)
            return loss + DistillKL.apply(clip_logits, t_logits, bi * clip_logits.shape[1] + si + pad, tj, w_dis, None, None, False)
        loss = loss + 0.5 * F.kl_div(F.log_softmax(clip_logits[bi, si + pad], -1), F.softmax(t_logits[tj], -1), reduction="batchmean")
        return loss

    def section_ms(self):
        """ms per forward section of the last step (events recorded on the current stream)"""
        torch.cuda.synchronize()
        out, prev = {}, self._events[0][1]
        for name, ev in self._events[1:]:
            out[name] = prev.elapsed_time(ev)
            prev = ev
        return out


def synthetic_image_counts(C, seed=1203):
    """a fixed, seeded, SYNTHETIC long-tail table of per-class image counts for the federated loss's weights when no dataset's counts are
    given -- made up, not LVIS's: class 0 gets 0 (LVIS has no category 0), classes 1..C-1 a random order of 1 + 10000 / rank"""
    g = torch.Generator().manual_seed(seed)
    rank = torch.randperm(C - 1, generator=g) + 1
    return torch.cat((torch.zeros(1, dtype=torch.int64), 1 + 10000 // rank))


CLIP_MAX_NORM = 0.1      # reference config/RichSem/baseline_4scale.py:19 (clip_max_norm), engine.py:110-112
LR = 1e-4


def make_optimizer(params, lr=LR, library=False, fused=True):
    """AdamW as the reference builds it (main.py:213-214; lr / weight decay of config/RichSem/baseline_4scale.py:7,14), one fused launch per
    step (fused optimizers do not bump the parameters' version counters; richsem_amd/param_cache.py's step hook does, so the bf16 layers'
    packed weights follow every step).  ``library``: richsem_amd.optim.ClipAdamW instead -- gradient clipping and AdamW in two launches of
    the library's own (opt-in: ``--library-optimizer``).  ``fused=False``: torch's own choice of implementation (run_ddp on CPU tensors)"""
    kw = dict(lr=lr, weight_decay=1e-4)
    if library:
        return ClipAdamW(params, max_norm=CLIP_MAX_NORM, **kw)
    return torch.optim.AdamW(params, fused=fused or None, **kw)


def optimizer_step(opt, params):
    """what follows ``losses.backward()`` in the reference's training loop (engine.py:109-113): gradient clipping to clip_max_norm, AdamW step.
    No host synchronisation: the norm stays on the device (``error_if_nonfinite`` is off as in the reference's call).  The library's optimizer
    clips inside its own step."""
    if not isinstance(opt, ClipAdamW):      # (make_optimizer(library=True) clips inside its step)
        torch.nn.utils.clip_grad_norm_(params, CLIP_MAX_NORM, foreach=True)
    opt.step()


class GroupedRepack:
    """``--grouped-repack``: a richsem_amd.repack.RepackPlan recorded around the first eager forward + backward (``recording()``), then
    attached to the library's optimizer (``attach``: its step ends with the one refresh launch) or refreshed after any other optimizer's
    step (``after_step``).  The captured forms of the step then hold no pack launch; ``plan`` is None when the switch is off."""

    def __init__(self, on):
        self.plan = RepackPlan() if on else None
        self._recorded = self._attached = False

    def recording(self):
        if self.plan is None or self._recorded:
            return contextlib.nullcontext()
        self._recorded = True
        return self.plan.record()

    def attach(self, opt):
        if self.plan is not None and isinstance(opt, ClipAdamW):
            opt.attach_repack(self.plan)
            self._attached = True

    def after_step(self):
        if self.plan is not None and not self._attached:
            self.plan.refresh()


class TrainLoop:
    """The one training loop (reference engine.py:100-113) of ``run``, ``run_graphed`` and ``run_graphed_device``: clear the gradients, run
    the body, backward -- :meth:`forward_backward` --, then gradient clipping + optimizer step + the re-pack -- :meth:`update`; :meth:`step`
    is both.  ``opt`` is None where ``optimizer`` is False: ``update`` then does nothing.  (``run_ddp`` keeps a loop of its own: see there.)"""

    def __init__(self, model, repack, lr=LR, library=False, optimizer=True):
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.opt = make_optimizer(self.params, lr, library) if optimizer else None
        self.repack = repack
        repack.attach(self.opt)

    def forward_backward(self, body, fwd=None):      # ``fwd``: an event recorded between the two (``run`` times the backward from it)
        for p in self.params:
            p.grad = None
        loss = body()
        if fwd is not None:
            fwd.record()
        loss.backward()
        return loss

    def update(self):
        if self.opt is not None:
            optimizer_step(self.opt, self.params)
            self.repack.after_step()

    def step(self, body):
        loss = self.forward_backward(body)
        self.update()
        return loss


def _setup(n_img, dev, noise_seed, fed_seed, timing, **step_kwargs):
    """-> (model, images, mask, targets): a Step prepared for its batch, noise and federated draws frozen where a seed is given; ``timing``:
    whether its forward records section events (they cannot be recorded while a stream is captured)"""
    model = Step(n_img=n_img, dev=dev, **step_kwargs)
    model.timing = timing
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    model._mask = mask
    if noise_seed is not None:
        model.freeze_noise(noise_seed)
    if fed_seed is not None:
        model.freeze_fed(fed_seed)
    return model, images, mask, targets


def run(n_img, dev, steps=5, warmup=2, graph=True, stop_at=None, lr=LR, noise_seed=None, return_model=False, library=False,
        grouped_repack=False, **step_kwargs):
    """time `steps` composed steps (forward + loss + backward + optimizer step); returns the dict bench.py attaches as ``full_step``
    (tests: ``lr``, ``noise_seed`` (Step.freeze_noise), ``return_model`` -- the trained Step under "model", its plan under "repack" --,
    ``step_kwargs``: Step's keywords, a smaller Step for instance; ``library``: make_optimizer's switch, ``grouped_repack``:
    :class:`GroupedRepack`'s; all three passed on whole to run_graphed, so ``graphed_sections`` times the same Step)"""
    model, images, mask, targets = _setup(n_img, dev, noise_seed, None, True, **step_kwargs)
    model.stop_at = stop_at      # (profiling aid: the step cut off after a section, see tools/step_sections.sh)
    repack = GroupedRepack(grouped_repack)
    loop = TrainLoop(model, repack, lr, library)

    def step(indices=None, optimize=True):
        # what only this harness does: it records the event between forward and backward, and its captured form leaves the optimizer out
        fwd = torch.cuda.Event(enable_timing=True) if model.timing else None
        with repack.recording():      # (the first step only, and only with grouped_repack)
            loss = loop.forward_backward(lambda: model(images, mask, targets, indices), fwd)
        if optimize:
            loop.update()
        return loss, fwd

    rows, totals, bwds = {}, [], []
    with capture_stream() as side:      # warm-up, the timed eager steps and the captures below: ONE stream
        # the trained parameters are handed over here, all parameters in the graphed forms: pin_grad_accumulators skips the frozen ones
        pinned = pin_grad_accumulators(loop.params)      # noqa: F841  (kept alive to the end of run(): every graph below reuses these nodes)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss, fwd = step()
            b.record()
            torch.cuda.synchronize()
            totals.append(a.elapsed_time(b))
            bwds.append(fwd.elapsed_time(b))
            for k, v in model.section_ms().items():
                rows.setdefault(k, []).append(v)
    ms = sum(totals) / len(totals)
    out = {"what": "ONE composed training step on the library's rows at configs[1] sizes: ResNet-50 (layer2-4 trained) -> input projections "
                   "-> 6 encoder layers -> two-stage score + top-900 -> denoising layout -> 6 decoder layers -> heads -> frozen CLIP-RN50 "
                   "teacher -> ROIAlign -> attention pool -> matcher -> losses, forward + backward, gradient clipping (0.1) + fused AdamW step "
                   "(reference engine.py:105-113), bf16 activations / fp32 parameters; synthetic weights and batch; no data pipeline "
                   "(bench_step.py)",
           "ms": round(ms, 2), "img_per_s": round(n_img / (ms * 1e-3), 2), "loss": float(loss.detach()),
           "forward_rows_ms": {k: round(sum(v) / len(v), 3) for k, v in rows.items()},
           "backward_ms": round(sum(bwds) / len(bwds), 2)}
    if return_model:
        out.update(model=model, repack=repack.plan)
    if not graph:
        return out
    # the device part as a captured graph: the assignment of the last eager step held fixed (the matcher's host round trip cannot be captured)
    indices = model.pack_indices(model.last_indices, targets)      # (device tensors: no host <-> device copies in the capture)
    torch.cuda.synchronize()
    model.timing = False

    def replay_ms(stop_at):
        """capture the step cut off after section `stop_at` (None: all of it) into a HIP graph; ms per replay"""
        model.stop_at = stop_at
        with torch.cuda.stream(side):
            for _ in range(2):
                step(indices, optimize=False)
        torch.cuda.synchronize()
        g = capture(lambda: step(indices, optimize=False), side)[0]      # the stream that was warmed up; the step's result dropped
        return _time_steps(g.replay, steps, 1)[0]

    def failed(e):      # a capture failure must not take the bench line down
        import traceback
        traceback.print_exc(file=sys.stderr)
        return f"{type(e).__name__}: {str(e)[:300]}"

    try:
        rep = replay_ms(None)
        out["graph_replay"] = {"ms": round(rep, 2), "img_per_s": round(n_img / (rep * 1e-3), 2),
                               "note": "forward + backward (no optimizer step: a diagnostic of the device work per row) captured once into a HIP "
                                       "graph and replayed, the Hungarian assignment of the last eager step held fixed (its host round trip "
                                       "cannot be captured)"}
        # GPU time per row, forward + backward: replay time of the step cut off after each section (a surrogate loss = the sum of the
        # section's outputs), differenced; "criterion" = the rest (teacher + matcher-less losses and their backward into the heads)
        prev, table = 0.0, {}
        for name in SECTIONS:
            t = replay_ms(name)
            table[name] = round(t - prev, 2)
            prev = t
        table["teacher+criterion"] = round(rep - prev, 2)
        out["graph_replay"]["rows_fwd_bwd_ms"] = table
    except Exception as e:      # noqa: BLE001
        out.setdefault("graph_replay", {})["error"] = failed(e)
    finally:
        model.stop_at = None
    try:
        del model
        torch.cuda.empty_cache()
        out["graphed_sections"] = run_graphed(n_img, dev, steps=steps, warmup=warmup, library=library, grouped_repack=grouped_repack, **step_kwargs)
    except Exception as e:      # noqa: BLE001
        out["graphed_sections"] = {"error": failed(e)}
    return out


class _Part(nn.Module):
    """``fn``, a function of tensors, as a module (what torch.cuda.make_graphed_callables captures, forward and backward) over the
    parameters of ``step`` -- None for the criterion, which has none of its own"""

    def __init__(self, step, fn):
        super().__init__()
        self.step, self.fn = step, fn

    def forward(self, *tensors):
        return self.fn(*tensors)


def _time_steps(step, steps, warmup):
    """-> (ms per call of ``step`` over ``steps`` calls after ``warmup`` calls, host clock around a synchronise; the last loss)"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, loss


def _graphed_result(what, n_img, ms, loss, params, optimizer, library):
    """the keys every call of run_graphed / run_graphed_device returns; the caller adds what ``return_grads`` / ``return_model`` ask for"""
    return {"what": what, "optimizer": ("ClipAdamW(max_norm=0.1): clipping + AdamW in two library launches" if library else
                                        "AdamW(fused) + clip_grad_norm_(0.1)") if optimizer else None,
            "ms": round(ms, 2), "img_per_s": round(n_img / (ms * 1e-3), 2), "loss": float(loss.detach()),
            "grad_norm": float(torch.sqrt(sum((p.grad.float() ** 2).sum() for p in params if p.grad is not None)))}


def _grads(model):
    return {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


def run_graphed(n_img, dev, steps=5, warmup=2, optimizer=True, noise_seed=None, return_grads=False, lr=LR, return_model=False, fed_seed=None,
                device_matcher=False, library=False, grouped_repack=False, **step_kwargs):
    """The composed step as a trainer can run it WITHOUT freezing the matcher: the two device-only parts -- everything up to the matcher,
    and the criterion -- each captured once, forward and backward, with ``torch.cuda.make_graphed_callables`` (HIP graphs replayed by
    autograd), the Hungarian assignment between them live on the host every step.  Eagerly the step is bound by ~2900 kernel launches
    (ms above); this is the same work with three launches' worth of host time.  Returns the dict bench.py attaches as
    ``full_step.graphed_sections`` (``step_kwargs``: a smaller Step for the tests; ``return_model``: the trained Step and the graphed model
    part under "model" / "ga", ``images`` under "images", the training step under "step"; ``fed_seed``: Step.freeze_fed).  The packed / cast forms of the parameters are built INSIDE the captured graphs
    (richsem_amd/param_cache.py): every replay re-packs from the current masters, the frozen teacher's graph included.
    ``device_matcher``: the device-only form instead, see :func:`run_graphed_device`.  ``library``: make_optimizer's switch.
    ``grouped_repack``: :class:`GroupedRepack` -- the plan is recorded in the eager warm-up step, the graphs then hold no pack launch and the
    one refresh follows the optimizer step (``return_model``: the plan under "repack")."""
    if device_matcher:
        return run_graphed_device(n_img, dev, steps=steps, warmup=warmup, optimizer=optimizer, noise_seed=noise_seed, return_grads=return_grads, lr=lr,
                                  return_model=return_model, fed_seed=fed_seed, library=library, grouped_repack=grouped_repack, **step_kwargs)
    model, images, mask, targets = _setup(n_img, dev, noise_seed, fed_seed, False, **step_kwargs)
    part_a, part_b = _Part(model, lambda x: model.model_part(x, mask, teacher=False)), _Part(None, model.loss_part)
    repack = GroupedRepack(grouped_repack)
    with capture_stream() as side:      # the eager warm-up, the captures and the training steps (richsem_amd/capture.py)
        pinned = pin_grad_accumulators(model.parameters())      # noqa: F841  (before anything touches a parameter; alive to the end)
        with torch.no_grad():
            outs = model.model_part(images, mask)
        idx = model.pack_indices(model.match(*outs[:4], targets), targets)
        with repack.recording():
            model.loss_part(*model.model_part(images, mask), *idx).backward()      # (eager once: workspaces of this stream, caches)
        for p in model.parameters():
            p.grad = None
        sample_b = tuple(o.detach().clone().requires_grad_(i < 5) for i, o in enumerate(outs)) + tuple(idx)
        torch.cuda.synchronize()
        ga, gb = graphed_callables((part_a, part_b), ((images,), sample_b), allow_unused_input=True)
        # the frozen teacher (no gradient, independent of the student) is a HIP graph of its own, replayed BETWEEN the two halves of the
        # matching: the cost blocks and their copy to the host are enqueued first, the teacher's ~2 ms of GPU work run while the host
        # waits for that copy and solves the seven assignments (scipy) -- the round trip costs the step nothing
        for _ in range(2):
            model.teacher_part(images)
        torch.cuda.synchronize()
        teacher_graph, t_static = capture(lambda: model.teacher_part(images), side)
        loop = TrainLoop(model, repack, lr, library, optimizer)
        last = {}

        def body():
            outs = ga(images)
            with torch.no_grad():
                pending = model.match_begin(*outs[:4], targets)           # device cost blocks -> one host copy, enqueued
                teacher_graph.replay()
                assign = model.match_end(pending)                         # wait for the copy, scipy (matcher.py) -- under the teacher
            last["assign"] = assign
            return gb(*outs, t_static, *model.pack_indices(assign, targets))

        step = functools.partial(loop.step, body)
        ms, loss = _time_steps(step, steps, warmup)
    out = _graphed_result(
        "the same step with its two device-only parts (model up to the matcher; criterion) captured forward + backward by "
        "torch.cuda.make_graphed_callables and the Hungarian assignment live on the host between them every step, under the frozen "
        "teacher's forward (a HIP graph of its own, replayed while the host waits for the cost blocks and solves the assignments)"
        + ("; then gradient clipping (0.1) + fused AdamW step (reference engine.py:105-113): a TRAINING step, the same thing "
           "full_step_ddp measures at N > 1" if optimizer else "; no optimizer step"), n_img, ms, loss, loop.params, optimizer, library)
    if return_grads:
        out.update(grads=_grads(model), indices=last["assign"], topk=model.last_topk.clone())
    if return_model:
        out.update(model=model, ga=ga, images=images, step=lambda: _on_stream(side, step), repack=repack.plan)
    return out


def run_graphed_device(n_img, dev, steps=5, warmup=2, optimizer=True, noise_seed=None, return_grads=False, lr=LR, return_model=False,
                       fed_seed=None, library=False, grouped_repack=False, **step_kwargs):
    """The training step with NO host wait between its first and last kernel: model, cost blocks, the Hungarian assignment
    (``msda_lsap_*``), frozen teacher and criterion captured forward + backward as ONE ``torch.cuda.make_graphed_callables`` callable, then
    gradient clipping + fused AdamW.  The assignment is live: every replay solves it for that replay's model outputs.  The solver's status
    is copied to pinned memory after the replay and read one step late (a non-zero entry raises ValueError then).  Returns what
    :func:`run_graphed` returns; with ``return_model`` also "query_of_target" / "status": the static tensors every replay rewrites."""
    model, images, _, _ = _setup(n_img, dev, noise_seed, fed_seed, False, device_matcher=True, **step_kwargs)
    whole = _Part(model, lambda x: model(x, model._mask, model._targets))      # model, cost blocks, assignment, teacher, criterion
    repack = GroupedRepack(grouped_repack)
    with capture_stream() as side:
        pinned = pin_grad_accumulators(model.parameters())      # noqa: F841  (alive to the end)
        with repack.recording():
            whole(images).backward()      # (eager once: workspaces of this stream, caches, the solver's LDS attribute)
        for p in model.parameters():
            p.grad = None
        torch.cuda.synchronize()
        model.late_status.flush()
        gw = graphed_callables(whole, (images,), allow_unused_input=True)
        torch.cuda.synchronize()
        model.late_status.flush()      # (the warm-up iterations ran eagerly and pushed theirs)
        loop = TrainLoop(model, repack, lr, library, optimizer)

        def step(batch_images=images):
            loss = loop.forward_backward(lambda: gw(batch_images))
            # what only this harness does: the solver's status goes to the host between backward and optimizer (raises for the PREVIOUS step's)
            model.late_status.push(model.last_status)
            loop.update()
            return loss

        ms, loss = _time_steps(step, steps, warmup)
        model.late_status.flush()
    out = _graphed_result(
        "the same training step with the Hungarian assignment solved on the device (msda_lsap_*): model, cost blocks, assignment, "
        "frozen teacher and criterion captured forward + backward as ONE graphed callable, no host wait between the step's first "
        "and last kernel; the solver's status is read one step late"
        + ("; then gradient clipping (0.1) + fused AdamW step" if optimizer else "; no optimizer step"), n_img, ms, loss, loop.params, optimizer, library)
    if return_grads:
        out.update(grads=_grads(model), topk=model.last_topk.clone())
    if return_model:
        out.update(model=model, ga=gw, images=images, step=lambda *a: _on_stream(side, lambda: step(*a)),
                   query_of_target=model.last_qot, status=model.last_status, repack=repack.plan)
    return out


def _on_stream(stream, fn):
    """run ``fn`` on ``stream`` (where run_graphed pinned the parameters' AccumulateGrad nodes) and make the current stream wait for it"""
    with torch.cuda.stream(stream):
        out = fn()
    torch.cuda.current_stream().wait_stream(stream)
    return out


def run_ddp(n_img, dev, dist, steps=5, warmup=2, optimizer=True, make_model=None, backend_device=None, lr=LR, return_model=False):
    """The composed step as a data-parallel TRAINING step (round-3 verdict item 5; reference main.py:204-206 wraps the whole model in
    DistributedDataParallel, engine.py:100-114 runs backward + optimizer step): the module in ``DistributedDataParallel`` (nccl = RCCL
    on GPUs; ``gradient_as_bucket_view=True``, DDP's own 25 MB buckets overlapped with the backward), AdamW on every trained parameter,
    every rank on its own images.  Called by ALL ranks.  Returns, on every rank, the dict bench.py attaches as ``full_step_ddp``:
    ``ms`` (max over ranks, barrier + synchronise on both sides of the timed steps), ``ms_no_collective`` (the same steps under
    ``no_sync()``: no all-reduce) and the job's images per second.  ``make_model``: a stand-in module factory (tests/test_dist_gloo.py
    runs the protocol on CPU with gloo; the module needs ``batch()`` -> forward arguments and optionally ``prepare(*batch()[1:])``;
    ``return_model``: the trained module under "model")."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    live = dist is not None and dist.is_initialized()
    world = dist.get_world_size() if live else 1
    model = make_model() if make_model is not None else Step(n_img=n_img, seed=0, dev=dev)      # (same weights on every rank; DDP broadcasts anyway)
    if hasattr(model, "timing"):
        model.timing = False
    batch = model.batch(seed=dist.get_rank() if live else 0) if make_model is None else model.batch()
    if make_model is None:
        model.prepare(batch[1], batch[2])
    is_cuda = torch.device(dev).type == "cuda"
    ddp = DDP(model, device_ids=[torch.device(dev).index] if is_cuda else None, gradient_as_bucket_view=True,
              broadcast_buffers=False) if live else model
    params = [p for p in model.parameters() if p.requires_grad]
    opt = make_optimizer(params, lr, fused=is_cuda) if optimizer else None

    # Not TrainLoop: this loop clears through the optimizer (zero_grad(set_to_none=True)), runs forward + backward under DDP's no_sync()
    # for the second timing, and clips with clip_grad_norm_'s default ``foreach`` (tests/test_dist_gloo.py runs it on CPU tensors)
    def step(sync=True):
        if opt is not None:
            opt.zero_grad(set_to_none=True)
        else:
            for p in params:
                p.grad = None
        ctx = ddp.no_sync() if (not sync and ddp is not model) else contextlib.nullcontext()
        with ctx:
            loss = ddp(*batch)
            loss.backward()
        if opt is not None:
            torch.nn.utils.clip_grad_norm_(params, CLIP_MAX_NORM)      # engine.py:110-112
            opt.step()
        return loss

    def fence():
        if live:
            dist.barrier()
        if is_cuda:
            torch.cuda.synchronize()

    def timed(sync):
        for _ in range(warmup):
            step(sync)
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step(sync)
        fence()
        el = time.perf_counter() - t0
        if live and world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=backend_device or (dev if is_cuda else "cpu"))
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el / steps * 1e3, float(loss.detach())

    ms, loss = timed(True)
    ms_nc, _ = timed(False)
    unused = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    return {"what": "the composed step as a data-parallel training step: the module in DistributedDataParallel (RCCL, gradient_as_bucket_view, "
                    "25 MB buckets overlapped with the backward), gradient clipping (0.1) + AdamW step included, every rank on its own images; "
                    "ms = max over ranks",
            "world": world, "ms": round(ms, 2), "ms_no_collective": round(ms_nc, 2), "img_per_s": round(world * n_img / (ms * 1e-3), 2),
            "img_per_s_per_rank": round(n_img / (ms * 1e-3), 2), "optimizer": "AdamW" if optimizer else None, "loss": loss,
            "trained_parameters": sum(p.numel() for p in params), "parameters_without_gradient": unused,
            **({"model": model} if return_model else {})}


# ---- the command line: one table of (flag, keyword, help); cli_kwargs turns the parsed flags into keywords ----------------------------------
SWITCHES = (
    ("--fed-loss", "fed_loss", "the criterion's federated loss (use_fed_loss, 50 classes per draw; synthetic class weights: Step.loss_part)"),
    ("--device-distill", "device_distill", "the criterion's KL distillation term as one row kernel (distill.DistillKL) instead of the PyTorch "
     "composition: Step.loss_part"),
    ("--device-dn", "device_dn", "the denoising queries (label / box noise, label embedding, padded query block, mask) from one kernel that reads "
     "the target counts on the device (richsem_amd/dn.py) instead of torch ops on the host's layout: Step.dn_section"),
    ("--device-geometry", "device_geometry", "the batch's geometry tensors (masks, valid ratios, reference points, sine position, anchors) from "
     "one kernel inside the step (richsem_amd/geometry.py) instead of torch ops in prepare(): Step.run_sections"),
    ("--library-optimizer", "library", "richsem_amd.optim.ClipAdamW (gradient clipping + AdamW in two launches of the library's own) instead "
     "of clip_grad_norm_ + torch's fused AdamW"),
    ("--grouped-repack", "grouped_repack", "every derived form of the parameters (bf16 casts, packed weights) refreshed from the masters in ONE "
     "launch after the optimizer step (richsem_amd/repack.py) instead of rebuilt by every cache inside the captured graphs"),
)


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser()
    for name, default in (("--steps", 5), ("--warmup", 2), ("--images", 2)):
        ap.add_argument(name, type=int, default=default)
    ap.add_argument("--no-graph", action="store_true", help="eager steps only (the form profiled for profiles/*_step_kernels.md)")
    ap.add_argument("--stop-at", default=None, help="profiling aid: cut the step off after this section (implies --no-graph): " + ", ".join(SECTIONS))
    ap.add_argument("--boxes-per-image", type=int, default=12, help="targets per synthetic image (default 12)")
    ap.add_argument("--device-matcher", action="store_true", help="time the graphed training step in both forms: the Hungarian assignment on the host "
                    "between two captured parts (twice, to show its spread) and on the device inside one captured step")
    for flag, _, text in SWITCHES:
        ap.add_argument(flag, action="store_true", help=text)
    return ap.parse_args(argv)


def cli_kwargs(a_):
    """the parsed command line -> (Step's keywords, the harness's): a switch of the table goes to Step where Step takes its keyword, to the
    harness otherwise, and only where its flag is given"""
    on = {kw: True for flag, kw, _ in SWITCHES if getattr(a_, flag[2:].replace("-", "_"))}
    of_step = inspect.signature(Step.__init__).parameters
    return ({"boxes_per_image": a_.boxes_per_image, **{k: v for k, v in on.items() if k in of_step}},
            {"steps": a_.steps, "warmup": a_.warmup, **{k: v for k, v in on.items() if k not in of_step}})


def main(argv=None):
    import json
    a_ = parse_args(argv)
    step_kw, harness_kw = cli_kwargs(a_)
    dev = torch.device("cuda", 0)
    if not a_.device_matcher:
        print(json.dumps(run(a_.images, dev, graph=not (a_.no_graph or a_.stop_at), stop_at=a_.stop_at, **harness_kw, **step_kw), indent=1))
        return
    res = {"boxes_per_image": a_.boxes_per_image}
    for name, dm in (("host_matcher", False), ("host_matcher_again", False), ("device_matcher", True)):
        r = run_graphed(a_.images, dev, device_matcher=dm, **harness_kw, **step_kw)
        res[name] = {k: r[k] for k in ("ms", "img_per_s", "loss")}
        torch.cuda.empty_cache()
        print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
