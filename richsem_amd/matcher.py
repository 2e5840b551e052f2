"""Hungarian matching with the cost blocks formed on the GPU (criterion plumbing).

Mirror of the reference's ``HungarianMatcher`` (models/richsem/matcher.py:8-78; same constructor, same ``forward(outputs,
targets)`` result: a list over images of (query indices, target indices) as int64 tensors).  What changes is the plumbing the
survey names: the reference forms the cost of every query against every target of the whole batch with a dozen element-wise
kernels, keeps the diagonal blocks only, and brings each matrix to the host with a synchronising ``.cpu()`` -- seven times a step
(richsem.py:1136, :1204, :1255).  Here one kernel (``msda_matcher_cost_*``, csrc/msda_matcher.h) writes the diagonal blocks only,
and :func:`match_many` lays the blocks of ALL decoder outputs of a step into one buffer that reaches the host with ONE
asynchronous copy and ONE event wait.  The assignment itself stays scipy's ``linear_sum_assignment`` on the host, as
``north_star`` asks (criterion in host Python).

:func:`global_num_boxes` / :class:`AsyncLossLog` remove the two remaining per-step device round trips of the criterion and the
engine (richsem.py:1143-1147, engine.py:84-91): the box count is known on the host and reduced there, the reduced loss dictionary
for the log is read one step late.

``HungarianMatcher(solver="device")`` / :meth:`HungarianMatcher.match_many_device` solve the assignment on the device instead
(``msda_lsap_*``, csrc/msda_lsap.h): opt-in, the default stays the host path above.  With a :class:`CostPlan` built beforehand the device
form neither waits nor copies anything to the host, so the whole training step can be one captured graph (bench_step.py
``device_matcher``); :func:`pairs_from_query_of_target` turns its result into the criterion's index tensors.
"""
import ctypes

import torch
from scipy.optimize import linear_sum_assignment
from torch import nn

from . import _lib, focal


def _stream(dev):
    return _lib.raw_stream(dev)


def _sizes_and_offsets(targets):
    """the per-image target counts of a batch and their prefix [0, T_0, T_0 + T_1, ...]"""
    sizes = [int(v["boxes"].shape[0]) for v in targets]
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    return sizes, offsets


def _read_late(t):
    """start reading the device tensor ``t`` on the host without a wait: -> (its copy in pinned memory, an event recorded behind the copy on
    the current stream); the copy is valid once the event has completed -- one step later, for the classes below"""
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    event = torch.cuda.Event()
    event.record(torch.cuda.current_stream(t.device))
    return host, event


class CostPlan:
    """Host-side bookkeeping of one batch of targets: per-image counts, their prefix on host and device, concatenated labels /
    boxes (matcher.py:55-57)."""

    def __init__(self, targets, device, dtype):
        self.device, self.dtype = torch.device(device), dtype
        self.num_queries = None      # (set by match_many_device: the query count the last solve ran with)
        self.sizes, self.offsets = _sizes_and_offsets(targets)
        self.total = self.offsets[-1]
        self.offsets_dev = torch.tensor(self.offsets, dtype=torch.int64).to(device, non_blocking=True)
        if self.total:
            self.tgt_ids = torch.cat([v["labels"] for v in targets]).to(device=device, dtype=torch.int64).contiguous()
            self.tgt_boxes = torch.cat([v["boxes"] for v in targets]).to(device=device, dtype=dtype).contiguous()
        else:
            self.tgt_ids = torch.zeros(0, dtype=torch.int64, device=device)
            self.tgt_boxes = torch.zeros(0, 4, dtype=dtype, device=device)

    @torch.no_grad()
    def update_(self, targets):
        """write another batch's labels, boxes and offsets into the device buffers this plan already has -- the same number of images and
        the same TOTAL number of targets (the per-image counts may change), anything else raises -- so that a graph captured with this plan
        solves the next batch on its next replay.  Host -> device copies on the current stream: call it between replays, not in a capture."""
        sizes, offsets = _sizes_and_offsets(targets)
        if len(sizes) != len(self.sizes):
            raise ValueError(f"CostPlan.update_: {len(sizes)} images, the plan was built for {len(self.sizes)}")
        if sum(sizes) != self.total:
            raise ValueError(f"CostPlan.update_: {sum(sizes)} targets in all, the plan was built for {self.total}")
        self.sizes, self.offsets = sizes, offsets
        self.offsets_dev.copy_(torch.tensor(offsets, dtype=torch.int64), non_blocking=True)
        if self.total:
            self.tgt_ids.copy_(torch.cat([v["labels"] for v in targets]).to(torch.int64), non_blocking=True)
            self.tgt_boxes.copy_(torch.cat([v["boxes"] for v in targets]).to(self.dtype), non_blocking=True)
        return self


class TargetBuffers:
    """The capacity form of :class:`CostPlan`: device buffers for ``n_images`` images and up to ``capacity`` targets in all, filled by
    :meth:`update_`.  ``total`` is the CAPACITY -- the size every launch that takes this plan is shaped by --; how many targets are live
    is ``offsets_dev[-1]``, which the kernels read on the device (``msda_matcher_cost_*`` writes ``nq * offsets_dev[-1]`` cost elements,
    ``msda_lsap_*`` the first ``offsets_dev[-1]`` columns of ``query_of_target``, ``msda_criterion_pairs_f32`` reads no further).  So a
    graph captured with these buffers serves any batch that fits them, whatever its per-image counts and their total.  Rows past the
    live targets hold label 0 and box (0.5, 0.5, 1, 1).  ``cost_blocks``, ``solve_blocks`` and ``match_many_device`` take it as a plan."""

    def __init__(self, n_images, capacity, device, dtype=torch.float32, max_per_image=None):
        n_images, capacity = int(n_images), int(capacity)
        if n_images < 1 or capacity < 1:
            raise ValueError(f"TargetBuffers: n_images and capacity must be >= 1, got {n_images} and {capacity}")
        self.device, self.dtype = torch.device(device), dtype
        self.num_queries = None
        self.capacity = self.total = capacity
        self.max_per_image = None if max_per_image is None else int(max_per_image)
        self.sizes = [0] * n_images
        self.offsets = [0] * (n_images + 1)
        self.live = 0
        self.offsets_dev = torch.zeros(n_images + 1, dtype=torch.int64, device=device)
        self.tgt_ids = torch.zeros(capacity, dtype=torch.int64, device=device)
        self.tgt_boxes = torch.tensor([0.5, 0.5, 1.0, 1.0], dtype=dtype).repeat(capacity, 1).to(device)

    @torch.no_grad()
    def update_(self, targets):
        """write a batch -- a list over the images of dicts with "labels" (T_b) and "boxes" (T_b, 4) -- into the buffers: host -> device
        copies on the current stream, between replays and not in a capture, as :meth:`CostPlan.update_`.  Another image count, more
        targets than ``capacity``, or an image with more than ``max_per_image`` of them raise ValueError and leave the buffers alone."""
        sizes, offsets = _sizes_and_offsets(targets)
        if len(sizes) != len(self.sizes):
            raise ValueError(f"TargetBuffers.update_: {len(sizes)} images, the buffers were built for {len(self.sizes)}")
        if sum(sizes) > self.capacity:
            raise ValueError(f"TargetBuffers.update_: {sum(sizes)} targets in all, the capacity is {self.capacity}")
        if self.max_per_image is not None and max(sizes) > self.max_per_image:
            raise ValueError(f"TargetBuffers.update_: an image with {max(sizes)} targets, at most {self.max_per_image} are allowed")
        live = offsets[-1]
        ids = torch.zeros(self.capacity, dtype=torch.int64)
        boxes = torch.tensor([0.5, 0.5, 1.0, 1.0], dtype=self.dtype).repeat(self.capacity, 1)
        if live:
            ids[:live] = torch.cat([v["labels"].detach().cpu().to(torch.int64).reshape(-1) for v in targets])
            boxes[:live] = torch.cat([v["boxes"].detach().cpu().to(self.dtype).reshape(-1, 4) for v in targets])
        self.sizes, self.offsets, self.live = sizes, offsets, live
        self.offsets_dev.copy_(torch.tensor(offsets, dtype=torch.int64), non_blocking=True)
        self.tgt_ids.copy_(ids, non_blocking=True)
        self.tgt_boxes.copy_(boxes, non_blocking=True)
        return self

    def class_agnostic(self):
        """the reference's ``enc_targets`` (richsem.py:1249-1255: the targets with every label set to 0, which the two-stage output is matched
        and scored against under ``enc_cls_agn``) as a plan over the SAME buffers: see :class:`ClassAgnosticTargets`"""
        return ClassAgnosticTargets(self)


class ClassAgnosticTargets:
    """A :class:`TargetBuffers` seen with every label 0.  ``offsets_dev`` and ``tgt_boxes`` ARE the parent's tensors, and the size bookkeeping
    (``sizes``, ``offsets``, ``live``, ``total``) is read from the parent, so it follows the parent's ``update_`` without a call of its own;
    ``tgt_ids`` is a constant zero buffer of the parent's capacity.  ``cost_blocks`` and ``match_many_device(last_plan=...)`` take it."""

    def __init__(self, parent):
        self.parent = parent
        self.num_queries = None
        self.tgt_ids = torch.zeros(parent.capacity, dtype=torch.int64, device=parent.device)

    device = property(lambda self: self.parent.device)
    dtype = property(lambda self: self.parent.dtype)
    capacity = property(lambda self: self.parent.capacity)
    total = property(lambda self: self.parent.total)
    max_per_image = property(lambda self: self.parent.max_per_image)
    sizes = property(lambda self: self.parent.sizes)
    offsets = property(lambda self: self.parent.offsets)
    live = property(lambda self: self.parent.live)
    offsets_dev = property(lambda self: self.parent.offsets_dev)
    tgt_boxes = property(lambda self: self.parent.tgt_boxes)

    def update_(self, targets):
        """the parent's ``update_`` (the labels of ``targets`` go to the parent; here they stay 0)"""
        self.parent.update_(targets)
        return self


def cost_blocks(pred_logits, pred_boxes, plan, cost_class, cost_bbox, cost_giou, focal_alpha, out=None, target_major=False):
    """Diagonal cost blocks of one decoder output on the device: a flat tensor of nq * plan.total elements, image b's (nq x T_b)
    block starting at nq * plan.offsets[b].  ``out``: slice of a larger buffer to write into.  ``target_major``: every block stored
    (T_b x nq) instead -- the same values in the layout the device solver scans with unit stride (``msda_matcher_cost_tm_*``)."""
    if not pred_logits.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    dt = pred_logits.dtype
    if dt not in (torch.float32, torch.float64):
        raise RuntimeError(f"matcher cost: float32 / float64 logits, got {dt}")
    bs, nq, C = pred_logits.shape
    assert pred_boxes.shape == (bs, nq, 4) and len(plan.sizes) == bs
    logits, boxes = pred_logits.detach().contiguous(), pred_boxes.detach().to(dt).contiguous()
    n = nq * plan.total
    if out is None:
        out = torch.empty(n, dtype=dt, device=logits.device)
    assert out.numel() == n and out.dtype == dt and out.is_contiguous()
    if n:
        fn = getattr(_lib.load(), ("msda_matcher_cost_tm_" if target_major else "msda_matcher_cost_") + ("f32" if dt == torch.float32 else "f64"))
        with _lib.on_device(logits.device):
            _lib.check(fn(logits.data_ptr(), boxes.data_ptr(), plan.tgt_ids.data_ptr(), plan.tgt_boxes.data_ptr(),
                          plan.offsets_dev.data_ptr(), bs, nq, C, plan.total, float(cost_class), float(cost_bbox), float(cost_giou),
                          float(focal_alpha), out.data_ptr(), _stream(logits.device)))
    return out


def _assign(host, nq, plan):
    res = []
    for b, tb in enumerate(plan.sizes):
        block = host[nq * plan.offsets[b]: nq * plan.offsets[b + 1]].view(nq, tb)
        i, j = linear_sum_assignment(block.numpy())
        res.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
    return res


LSAP_MAX_DIM = 4096      # msda_lsap_*: queries per output, and targets per batch (csrc/msda_lsap.h kLsapMaxDim)


def lsap_supported(nq, total):
    """whether the device solver takes ``nq`` queries against ``total`` targets in the batch (beyond: MSDA_ERR_TOO_LARGE, the host solves)"""
    return nq <= LSAP_MAX_DIM and total <= LSAP_MAX_DIM


def solve_blocks(cost, plan, n_out, nq, target_major=False):
    """``msda_lsap_*`` on ``n_out`` consecutive cost buffers of nq * plan.total elements (float32 / float64, as :func:`cost_blocks` writes
    them) -> (query_of_target (n_out, plan.total) int64, status (n_out, images) int32), see include/richsem_msda.h.  One launch; the
    per-image counts are read from ``plan.offsets_dev`` by the kernel.  Nothing waits."""
    if not cost.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if cost.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"lsap: float32 / float64 costs, got {cost.dtype}")
    B = len(plan.sizes)
    assert cost.is_contiguous() and cost.numel() == n_out * nq * plan.total
    qot = torch.empty((n_out, plan.total), dtype=torch.int64, device=cost.device)
    status = torch.empty((n_out, B), dtype=torch.int32, device=cost.device)
    L = _lib.load()
    nbytes = ctypes.c_int64(0)
    _lib.check(L.msda_lsap_workspace_bytes(n_out, B, nq, plan.total, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=cost.device) if nbytes.value else None
    fn = L.msda_lsap_f32 if cost.dtype == torch.float32 else L.msda_lsap_f64
    with _lib.on_device(cost.device):
        _lib.check(fn(cost.data_ptr(), int(bool(target_major)), plan.offsets_dev.data_ptr(), n_out, B, nq, plan.total, qot.data_ptr(),
                      status.data_ptr(), ws.data_ptr() if ws is not None else None, _stream(cost.device)))
    return qot, status


def pairs_from_query_of_target(query_of_target, plan, num_queries=None):
    """The criterion's index tensors from the device solver's result, as ``Step.pack_indices`` (bench_step.py) lays them out: with
    ``query_of_target`` (n_out, total) of n_out - 1 decoder outputs followed by the two-stage output -> three (4, K) int64 tensors of rows
    (layer, image, query, target): the decoder outputs' pairs (K = (n_out - 1) * total), the two-stage output's and the last decoder
    layer's (K = total, layer 0).  Pure torch on the tensors' device (CPU tensors work too), nothing read back: a target's image comes from
    ``plan.offsets_dev`` (which follows :meth:`CostPlan.update_`), a query left at -1 by an unsolved block is clamped to 0 -- the solver's
    status, read late, is what reports it.  Pairs come in target order (the host path: query order); the pair SET is the same.
    Every image must have at most ``num_queries`` targets (default: what the plan was last solved with), since the criterion's tensors hold
    one pair per target: checked on the host from ``plan.sizes``."""
    nq = plan.num_queries if num_queries is None else num_queries
    if nq is not None and plan.sizes and max(plan.sizes) > nq:
        raise ValueError(f"pairs_from_query_of_target: an image with {max(plan.sizes)} targets against {nq} queries leaves targets unmatched")
    n_out, total = query_of_target.shape
    assert total == plan.total and n_out >= 2
    dev = query_of_target.device
    tj = torch.arange(total, dtype=torch.int64, device=dev)
    bi = torch.bucketize(tj, plan.offsets_dev[1:].to(dev), right=True)
    si = query_of_target.clamp(min=0)

    def rows(first, last):
        n = last - first
        li = torch.arange(n, dtype=torch.int64, device=dev)[:, None].expand(n, total)
        return torch.stack((li.reshape(-1), bi.repeat(n), si[first:last].reshape(-1), tj.repeat(n)))
    return rows(0, n_out - 1), rows(n_out - 1, n_out), rows(n_out - 2, n_out - 1)


class HungarianMatcher(nn.Module):
    """Same signature and result as the reference's class (matcher.py:8-78).  ``solver``: "host" (default) -- scipy's
    ``linear_sum_assignment`` on cost blocks copied to the host; "device" -- the same assignment from ``msda_lsap_*`` on the GPU (equal to
    scipy's wherever the optimum is unique; any optimal assignment where costs tie), read back for the reference's list format."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, focal_alpha=0.25, solver="host"):
        super().__init__()
        if solver not in ("host", "device"):
            raise ValueError(f'HungarianMatcher: solver must be "host" or "device", got {solver!r}')
        self.solver = solver
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.focal_alpha = focal_alpha
        self._pinned = None

    def _host_buffer(self, n, dtype):
        if self._pinned is None or self._pinned.numel() < n or self._pinned.dtype != dtype:
            self._pinned = torch.empty(max(n, 1), dtype=dtype, pin_memory=True)
        return self._pinned[:n]

    @torch.no_grad()
    def match_many(self, outputs_list, targets):
        """Match several decoder outputs (each a dict with "pred_logits" (bs, nq_o, C) and "pred_boxes" (bs, nq_o, 4)) against the
        same targets: one cost kernel per output into one device buffer, one copy to the host, one wait.  Returns a list (per
        output) of the reference's per-image index pairs."""
        if self.solver == "device":
            first = outputs_list[0]["pred_logits"]
            plan = CostPlan(targets, first.device, first.dtype)
            if all(lsap_supported(o["pred_logits"].shape[1], plan.total) for o in outputs_list):
                return self._lists_from_device(*self.match_many_device(outputs_list, plan), plan)
            # (beyond the kernel's limits -- MSDA_ERR_TOO_LARGE -- the host path solves, as documented)
        return self.match_many_end(self.match_many_begin(outputs_list, targets))

    @torch.no_grad()
    def match_many_device(self, outputs_list, plan, target_major=True, last_plan=None):
        """Match several decoder outputs against the targets of ``plan`` (a :class:`CostPlan` built BEFOREHAND: its constructor copies host
        data to the device) entirely on the device: cost kernels into one buffer, then one ``msda_lsap_*`` launch per run of outputs with
        the same query count (one launch when all have it).  -> (query_of_target (n_out, plan.total) int64: the query matched to each
        target, -1 where none; status (n_out, images) int32: 0 solved, non-zero see include/richsem_msda.h).  Nothing waits and nothing
        reaches the host: safe inside ``torch.cuda.graph`` / ``make_graphed_callables`` after one eager call; ``plan.update_`` feeds a
        captured call its next batch.  ``last_plan``: the plan the LAST output's cost blocks are computed against -- the two-stage output
        under ``enc_cls_agn`` against ``plan.class_agnostic()`` (richsem.py:1249-1255) --; it shares ``plan``'s offsets, so the solve launches
        are the same."""
        if last_plan is not None and (last_plan.total != plan.total or last_plan.offsets_dev.data_ptr() != plan.offsets_dev.data_ptr()):
            raise ValueError("match_many_device: last_plan shares the offsets of plan (plan.class_agnostic())")
        first = outputs_list[0]["pred_logits"]
        nqs = [o["pred_logits"].shape[1] for o in outputs_list]
        dev_buf = torch.empty(sum(nq * plan.total for nq in nqs), dtype=first.dtype, device=first.device)
        at, runs = 0, []
        for i, (o, nq) in enumerate(zip(outputs_list, nqs)):
            cost_plan = last_plan if last_plan is not None and i == len(nqs) - 1 else plan
            cost_blocks(o["pred_logits"], o["pred_boxes"], cost_plan, self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha,
                        out=dev_buf[at: at + nq * plan.total], target_major=target_major)
            if runs and runs[-1][1] == nq:
                runs[-1][2] += 1
            else:
                runs.append([at, nq, 1])
            at += nq * plan.total
        parts = [solve_blocks(dev_buf[a: a + n * nq * plan.total], plan, n, nq, target_major) for a, nq, n in runs]
        plan.num_queries = min(nqs)
        if len(parts) == 1:
            return parts[0]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    @staticmethod
    def _lists_from_device(query_of_target, status, plan):
        """the reference's format from the solver's result (reads it back: one wait); a block that was not solved raises as scipy does"""
        st, qot = status.cpu(), query_of_target.cpu()
        if bool((st != 0).any()):
            o, b = (st != 0).nonzero()[0].tolist()
            raise ValueError(f"matrix contains invalid numeric entries (output {o}, image {b}: solver status {int(st[o, b])})")
        res = []
        for row in qot:
            per_image = []
            for b in range(len(plan.sizes)):
                q = row[plan.offsets[b]: plan.offsets[b + 1]]
                j = (q >= 0).nonzero()[:, 0]
                i, order = q[j].sort()
                per_image.append((i, j[order]))
            res.append(per_image)
        return res

    @torch.no_grad()
    def match_many_begin(self, outputs_list, targets):
        """the device half of :meth:`match_many`: cost kernels, the copy to pinned host memory and an event behind it are ENQUEUED; nothing
        waits.  Work enqueued after this call (a frozen teacher's forward, say) runs on the GPU while :meth:`match_many_end` waits for the
        copy and solves the assignments on the host."""
        first = outputs_list[0]["pred_logits"]
        plan = CostPlan(targets, first.device, first.dtype)
        nqs = [o["pred_logits"].shape[1] for o in outputs_list]
        total = sum(nq * plan.total for nq in nqs)
        dev_buf = torch.empty(total, dtype=first.dtype, device=first.device)
        at = 0
        for o, nq in zip(outputs_list, nqs):
            cost_blocks(o["pred_logits"], o["pred_boxes"], plan, self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha,
                        out=dev_buf[at: at + nq * plan.total])
            at += nq * plan.total
        host = self._host_buffer(total, first.dtype)
        host.copy_(dev_buf, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(first.device))
        return plan, nqs, host, done, dev_buf

    @torch.no_grad()
    def match_many_end(self, pending):
        plan, nqs, host, done, _keep = pending
        done.synchronize()          # the one wait of the step's matching (the reference: one .cpu() per output)
        res, at = [], 0
        for nq in nqs:
            res.append(_assign(host[at: at + nq * plan.total], nq, plan))
            at += nq * plan.total
        return res

    @torch.no_grad()
    def forward(self, outputs, targets):
        return self.match_many([outputs], targets)[0]


def global_num_boxes(indices, world_size=1, group=None):
    """``num_boxes`` of the criterion (richsem.py:1143-1147: number of matched targets summed over the ranks, divided by the world
    size, clamped to >= 1) without the device round trip: the count is a host integer already, so it is reduced as a host tensor
    (a gloo group) -- or not at all on one rank -- instead of a CUDA tensor + ``.item()``."""
    n = float(sum(len(t[1]) for t in indices))
    if world_size > 1:
        import torch.distributed as dist
        t = torch.tensor([n], dtype=torch.float32)
        dist.all_reduce(t, group=group)     # `group` must be a CPU (gloo) group: the tensor lives on the host
        n = float(t.item())
    return max(n / world_size, 1.0)


class AsyncLossLog:
    """The engine's logging reduction (engine.py:84-91 with util/misc.py:139-164) without its per-step ``.item()``: the loss
    dictionary is stacked in sorted key order (as reduce_dict does), all-reduced asynchronously, copied to pinned memory, and
    READ ONE STEP LATE -- ``push`` returns the previous step's reduced dictionary (None on the first call), ``flush`` the last."""

    def __init__(self, world_size=1, group=None, average=True):
        self.world_size, self.group, self.average = world_size, group, average
        self._pending = None

    def _finish(self):
        if self._pending is None:
            return None
        names, host, event = self._pending
        if event is not None:
            event.synchronize()
        self._pending = None
        return {k: float(v) for k, v in zip(names, host.tolist())}

    @torch.no_grad()
    def push(self, loss_dict):
        prev = self._finish()
        names = sorted(loss_dict.keys())
        values = torch.stack([loss_dict[k].detach().float().reshape(()) for k in names], dim=0)
        if self.world_size > 1:
            import torch.distributed as dist
            # on RCCL the wait below is a stream dependency, not a host block; on a host (gloo) group it blocks, as it must
            dist.all_reduce(values, group=self.group, async_op=True).wait()
            if self.average:
                values = values / self.world_size
        self._pending = (names,) + (_read_late(values) if values.is_cuda else (values, None))
        return prev

    def flush(self):
        return self._finish()


class LateStatus:
    """The device solver's status (``match_many_device``) without a wait: ``push`` copies this step's status tensor to pinned memory behind
    an event and checks the PREVIOUS step's -- a non-zero entry raises ValueError (scipy raises for the same inputs, at once) --, ``flush``
    checks the last one.  The read is one step late, as :class:`AsyncLossLog`'s."""

    def __init__(self):
        self._pending = None

    def _finish(self):
        if self._pending is None:
            return
        host, event = self._pending
        self._pending = None
        if event is not None:
            event.synchronize()
        if bool((host != 0).any()):
            raise ValueError(self._message(host))

    @staticmethod
    def _message(host):
        """the error text for a status with a non-zero entry (subclasses: what their status means)"""
        o, b = (host != 0).nonzero()[0].tolist()
        return f"matrix contains invalid numeric entries (the previous step's assignment: output {o}, image {b}, solver status {int(host[o, b])})"

    @torch.no_grad()
    def push(self, status):
        self._finish()
        self._pending = _read_late(status) if status.is_cuda else (status.clone(), None)

    def flush(self):
        self._finish()


class FocalNegativeSum(torch.autograd.Function):
    """``sum_rows w[row] * sum_c (1 - alpha) * sigmoid(x)^2 * softplus(x)``: the sigmoid focal loss (reference richsem.py:1124-1160 through
    ``sigmoid_focal_loss``) of a logit tensor as if every entry were negative, with one weight per row (query) -- the criterion adds what
    the few positive entries contribute instead.  One kernel forward, one backward (``msda_focal_neg_sum_f32 / msda_focal_neg_grad_f32``,
    csrc/rows_api.hip) where PyTorch's ops make a dozen passes over the (6, N, queries, classes) logits.
    ``apply(logits (..., C) float32, row_weight (...) float32, alpha)`` -> 0-dim float32."""

    @staticmethod
    def forward(ctx, logits, row_weight, alpha):
        if not logits.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        assert logits.dtype == torch.float32 and row_weight.dtype == torch.float32 and row_weight.numel() * logits.shape[-1] == logits.numel()
        x, w = logits.contiguous(), row_weight.contiguous()
        ctx.save_for_backward(x, w)
        ctx.alpha = float(alpha)
        with _lib.on_device(x.device):
            return focal.neg_sum(x, w, ctx.alpha).sum().float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        with _lib.on_device(x.device):
            return focal.neg_grad(x, w, ctx.alpha, g.reshape(1).float().contiguous()), None, None


class _PairSum(torch.autograd.Function):
    """a weighted per-pair loss as one kernel: the forward computes the sum AND its gradient w.r.t. the predictions; the backward scales"""

    @staticmethod
    def _launch(ctx, fn, pred, *args):
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        with _lib.on_device(pred.device):
            _lib.check(fn(pred.data_ptr(), *args, loss.data_ptr(), grad.data_ptr(), _lib.raw_stream(pred.device)))
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return (grad * g,) + (None,) * (ctx.n_inputs - 1)


class BoxPairLoss(_PairSum):
    """``sum_k w[k] * (c_l1 * |p_k - t_k|_1 + c_giou * (1 - GIoU(p_k, t_k)))`` over K matched (cx, cy, w, h) pairs (SetCriterion.loss_boxes,
    richsem.py:1162-1188) as one kernel (``msda_box_pair_loss_f32``): ``apply(pred (K, 4), target (K, 4), weight (K), c_l1, c_giou)`` -> 0-dim;
    gradient for ``pred``.  PyTorch's op sequence is ~35 launches forward and ~70 backward on a few thousand pairs."""

    @staticmethod
    def forward(ctx, pred, target, weight, c_l1, c_giou):
        if not pred.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        assert pred.dtype == torch.float32 and pred.dim() == 2 and pred.shape[1] == 4 and target.shape == pred.shape and weight.numel() == pred.shape[0]
        p, t, w = pred.contiguous(), target.detach().float().contiguous(), weight.detach().float().contiguous()
        ctx.n_inputs = 5
        if p.shape[0] == 0:
            ctx.save_for_backward(torch.zeros_like(p))
            return p.sum()
        return _PairSum._launch(ctx, _lib.load().msda_box_pair_loss_f32, p, t.data_ptr(), w.data_ptr(), p.shape[0], float(c_l1), float(c_giou))


class FocalPositiveSum(_PairSum):
    """``sum_k w[k] * (alpha (1 - q_k)^2 softplus(-x_k) - (1 - alpha) q_k^2 softplus(x_k))``, q = sigmoid(x): what the positive entries of a
    sigmoid focal loss contribute instead of the all-negative term :class:`FocalNegativeSum` counted for them, as one kernel
    (``msda_focal_pos_sum_f32``): ``apply(x (K), weight (K), alpha)`` -> 0-dim; gradient for ``x``."""

    @staticmethod
    def forward(ctx, x, weight, alpha):
        if not x.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        assert x.dtype == torch.float32 and x.dim() == 1 and weight.numel() == x.numel()
        xc, w = x.contiguous(), weight.detach().float().contiguous()
        ctx.n_inputs = 3
        if xc.numel() == 0:
            ctx.save_for_backward(torch.zeros_like(xc))
            return xc.sum()
        return _PairSum._launch(ctx, _lib.load().msda_focal_pos_sum_f32, xc, w.data_ptr(), xc.numel(), float(alpha))
