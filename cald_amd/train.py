"""Training step of the Faster R-CNN detector on the MI355X.

What the reference does per iteration (cald_train.py:40-74 ``train_one_epoch``; detection/engine.py:19-61):

    loss_dict = task_model(images, targets); losses = sum(loss_dict.values())
    task_optimizer.zero_grad(); losses.backward(); task_optimizer.step()

with ``task_model`` = detection/frcnn_la.py ``FRCNN_Feature`` in train mode -- i.e. torchvision 0.8.2's GeneralizedRCNN training
forward (transform -> ResNet-FPN -> RPN losses -> sampled RoI-head losses) under torch autograd on cuDNN/cuBLAS.  Here the same
graph is strung from the ``cald_train_*`` device operators (cald_amd/csrc/train_*.hip): the forward runs on the inference MFMA
kernels with weights packed on the device every step, the backward is hand-written (data gradients on the same kernels with the
flipped filter, weight gradients on the split-K MFMA kernel, RoIAlign / FPN / ReLU / FrozenBatchNorm backward kernels), and
``SGD`` is one fused kernel per tensor.  torch supplies device memory, the stream, the Parameter / Optimizer / autograd-Function
*interfaces* (so ``losses.backward()`` and the reference's lr schedulers work unchanged) and the CPU random permutations of the
samplers; it performs none of the arithmetic.

torchvision semantics restated here (0.8.2, "TV-mem" in SURVEY Appendix A; in-repo copies cited where they exist):
  * trainable parameters: body layers 2-4 (``resnet_fpn_backbone(trainable_layers=3)``), FPN, RPN head, box head, predictor;
    every BatchNorm is FrozenBatchNorm2d; conv1 / layer1 are frozen                                    (frcnn_la.py:283)
  * RPN: anchors (32..512) x (0.5, 1, 2); Matcher(0.7, 0.3, allow_low_quality); BalancedPositiveNegativeSampler(256, 0.5);
    BCE-with-logits objectness loss; smooth-L1 (beta 1/9) box loss / #sampled; proposals from pre/post_nms_top_n_train = 2000
                                                                                                        (frcnn_la.py:154-203)
  * RoI heads: proposals + ground truth; Matcher(0.5, 0.5); sampler(512, 0.25); BoxCoder (10, 10, 5, 5); cross-entropy +
    smooth-L1 (beta 1/9) / #sampled                                                                     (frcnn_la.py:160-222)
The samplers draw from torch's CPU generator (the reference draws ``torch.randperm`` on its CUDA device: a different stream of
random numbers, the same distribution over subsets).  ``sampler="choose_k"`` (default) keeps the k smallest of iid uniform keys, one per candidate: ``choose_k``
below for the RPN anchors of an image, one ``torch.rand`` call and one host routine (``cald_train_roi_sample_host``) for the RoI
candidates of the whole batch; ``sampler="randperm"`` consumes ``torch.randperm(n, generator=g)[:k]`` for the positives, then for the negatives, image by
image, RPN before the RoI heads -- exactly the calls torchvision's BalancedPositiveNegativeSampler makes, so a seeded CPU
generator reproduces torchvision's own samples (``tests/test_gpu_train.py::test_randperm_sampler_*``).
"""
import contextlib
import os
import time

import numpy as np
import torch

from . import train_ops as ops


_PACK_PLAN = os.environ.get("CALD_TRAIN_PACK_PLAN", "1") != "0"      # all trainable layers re-packed in two launches per step


def _bn_fold(sd, prefix, eps=1e-5):
    """FrozenBatchNorm2d as y = x * scale + shift (torchvision.ops.misc.FrozenBatchNorm2d, eps 1e-5 in 0.8.x)."""
    w, b = sd[prefix + ".weight"].double(), sd[prefix + ".bias"].double()
    rm, rv = sd[prefix + ".running_mean"].double(), sd[prefix + ".running_var"].double()
    scale = w * (rv + eps).rsqrt()
    return scale.float(), (b - rm * scale).float()


def choose_k(n, k, generator=None):
    """k distinct indices of range(n), every k-subset equally likely -- what ``torch.randperm(n)[:k]`` of torchvision's
    BalancedPositiveNegativeSampler selects, without permuting all n candidates (n is ~10^5 RPN negatives per image):
    sequential uniform draws from the CPU generator, repeats skipped."""
    if k >= n:
        return torch.arange(n)
    if 4 * k > n or n <= 8192:          # a few thousand candidates (the RoI sampler's): one permutation costs less than draw-and-dedupe
        return torch.randperm(n, generator=generator)[:k]
    got = np.empty(0, np.int64)
    while len(got) < k:
        draw = torch.randint(n, (2 * (k - len(got)) + 16,), generator=generator).numpy()
        allv = np.concatenate([got, draw])
        _, first = np.unique(allv, return_index=True)
        got = allv[np.sort(first)][:k]
    return torch.from_numpy(got)


class _LazyDict(dict):
    """A dict some of whose entries are computed on first use (zero-argument callables in `lazy`): what only tests and inspection read
    from the last forward (the proposals as a list, the sampled candidates per image, the RoI labels on the host) stays off the step's
    critical path -- the GPU is waiting while the forward's one host stop runs."""

    def __init__(self, lazy, **kw):
        super().__init__(**kw)
        self._lazy = dict(lazy)

    def __missing__(self, key):
        if key in self._lazy:
            self[key] = self._lazy.pop(key)()
            return self[key]
        raise KeyError(key)

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default


class _Conv(object):
    """One conv / linear layer of the graph: forward on the packed weight, backward = weight gradient + data gradient."""

    def __init__(self, net, wnames, bnames=None, bn=None, stride=1, pad=0, cin_k=None, out_ld=None, mode=0, taps=None):
        self.net, self.stride, self.pad, self.mode, self.taps = net, stride, pad, mode, taps
        self.w = net.merged(wnames)                     # torch-layout view (several adjacent parameters merged along dim 0)
        self.b = net.merged(bnames) if bnames else None
        self.gw = net.merged_grad(wnames)
        self.gb = net.merged_grad(bnames) if bnames else None
        self.trainable = self.gw is not None
        self.scale, self.shift = (None, None) if bn is None else net.bn[bn]
        if mode == 2:
            self.Cout, self.Cin, self.K = self.w.shape[0], self.w.shape[1] // taps, 1
        elif self.w.dim() == 2:
            self.Cout, self.Cin, self.K = self.w.shape[0], self.w.shape[1], 1
        else:
            self.Cout, self.Cin, self.K = self.w.shape[0], self.w.shape[1], self.w.shape[2]
        self.cin_k = cin_k if cin_k is not None else self.Cin
        self.out_ld = out_ld if out_ld is not None else self.Cout
        self._pk = self._pkd = None
        self._pk_version = self._pkd_version = -1
        self.x = None
        net.convs.append(self)

    def _packed(self):
        if self._pk is None or (self.trainable and self._pk_version != self.net.version):
            buf = self._pk.buf if self._pk is not None else None
            self._pk = ops.PackedConv(self.w, self.b, self.scale, self.shift, CinK=self.cin_k, mode=self.mode, taps=self.taps, out=buf)
            self._pk_version = self.net.version
            self._pkd_version = -1
        return self._pk

    def _plan_packs(self):
        """The forward and data-gradient PackedConv of a trainable layer for a PackPlan (allocated, not packed, on first use)."""
        if self._pk is None:
            self._pk = ops.PackedConv(self.w, self.b, self.scale, self.shift, CinK=self.cin_k, mode=self.mode, taps=self.taps, pack=False)
        if self._pkd is None:
            self._pkd = ops.PackedConv(self.w, scale=self.scale, CinK=self.out_ld, mode=3 if self.mode == 2 else 1, taps=self.taps, pack=False)
        return [self._pk, self._pkd]

    def _packed_grad(self):
        if self._pkd is None or self._pkd_version != self.net.version:
            buf = self._pkd.buf if self._pkd is not None else None
            # FrozenBatchNorm layers: the scale rides in the packed filter, so the incoming gradient is the one wrt the BN output
            self._pkd = ops.PackedConv(self.w, scale=self.scale, CinK=self.out_ld, mode=3 if self.mode == 2 else 1, taps=self.taps, out=buf)
            self._pkd_version = self.net.version
        return self._pkd

    def _count(self, x, passes):
        """algorithmic FLOPs of `passes` GEMM passes (forward, data gradient, weight gradient) over input x"""
        net = self.net
        if net.flops is not None:
            if self.mode == 2 or self.w.dim() == 2:
                rows, k = x.shape[2], self.w.shape[1]
            else:
                ho, wo = (x.shape[1] + 2 * self.pad - self.K) // self.stride + 1, (x.shape[2] + 2 * self.pad - self.K) // self.stride + 1
                rows, k = x.shape[0] * ho * wo, (3 if self.Cin == 4 else self.Cin) * self.K * self.K
            net.flops += 2.0 * rows * self.Cout * k * passes

    def fwd(self, x, relu=False, residual=None, up=None, out=None):
        if self.trainable:
            self.x = x
        self._count(x, 1)
        return ops.conv(x, self._packed(), stride=self.stride, pad=self.pad, relu=relu, residual=residual, up=up, out=out, out_ld=self.out_ld)

    def bwd(self, g, need_dx=True, residual=None, accumulate=False, x=None, mask=None, wgrad=True):
        """g: gradient wrt this layer's output AFTER its FrozenBatchNorm (if any) and after the ReLU mask, row stride out_ld: the BN
        scale is folded into the packed data-gradient filter and into the weight-gradient reduction.  mask: the saved post-ReLU
        activation the returned data gradient flows into (its ReLU backward is applied in the conv epilogue)."""
        x = self.x if x is None else x
        accumulate = accumulate or self.net.accumulate_grads
        self._count(x, int(bool(need_dx)) + int(bool(wgrad)))
        side, prev = self.net.side, ops._WGRAD_CTX[0]
        if wgrad:
            if side is not None:        # the weight gradient depends on (x, g) only: issue it beside the data gradient
                side[0].wait_stream(torch.cuda.current_stream(self.net.dev))
                x.record_stream(side[0]); g.record_stream(side[0])
                ops._WGRAD_CTX[0] = side[1]
            try:
                if self.mode == 2 or self.w.dim() == 2:
                    ops.linear_wgrad(x.view(g.shape[2], -1), g.view(g.shape[2], -1), self.Cout, self.gw, self.gb, taps=self.taps or 1, accumulate=accumulate)
                else:
                    ops.conv_wgrad(x, g, self.Cin, self.Cout, self.K, self.K, self.stride, self.pad, self.gw, self.gb, accumulate=accumulate,
                                   row_scale=self.scale)
            finally:
                ops._WGRAD_CTX[0] = prev
        if not need_dx:
            return None
        pkd = self._packed_grad()
        if self.mode == 2 or self.w.dim() == 2:
            return ops.conv(g, pkd, residual=residual, mask=mask)
        return ops.conv_dgrad(g, pkd, x.shape[1], x.shape[2], self.stride, self.pad, residual=residual, mask=mask)


class _Bottleneck(object):
    def __init__(self, net, prefix, stride, has_down, need_dx):
        self.c1 = _Conv(net, [prefix + ".conv1.weight"], bn=prefix + ".bn1")
        self.c2 = _Conv(net, [prefix + ".conv2.weight"], bn=prefix + ".bn2", stride=stride, pad=1)
        self.c3 = _Conv(net, [prefix + ".conv3.weight"], bn=prefix + ".bn3")
        self.down = _Conv(net, [prefix + ".downsample.0.weight"], bn=prefix + ".downsample.1", stride=stride) if has_down else None
        self.trainable, self.need_dx = self.c1.trainable, need_dx

    def fwd(self, x):
        self.a1 = self.c1.fwd(x, relu=True)
        self.a2 = self.c2.fwd(self.a1, relu=True)
        idt = self.down.fwd(x) if self.down is not None else x
        self.out = self.c3.fwd(self.a2, relu=True, residual=idt)
        return self.out

    def bwd(self, g, mask_input):
        """g: gradient wrt the block output with the block's final ReLU already applied backwards (g = dL/dout where out > 0, else 0).
        Returns the gradient wrt the block input x -- masked by x > 0 when `mask_input` (x is the previous block's post-ReLU output and
        nothing else is added to its gradient), unmasked otherwise -- or None when the input needs no gradient.  Every ReLU backward
        and FrozenBatchNorm scale of the block rides in a conv epilogue / packed filter: no elementwise pass."""
        ga2 = self.c3.bwd(g, mask=self.a2)
        ga1 = self.c2.bwd(ga2, mask=self.a1)
        x = self.c1.x
        if self.down is not None:
            if not self.need_dx:
                self.c1.bwd(ga1, need_dx=False); self.down.bwd(g, need_dx=False)
                return None
            gx = self.down.bwd(g)
            return self.c1.bwd(ga1, residual=gx, mask=x if mask_input else None)
        return self.c1.bwd(ga1, residual=g, mask=x if mask_input else None)


class _TrainerBase(object):
    """What the two detectors share: parameter storage, the ResNet body (forward + backward), input preparation."""
    LOSS_NAMES = ()
    MERGE_GROUPS = ()

    def _init_common(self, state_dict, num_classes, depth, min_size, max_size, device, trainable_layers, generator, sampler="choose_k"):
        if sampler not in ("choose_k", "randperm"):
            raise ValueError("sampler must be 'choose_k' or 'randperm', got %r" % (sampler,))
        self.sampler = sampler
        self.dev = torch.device(device)
        self.C, self.min_size, self.max_size = num_classes, int(min_size), int(max_size)
        self.generator = generator
        self.convs = []
        self.version = 0                                   # bumped whenever the parameters change: packed weights are rebuilt lazily
        sd = {k: (v.detach().float().cpu() if hasattr(v, "detach") else torch.from_numpy(np.asarray(v, np.float32)))
              for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        if not 0 <= trainable_layers <= 4:
            raise NotImplementedError("trainable_layers must be 0..4 (the reference uses torchvision's default 3; 5 would also train conv1)")
        frozen_layers = ["layer4", "layer3", "layer2", "layer1", "conv1"][trainable_layers:]
        def is_frozen(k):
            if ".bn" in k or "downsample.1" in k or k.startswith("backbone.body.bn1"):
                return True
            return k.startswith("backbone.body.") and any(k.startswith("backbone.body." + f) for f in frozen_layers + ["bn1"])
        # parameter storage: trainable tensors live in ONE flat buffer in state-dict order, so that tensors torchvision keeps
        # apart but the kernels treat as one matrix (RPN cls_logits + bbox_pred, predictor cls_score + bbox_pred) are adjacent
        self.names = [k for k in sd if not is_frozen(k)]
        self._merge_groups = [list(g) for g in self.MERGE_GROUPS]
        for a, b in self._merge_groups:
            self.names.remove(b)
            self.names.insert(self.names.index(a) + 1, b)
        sizes = [sd[k].numel() for k in self.names]
        pad = [(-s) % 4 for s in sizes]                    # keep every tensor 16-byte aligned...
        for grp in self._merge_groups:                     # ...except inside a merged group, which must be contiguous
            i = self.names.index(grp[0])
            assert self.names[i + 1] == grp[1], "state-dict order must keep %s adjacent" % grp
            pad[i] = 0
        offs, o = [], 0
        for s, p in zip(sizes, pad):
            offs.append(o); o += s + p
        self.flat = torch.zeros(o, dtype=torch.float32, device=self.dev)
        self.gflat = torch.zeros(o, dtype=torch.float32, device=self.dev)
        self._off = dict(zip(self.names, offs))
        self.params, self.grads, self.frozen = {}, {}, {}
        for k, off in zip(self.names, offs):
            v = self.flat[off:off + sd[k].numel()].view(sd[k].shape)
            v.copy_(sd[k])
            self.params[k] = torch.nn.Parameter(v, requires_grad=True)
            self.grads[k] = self.gflat[off:off + sd[k].numel()].view(sd[k].shape)
        for k in sd:
            if k not in self.params:
                self.frozen[k] = sd[k].to(self.dev)
        self.bn = {}
        for k in sd:
            if k.endswith(".running_var"):
                p = k[:-len(".running_var")]
                sc, sh = _bn_fold(sd, p)
                self.bn[p] = (sc.to(self.dev), sh.to(self.dev))
        # ---- graph ----
        w1 = self.frozen["backbone.body.conv1.weight"]
        self.frozen["__conv1_4ch"] = torch.cat([w1, torch.zeros_like(w1[:, :1])], dim=1).contiguous()      # the stem reads RGB0
        self.stem = _Conv(self, ["__conv1_4ch"], bn="backbone.body.bn1", stride=2, pad=3)
        nblocks = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}[depth]
        self.layers = []
        for li, nb in enumerate(nblocks):
            name = "layer%d" % (li + 1)
            trainable = name not in frozen_layers
            prev_trainable = li > 0 and ("layer%d" % li) not in frozen_layers
            blocks = [_Bottleneck(self, "backbone.body.%s.%d" % (name, b), stride=(2 if (b == 0 and li > 0) else 1), has_down=(b == 0),
                                  need_dx=(b > 0 or prev_trainable)) for b in range(nb)]
            self.layers.append((trainable, blocks))
        self._anchors = {}
        self.last = None
        self.timing = None          # set to a list to collect (section, wall-clock) marks of forward(); each mark synchronizes
        self.flops = None           # set to 0.0 to accumulate the algorithmic GEMM FLOPs of forward() + backward()
        self.accumulate_grads = False   # True: backward() adds to the flat gradient buffer (autograd's semantics when .grad is already set)
        # weight gradients run on a second stream: at batch 4 most layers fill a fraction of the 256 CUs, and dW / dX of one layer
        # are independent.  CALD_TRAIN_SIDE_STREAM=0 keeps everything on one stream.
        self.side = self.aux = None
        self._pack_plan = None
        self._roi_pin = None
        if os.environ.get("CALD_TRAIN_SIDE_STREAM", "1") != "0":
            from .detector import get_side_ctx
            st = torch.cuda.Stream(device=self.dev)
            di = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
            self.side = (st, get_side_ctx(di, st))
            # a third stream for what depends on the batch only (input upload, anchor matching, RPN sampling): its device->host copy
            # then waits for the match kernels, not for the previous step's backward still queued on the main stream
            st2 = torch.cuda.Stream(device=self.dev)
            self.aux = (st2, get_side_ctx(di, st2))

    def _join_side(self):
        if self.side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self.side[0])

    @contextlib.contextmanager
    def _aux_stream(self):
        """What the block issues goes to the batch-only stream and its context (to the current stream where there is none)."""
        if self.aux is None:
            yield
            return
        prev, ops._WGRAD_CTX[0] = ops._WGRAD_CTX[0], self.aux[1]
        try:
            with torch.cuda.stream(self.aux[0]):
                yield
        finally:
            ops._WGRAD_CTX[0] = prev

    # ---- parameter plumbing ----
    def _lookup(self, name):
        return self.params[name] if name in self.params else self.frozen[name]

    def merged(self, names):
        if names is None:
            return None
        if len(names) == 1:
            return self._lookup(names[0]).detach()
        first, n = self._lookup(names[0]).detach(), sum(self._lookup(k).numel() for k in names)
        rows = sum(self._lookup(k).shape[0] for k in names)
        return self.flat[self._off[names[0]]:self._off[names[0]] + n].view((rows,) + tuple(first.shape[1:]))

    def merged_grad(self, names):
        if names is None or names[0] not in self.params:
            return None
        first, n = self.params[names[0]], sum(self.params[k].numel() for k in names)
        rows = sum(self.params[k].shape[0] for k in names)
        return self.gflat[self._off[names[0]]:self._off[names[0]] + n].view((rows,) + tuple(first.shape[1:]))

    def parameters(self):
        return [self.params[k] for k in self.names]

    def named_parameters(self):
        return [(k, self.params[k]) for k in self.names]

    def state_dict(self):
        out = {k: v.detach().clone() for k, v in self.params.items()}
        out.update({k: v.clone() for k, v in self.frozen.items() if not k.startswith("__")})
        return out

    def parameters_changed(self):
        self.version += 1

    # ---- forward ----
    def _prepare_images(self, images):
        u8, rem = [], []
        for img in images:
            if img.dtype == torch.uint8:
                u8.append((img if img.shape[-1] == 3 else img.permute(1, 2, 0)).contiguous().to(self.dev)); rem.append(None)
                continue
            x = img.detach().to(torch.float32).to(self.dev).contiguous()
            g = (x * 255.0).round().clamp(0, 255).to(torch.uint8)
            from .detector import _u8_over_255
            r = x - _u8_over_255(x.device)[g.long()]
            u8.append(g.permute(1, 2, 0).contiguous()); rem.append(r.contiguous() if bool((r != 0).any()) else None)
        return u8, rem

    def anchors(self, Hp, Wp, level_hw):
        key = (Hp, Wp)
        if key not in self._anchors:
            if len(self._anchors) >= 16:                    # a few MB per padded batch size: keep the cache bounded over a long epoch
                self._anchors.pop(next(iter(self._anchors)))
            self._anchors[key] = ops.anchors(Hp, Wp, level_hw, self.dev, kind=self.ANCHOR_KIND)
        return self._anchors[key]

    def _sample(self, pos, neg, batch, frac):
        """BalancedPositiveNegativeSampler for one image: index tensors (CPU) of the sampled positives / negatives."""
        num_pos = min(int(batch * frac), pos.numel())
        num_neg = min(batch - num_pos, neg.numel())
        if self.sampler == "randperm":      # torchvision's own calls, in its order: positives first, then negatives
            perm_pos = torch.randperm(pos.numel(), generator=self.generator)[:num_pos]
            perm_neg = torch.randperm(neg.numel(), generator=self.generator)[:num_neg]
            return pos[perm_pos], neg[perm_neg]
        return pos[choose_k(pos.numel(), num_pos, self.generator)], neg[choose_k(neg.numel(), num_neg, self.generator)]

    def _fpn_out_fwd(self, inner):
        """The FPN output 3x3 convs (one weight per level) of all levels in one grouped launch."""
        for cv, x in zip(self.fout, inner):
            cv.x = x; cv._count(x, 1)
        return ops.conv_group(inner, [cv._packed() for cv in self.fout], pad=1)

    def _fpn_out_bwd(self, gP):
        """Weight gradients per level (side stream), data gradients of all levels in one grouped launch."""
        for cv, g in zip(self.fout, gP):
            cv.bwd(g, need_dx=False); cv._count(cv.x, 1)
        return ops.conv_group(gP, [cv._packed_grad() for cv in self.fout], pad=1)

    def _mark(self, name):
        if self.timing is not None:
            torch.cuda.synchronize(self.dev); self.timing.append((name, time.time()))

    def _repack(self):
        """Forward and data-gradient forms of every trainable weight, packed on the side stream while the main stream runs the
        frozen stem / layer 1 (the packs depend on the parameters only)."""
        if self.side is None:
            return
        st, ctx = self.side
        st.wait_stream(self._main)                          # the optimizer's update of the flat parameter buffer
        prev, ops._WGRAD_CTX[0] = ops._WGRAD_CTX[0], ctx
        try:
            with torch.cuda.stream(st):
                planned = [cv for cv in self.convs if cv.trainable] if _PACK_PLAN else []
                if planned:
                    # every layer's two forms in two launches: ~220 per-layer launches kept this stream busy for 1.5 ms, longer than
                    # the frozen layers cover (tools/train_event_timeline.py: layer 2 started 1.5 ms after the optimizer step)
                    if self._pack_plan is None:
                        self._pack_plan = ops.PackPlan([pk for cv in planned for pk in cv._plan_packs()], self.dev)
                    self._pack_plan.run()
                    for cv in planned:
                        cv._pk_version = cv._pkd_version = self.version
                for cv in self.convs:
                    if cv.trainable:
                        cv._packed(); cv._packed_grad()
        finally:
            ops._WGRAD_CTX[0] = prev
        self._packs_ready = torch.cuda.Event()
        self._packs_ready.record(st)

    def _begin_step(self):
        from .detector import get_ctx
        get_ctx(self.dev.index if self.dev.index is not None else torch.cuda.current_device())     # binds the main context to THIS stream on first use
        self._main = torch.cuda.current_stream(self.dev)
        self.version += 1                                  # whoever updated the parameters (any optimizer): repack the trainable layers
        self._repack()

    def _inputs(self, u8, rem, targets):
        """Host side of GeneralizedRCNNTransform: sizes, resized ground-truth boxes (device) and labels (host)."""
        sizes = [ops.transform_size(im.shape[0], im.shape[1], self.min_size, self.max_size) for im in u8]
        Hp, Wp = max(s[2] for s in sizes), max(s[3] for s in sizes)
        self.last_padded_hw = (Hp, Wp)
        img_sizes = [(s[0], s[1]) for s in sizes]
        gts, gt_labels = [], []
        for n_img, (im, s, t) in enumerate(zip(u8, sizes, targets)):      # resize_boxes: per-axis ratio in float32
            b = t["boxes"].detach().float().cpu().reshape(-1, 4)
            bad = (b[:, 2:] <= b[:, :2]).any(dim=1)                 # GeneralizedRCNN.forward's check (torchvision 0.8.2)
            if bool(bad.any()):
                j = int(torch.nonzero(bad)[0])
                raise ValueError("All bounding boxes should have positive height and width. Found invalid box %s for target at index %d."
                                 % (b[j].tolist(), n_img))
            rh = torch.tensor(s[0], dtype=torch.float32) / torch.tensor(im.shape[0], dtype=torch.float32)
            rw = torch.tensor(s[1], dtype=torch.float32) / torch.tensor(im.shape[1], dtype=torch.float32)
            gts.append(torch.stack([b[:, 0] * rw, b[:, 1] * rh, b[:, 2] * rw, b[:, 3] * rh], dim=1).to(self.dev).contiguous())
            gt_labels.append(t["labels"].detach().long().cpu().reshape(-1))
        self._mark("inputs")
        return u8, rem, Hp, Wp, img_sizes, gts, gt_labels

    def _body(self, u8, rem, Hp, Wp, img_sizes):
        """normalize + resize + pad on the device, stem, the four body stages.  Returns feats C2..C5."""
        x = ops.preprocess(u8, img_sizes, Hp, Wp, rem)
        x = ops.maxpool(self.stem.fwd(x, relu=True))
        self._mark("stem")
        feats = []
        waited = self.side is None
        for li, (trainable, blocks) in enumerate(self.layers):
            if trainable and not waited:                    # first layer that reads a freshly packed weight
                self._main.wait_event(self._packs_ready)
                waited = True
            for blk in blocks:
                x = blk.fwd(x)
            feats.append(x)
            if li < 3:
                self._mark("layer%d" % (li + 1))
        if not waited:
            self._main.wait_event(self._packs_ready)
        self._mark("body")
        return feats

    def _body_backward(self, gC):
        """gC[li]: gradient wrt the output of body layer li + 1 coming from the FPN laterals (None where there is none)."""
        g = None
        for li in (3, 2, 1, 0):
            trainable, blocks = self.layers[li]
            if not trainable:
                break
            if gC[li] is not None:
                g = gC[li] if g is None else ops.add(gC[li], g)
            ops.relu_bwd_(g, blocks[-1].out)                # the layer's last ReLU: the only elementwise pass of the layer
            if li < 3:
                self._mark("bwd layer%d" % (li + 2))
            for bi in range(len(blocks) - 1, -1, -1):
                # inside a layer the block input is the previous block's output and receives this gradient only: its ReLU backward is
                # fused; at the top of a layer the input also feeds an FPN lateral, whose gradient is added first (next iteration)
                g = blocks[bi].bwd(g, mask_input=bi > 0)

    def body_relu_decisions(self):
        out = {}
        nchw = lambda t: (t > 0).permute(0, 3, 1, 2).cpu()
        for li, (trainable, blocks) in enumerate(self.layers):
            for b, blk in enumerate(blocks):
                if trainable:
                    out.update({"layer%d.%d.a1" % (li + 1, b): nchw(blk.a1), "layer%d.%d.a2" % (li + 1, b): nchw(blk.a2), "layer%d.%d.out" % (li + 1, b): nchw(blk.out)})
        return out


class _Step(object):
    """What the stages of one FasterRCNNTrainer.forward hand to each other, named by the stage that sets it.  KEPT: the fields that
    become ``self.last`` (what backward(), the tests and the tools read of the last forward)."""
    __slots__ = ("N", "u8", "rem",
                 # RPN targets
                 "Hp", "Wp", "img_sizes", "gts", "gt_labels", "n_gt", "gt_off", "gt_labels_cat", "gts_all", "level_hw", "head_sizes",
                 "obj_idx", "obj_lab", "box_idx", "rpn_tgt", "rpn_samples",
                 # FPN + RPN head
                 "feats", "inner", "P", "tl", "heads", "head_flat",
                 # proposals
                 "props", "counts",
                 # RoI sampling
                 "R", "per_img", "rois", "labels", "pred_idx", "box_tgt", "roi_labels_np", "box_samples", "lazy",
                 # box head
                 "roi_rows", "f6", "f7", "pred")
    KEPT = ("N", "R", "feats", "inner", "P", "tl", "heads", "head_flat", "head_sizes", "level_hw", "obj_idx", "obj_lab", "box_idx", "rpn_tgt",
            "rois", "roi_rows", "f6", "f7", "pred", "labels", "pred_idx", "box_tgt")


class FasterRCNNTrainer(_TrainerBase):
    """The trainable mirror of detection/frcnn_la.py FRCNN_Feature (ResNet-50/101 FPN Faster R-CNN) on one MI355X."""
    LOSS_NAMES = ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")
    MERGE_GROUPS = (("rpn.head.cls_logits.weight", "rpn.head.bbox_pred.weight"), ("rpn.head.cls_logits.bias", "rpn.head.bbox_pred.bias"),
                    ("roi_heads.box_predictor.cls_score.weight", "roi_heads.box_predictor.bbox_pred.weight"),
                    ("roi_heads.box_predictor.cls_score.bias", "roi_heads.box_predictor.bbox_pred.bias"))
    ANCHOR_KIND = 0

    def __init__(self, state_dict, num_classes, depth=50, min_size=600, max_size=1000, device="cuda", trainable_layers=3,
                 rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=2000, rpn_nms_thresh=0.7, rpn_fg_iou=0.7, rpn_bg_iou=0.3,
                 rpn_batch=256, rpn_pos_fraction=0.5, box_fg_iou=0.5, box_bg_iou=0.5, box_batch=512, box_pos_fraction=0.25,
                 bbox_reg_weights=(10.0, 10.0, 5.0, 5.0), generator=None, sampler="choose_k", loss_mode=None):
        if loss_mode not in (None, "ll"):
            raise ValueError("loss_mode must be None or 'll', got %r" % (loss_mode,))
        # "ll": the learning-loss baseline's task model (detection/frcnn_ll.py): one loss per IMAGE (frcnn_ll.py:29-64, :243-276) and the
        # four pooled pyramid vectors LossNet reads (ll_train.py:77); None launches exactly what it always launched
        self.loss_mode = loss_mode
        self._init_common(state_dict, num_classes, depth, min_size, max_size, device, trainable_layers, generator, sampler)
        self.cfg = dict(pre_n=rpn_pre_nms_top_n, post_n=rpn_post_nms_top_n, nms=rpn_nms_thresh, rpn_fg=rpn_fg_iou, rpn_bg=rpn_bg_iou,
                        rpn_batch=rpn_batch, rpn_pos=rpn_pos_fraction, box_fg=box_fg_iou, box_bg=box_bg_iou, box_batch=box_batch,
                        box_pos=box_pos_fraction, w=tuple(bbox_reg_weights))
        self.lat = [_Conv(self, ["backbone.fpn.inner_blocks.%d.weight" % i], ["backbone.fpn.inner_blocks.%d.bias" % i]) for i in range(4)]
        self.fout = [_Conv(self, ["backbone.fpn.layer_blocks.%d.weight" % i], ["backbone.fpn.layer_blocks.%d.bias" % i], pad=1) for i in range(4)]
        self.rpn_conv = _Conv(self, ["rpn.head.conv.weight"], ["rpn.head.conv.bias"], pad=1)
        self.rpn_head = _Conv(self, self._merge_groups[0], self._merge_groups[1], out_ld=16)
        self.fc6 = _Conv(self, ["roi_heads.box_head.fc6.weight"], ["roi_heads.box_head.fc6.bias"], mode=2, taps=49)
        self.fc7 = _Conv(self, ["roi_heads.box_head.fc7.weight"], ["roi_heads.box_head.fc7.bias"])
        self.pred_ld = ops.round_up(5 * num_classes, 4)
        self.pred = _Conv(self, self._merge_groups[2], self._merge_groups[3], out_ld=self.pred_ld)
        assert self.pred.Cout == 5 * num_classes, "box predictor does not match num_classes"

    def forward(self, images, targets):
        """Training forward.  Returns the four losses as 1-element device tensors (no autograd) and keeps what backward needs.
        loss_mode "ll": returns ({name: [N] per-image losses}, pooled [N, 4, 256])."""
        s = _Step()
        s.N = len(images)
        self._mark("start")
        self._begin_step()
        s.u8, s.rem = self._prepare_images(images)          # on the main stream: the images may have just been produced there
        self._rpn_targets(s, targets)
        self._fpn_rpn_head(s)
        self._proposals(s)
        self._roi_sampling(s)
        self._box_head(s)
        return self._losses(s)

    def _rpn_targets(self, s, targets):
        """Stage 1, on the batch-only stream: input sizes, ground truth, anchor matching, the RPN sampler, the RPN loss kernels' index lists."""
        cfg, N = self.cfg, s.N
        with self._aux_stream():
            s.u8, s.rem, s.Hp, s.Wp, s.img_sizes, s.gts, s.gt_labels = self._inputs(s.u8, s.rem, targets)
            Hp, Wp, gts = s.Hp, s.Wp, s.gts
            # The RPN targets depend on the anchors and the ground truth only: match + sample them BEFORE the network is enqueued, so the
            # device->host copy of the match results does not wait for (and the host-side sampling does not stall) the body's kernels.
            level_hw = [(Hp // 4, Wp // 4), (Hp // 8, Wp // 8), (Hp // 16, Wp // 16), (Hp // 32, Wp // 32)]
            level_hw.append(((level_hw[3][0] - 1) // 2 + 1, (level_hw[3][1] - 1) // 2 + 1))
            head_sizes = [N * h * w * 16 for h, w in level_hw]
            anchors = self.anchors(Hp, Wp, level_hw)
            A_img = anchors.shape[0]
            # ---- RPN targets and sampling (anchor order: level, y, x, anchor).  One device->host copy of all match results, host-side
            # sampling (torch CPU generator), one host->device copy of every index the loss kernels need. ----
            lvl_start = np.cumsum([0] + [h * w * 3 for h, w in level_hw])
            head_off = np.cumsum([0] + head_sizes)
            lvl_pix = np.array([h * w for h, w in level_hw])
            def head_offsets(img, idx):                                  # float offset of anchor idx's objectness logit in head_flat
                l = np.searchsorted(lvl_start, idx, side="right") - 1
                rel = idx - lvl_start[l]
                pix, a = rel // 3, rel % 3
                return head_off[l] + (img * lvl_pix[l] + pix) * 16 + a, a
            n_gt = [int(g.shape[0]) for g in gts]
            gt_off = np.cumsum([0] + n_gt)
            s.gt_labels_cat = np.ascontiguousarray(torch.cat(s.gt_labels).numpy()) if sum(n_gt) else np.zeros(1, np.int64)
            s.gts_all = torch.cat(gts + [torch.zeros((1, 4), device=self.dev)])      # last row: the "matched box" of images without ground truth
            matched_dev = torch.full((N, A_img), -1, dtype=torch.int32, device=self.dev)
            for i in range(N):
                if n_gt[i]:
                    ops.match(anchors, gts[i], cfg["rpn_fg"], cfg["rpn_bg"], True, out=matched_dev[i])
            matched_all = matched_dev.cpu().numpy()
            obj_idx, obj_lab, box_idx, anc_idx, gt_idx = [], [], [], [], []
            s.rpn_samples = []
            for i in range(N):
                m = matched_all[i]
                pos, neg = torch.from_numpy(np.flatnonzero(m >= 0)), torch.from_numpy(np.flatnonzero(m == -1))
                sp, sn = self._sample(pos, neg, cfg["rpn_batch"], cfg["rpn_pos"])
                sp, sn = np.sort(sp.numpy()), np.sort(sn.numpy())
                s.rpn_samples.append((sp, sn))
                op_, ap_ = head_offsets(i, sp); on_, _ = head_offsets(i, sn)
                obj_idx += [op_, on_]; obj_lab += [np.ones(len(op_), np.float32), np.zeros(len(on_), np.float32)]
                box_idx.append(op_ - ap_ + 3 + 4 * ap_)                  # channel 3 + 4a of the same pixel
                anc_idx.append(sp); gt_idx.append(gt_off[i] + m[sp])
            obj_idx, box_idx, anc_idx, gt_idx = [np.concatenate(v).astype(np.int64) for v in (obj_idx, box_idx, anc_idx, gt_idx)]
            packed = torch.from_numpy(np.concatenate([obj_idx, box_idx, anc_idx, gt_idx])).to(self.dev)
            n_obj, n_pos = len(obj_idx), len(box_idx)
            s.obj_idx, s.box_idx = packed[:n_obj], packed[n_obj:n_obj + n_pos]
            anc_sel, gt_sel = packed[n_obj + n_pos:n_obj + 2 * n_pos], packed[n_obj + 2 * n_pos:]
            s.obj_lab = torch.from_numpy(np.concatenate(obj_lab)).to(self.dev)
            s.rpn_tgt = ops.box_encode(s.gts_all[gt_sel], anchors[anc_sel], (1.0, 1.0, 1.0, 1.0))
            s.level_hw, s.head_sizes, s.n_gt, s.gt_off = level_hw, head_sizes, n_gt, gt_off
            self._mark("rpn targets")
        if self.aux is not None:                            # what the main stream consumes from the batch-only stream
            self._main.wait_stream(self.aux[0])
            for t in list(gts) + [s.gts_all, packed, s.obj_lab, s.rpn_tgt]:
                t.record_stream(self._main)

    def _fpn_rpn_head(self, s):
        """Stage 2: body, FPN (top-down), LastLevelMaxPool, the RPN head on the five levels."""
        N = s.N
        s.feats = feats = self._body(s.u8, s.rem, s.Hp, s.Wp, s.img_sizes)
        s.inner = inner = [None] * 4
        inner[3] = self.lat[3].fwd(feats[3])
        for i in (2, 1, 0):
            inner[i] = self.lat[i].fwd(feats[i], up=inner[i + 1])
        s.P = P = self._fpn_out_fwd(inner)
        P.append(ops.subsample2(P[3]))
        assert s.level_hw == [(p.shape[1], p.shape[2]) for p in P]
        # RPN head on the five levels: outputs in ONE buffer so that the loss kernels address (level, pixel, channel) by offset
        s.head_flat = torch.zeros(sum(s.head_sizes), dtype=torch.float32, device=self.dev)
        s.heads, o = [], 0
        s.tl = tl = ops.conv_group(P, self.rpn_conv._packed(), pad=1, relu=True)     # shared 3x3 conv on the five levels: one launch
        for i, (h, w) in enumerate(s.level_hw):
            s.heads.append(ops.conv(tl[i], self.rpn_head._packed(), out=s.head_flat[o:o + s.head_sizes[i]].view(N, h, w, 16), out_ld=16))
            self.rpn_conv._count(P[i], 1); self.rpn_head._count(tl[i], 1)
            o += s.head_sizes[i]
        self._mark("fpn+rpn head")

    def _proposals(self, s):
        """Stage 3: the RPN's proposals, a fixed [N, post_n, 4] block and the number of used rows per image, both left on the device."""
        cfg = self.cfg
        s.props, s.counts = ops.rpn_proposals(s.heads, s.Hp, s.Wp, s.img_sizes, cfg["pre_n"], cfg["post_n"], cfg["nms"], 1e-3)
        self._mark("proposals")

    def _roi_sampling(self, s):
        """Stage 4: the RoI heads' candidates matched on the device, labelled and sampled on the host (the forward's ONE host stop after
        the RPN's): RoIAlign's rows, their labels and regression targets, the loss kernels' index lists."""
        cfg, N, n_gt, props = self.cfg, s.N, s.n_gt, s.props
        # The proposal counts are not waited for.  The RoI candidates are matched in a fixed-row table (image i: its post_n proposal
        # slots, used or not, then its ground truth) and the counts travel to the host in the same copy as the match results; unused
        # slots are dropped there.
        post = int(props.shape[1])
        pr_off = np.cumsum([0] + [post + g for g in n_gt])
        T = int(pr_off[-1])
        pr_all = torch.cat([t for i in range(N) for t in ((props[i], s.gts[i]) if n_gt[i] else (props[i],))]).contiguous()
        matched_dev = torch.full((T + N,), -1, dtype=torch.int32, device=self.dev)
        for i in range(N):
            if n_gt[i]:
                ops.match(pr_all[pr_off[i]:pr_off[i + 1]], s.gts[i], cfg["box_fg"], cfg["box_bg"], False, out=matched_dev[pr_off[i]:pr_off[i + 1]])
        matched_dev[T:] = s.counts.to(torch.int32)
        matched_all = matched_dev.cpu().numpy()
        # ---- the GPU waits from here to the host->device copy of the sampler: everything in between is host time on the step's critical path ----
        counts = matched_all[T:]
        sample = self._sample_rois_choose_k if self.sampler == "choose_k" else self._sample_rois_randperm
        sample(s, pr_all, pr_off, matched_all, counts)
        # what only tests and inspection read: the proposals as a list, the RoI labels on the host
        s.lazy = {"proposals": lambda c=counts.copy(): [props[i, :int(c[i])] for i in range(N)],
                  "roi_labels": lambda l=s.roi_labels_np: torch.from_numpy(np.ascontiguousarray(l))}
        self._mark("roi sampling")

    def _sample_rois_choose_k(self, s, pr_all, pr_off, matched_all, counts):
        """One C call for the whole batch (cald_train_roi_sample_host): labels, the balanced sampler (the k smallest of iid uniform keys
        per class -- one generator call for all images, one key per table row), every index list of the loss kernels, written into
        pinned memory and uploaded as one block; one kernel (cald_train_roi_gather) then builds RoIAlign's rows and the regression
        targets.  The numpy loop of the other sampler + eight small torch ops cost 0.6 ms of GPU idle per step."""
        cfg, N, post = self.cfg, s.N, int(s.props.shape[1])
        keys = torch.rand(sum(post + g for g in s.n_gt), generator=self.generator, dtype=torch.float64).numpy()
        cap = N * cfg["box_batch"]
        if self._roi_pin is None or self._roi_pin.numel() < 6 * cap:
            self._roi_pin = torch.empty(6 * cap, dtype=torch.int64, pin_memory=True)
        pin_np = self._roi_pin.numpy()
        _, _, R, n_posrows, per_img = ops.roi_sample_host([post] * N, s.n_gt, counts, matched_all, s.gt_labels_cat, keys, cfg["box_batch"], cfg["box_pos"],
                                                          self.pred_ld, self.C, out=pin_np)
        packed2 = torch.empty(6 * cap, dtype=torch.int64, device=self.dev)
        packed2.copy_(self._roi_pin[:6 * cap], non_blocking=True)       # the pinned block is rewritten only after the next step's stop
        s.rois, s.box_tgt = ops.roi_gather(pr_all, s.gts_all, packed2, cap, R, n_posrows, cfg["w"])
        s.R, s.per_img = R, per_img
        s.labels, s.pred_idx = packed2[2 * cap:2 * cap + R], packed2[3 * cap:3 * cap + n_posrows]
        keep_np, s.roi_labels_np = pin_np[:R].copy(), pin_np[2 * cap:2 * cap + R].copy()
        def box_samples(keep=keep_np, lab=s.roi_labels_np, per_img=per_img, cn=counts.copy(), pr_off=pr_off.copy()):
            out, o = [], 0
            for i in range(N):                      # table row -> compact candidate number (used proposals, then the ground truth)
                r = keep[o:o + per_img[i]] - pr_off[i]
                c = np.where(r < post, r, r - post + int(cn[i]))
                l = lab[o:o + per_img[i]]
                out.append((c[l > 0], c[l == 0])); o += per_img[i]
            return out
        s.box_samples = box_samples

    def _sample_rois_randperm(self, s, pr_all, pr_off, matched_all, counts):
        """torchvision's own sampler calls image by image (_sample) on the compact candidate list of each image -- its used proposals,
        then its ground truth -- with the index lists and targets put together by numpy and small torch ops."""
        cfg, N, n_gt, post = self.cfg, s.N, s.n_gt, int(s.props.shape[1])
        # compact candidate number -> row of the fixed-row table (the used proposal slots, then the ground truth)
        rowmap = [np.concatenate([np.arange(int(counts[i])), post + np.arange(n_gt[i])]).astype(np.int64) for i in range(N)]
        keep_all, lab_all, gtsel_all, img_col, box_samples = [], [], [], [], []
        for i in range(N):
            m = matched_all[pr_off[i]:pr_off[i + 1]][rowmap[i]]
            if n_gt[i]:
                labels = s.gt_labels[i].numpy()[np.maximum(m, 0)].copy()
                labels[m == -1] = 0
                labels[m == -2] = -1
            else:
                labels = np.zeros(len(m), np.int64)
            pos, neg = torch.from_numpy(np.flatnonzero(labels >= 1)), torch.from_numpy(np.flatnonzero(labels == 0))
            sp, sn = self._sample(pos, neg, cfg["box_batch"], cfg["box_pos"])
            box_samples.append((np.sort(sp.numpy()), np.sort(sn.numpy())))
            keep = np.sort(np.concatenate([sp.numpy(), sn.numpy()]))
            keep_all.append(pr_off[i] + rowmap[i][keep]); lab_all.append(labels[keep])
            gtsel_all.append(s.gt_off[i] + np.maximum(m[keep], 0) if n_gt[i] else np.full(len(keep), s.gt_off[-1], np.int64))
            img_col.append(np.full(len(keep), float(i), np.float32))
        s.roi_labels_np = roi_labels_np = np.concatenate(lab_all).astype(np.int64)
        s.per_img = [len(l) for l in lab_all]
        s.R = R = len(roi_labels_np)
        pos_rows = np.flatnonzero(roi_labels_np > 0)
        n_posrows = len(pos_rows)
        pred_idx_np = pos_rows * self.pred_ld + self.C + 4 * roi_labels_np[pos_rows]
        packed2 = torch.from_numpy(np.concatenate([np.concatenate(keep_all), np.concatenate(gtsel_all), roi_labels_np, pred_idx_np, pos_rows]).astype(np.int64)).to(self.dev)
        img_col_dev = torch.from_numpy(np.concatenate(img_col)).to(self.dev)
        keep_sel, gt_sel2, s.labels = packed2[:R], packed2[R:2 * R], packed2[2 * R:3 * R]
        s.pred_idx, pos_sel = packed2[3 * R:3 * R + n_posrows], packed2[3 * R + n_posrows:3 * R + 2 * n_posrows]
        boxes = pr_all[keep_sel]
        s.rois = torch.cat([img_col_dev[:, None], boxes], dim=1).contiguous()
        roi_gt = s.gts_all[gt_sel2]
        s.box_tgt = ops.box_encode(roi_gt.contiguous(), boxes.contiguous(), cfg["w"])[pos_sel].contiguous()
        s.box_samples = lambda: box_samples

    def _box_head(self, s):
        """Stage 5: RoIAlign, the two-layer head, the predictor; the step's record for backward() and inspection."""
        s.roi_rows = ops.roi_align(s.P[:4], s.rois)
        s.f6 = self.fc6.fwd(s.roi_rows.view(1, 1, s.R, -1), relu=True)
        s.f7 = self.fc7.fwd(s.f6, relu=True)
        s.pred = self.pred.fwd(s.f7)
        self.last = _LazyDict(s.lazy, samples=_LazyDict({"box": s.box_samples}, rpn=s.rpn_samples), **{k: getattr(s, k) for k in _Step.KEPT})
        self._mark("box head")

    def _losses(self, s):
        """Stage 6: the four losses -- per batch, or per image with the pooled pyramid vectors in loss_mode "ll"."""
        L, N = self.last, s.N
        if self.loss_mode == "ll":
            # per-image segments of the index lists (they are built image by image) and the reference's normalisers
            L["rpn_cnt"] = [len(sp) + len(sn) for sp, sn in s.rpn_samples]
            L["rpn_pos_cnt"] = [len(sp) for sp, _ in s.rpn_samples]
            L["roi_cnt"] = [int(v) for v in s.per_img]
            edges = np.cumsum([0] + L["roi_cnt"])
            L["roi_pos_cnt"] = [int((s.roi_labels_np[edges[i]:edges[i + 1]] > 0).sum()) for i in range(N)]
            losses = self._ll_losses(L)
            L["pooled"] = ops.train_gap(s.P[:4])        # the batch's PADDED maps, as frcnn_ll.py:601-602 pools them
            self._mark("losses")
            return losses, L["pooled"]
        losses = {
            "loss_classifier": ops.softmax_ce(s.pred.view(s.R, -1), s.labels, self.C),
            "loss_box_reg": ops.smooth_l1(s.pred, s.pred_idx, s.box_tgt, 1.0 / 9, s.R),
            "loss_objectness": ops.bce_logits(s.head_flat, s.obj_idx, s.obj_lab),
            "loss_rpn_box_reg": ops.smooth_l1(s.head_flat, s.box_idx, s.rpn_tgt, 1.0 / 9, s.obj_idx.numel()),
        }
        self._mark("losses")
        return losses

    def _ll_losses(self, L, gs=None, gpred=None, ghead=None, which=(0, 1, 2, 3)):
        """The per-image task losses of loss_mode "ll" in the reference's dict order: cross entropy = mean over image i's sampled rows,
        box loss = smooth_l1(beta 1, sum) / R_i (frcnn_ll.py:48-61), objectness = BCE mean over image i's sampled anchors, RPN box loss
        = L1 sum / (sampled anchors of image i) (frcnn_ll.py:267-273).  gs [4, N] (device): per-image gradient scales, with gpred /
        ghead the zeroed gradient buffers the kernels write into."""
        g = (lambda i: None) if gs is None else (lambda i: gs[i])
        R = L["R"]
        out = {}
        if 0 in which:
            out["loss_classifier"] = ops.softmax_ce_seg(L["pred"].view(R, -1), L["labels"], self.C, L["roi_cnt"], grad=gpred, gscale=g(0))
        if 1 in which:
            out["loss_box_reg"] = ops.smooth_l1_seg(L["pred"], L["pred_idx"], L["box_tgt"], 1.0, L["roi_pos_cnt"], L["roi_cnt"], grad=gpred, gscale=g(1))
        if 2 in which:
            out["loss_objectness"] = ops.bce_logits_seg(L["head_flat"], L["obj_idx"], L["obj_lab"], L["rpn_cnt"], grad=ghead, gscale=g(2))
        if 3 in which:
            out["loss_rpn_box_reg"] = ops.smooth_l1_seg(L["head_flat"], L["box_idx"], L["rpn_tgt"], 0.0, L["rpn_pos_cnt"], L["rpn_cnt"], grad=ghead, gscale=g(3))
        return out

    def relu_decisions(self):
        """{name: bool NCHW / [R, C] CPU tensor}: which side every ReLU of the last forward's differentiated part took (for
        gradient checks against a higher-precision restatement, which must take the same branches)."""
        L, out = self.last, self.body_relu_decisions()
        nchw = lambda t: (t > 0).permute(0, 3, 1, 2).cpu()
        for i, t in enumerate(L["tl"]):
            out["rpn.%d" % i] = nchw(t)
        out["fc6"] = (L["f6"] > 0).view(L["R"], -1).cpu(); out["fc7"] = (L["f7"] > 0).view(L["R"], -1).cpu()
        return out

    def _rpn_branch_weights(self, L, g_obj, g_reg):
        """First half of the RPN branch: RPN losses -> gradient of the 1x1 head's output -> the weight gradients of the head and of the
        3x3 conv (shared weights: they accumulate over the five levels) and the head's data gradient (with the conv's ReLU backward).
        Returns that gradient per level -- what the 3x3 conv's data gradient (_rpn_branch_data) starts from."""
        N, P, level_hw = L["N"], L["P"], L["level_hw"]
        ghead_flat = torch.zeros_like(L["head_flat"])
        if self.loss_mode == "ll":                           # g_obj: the [4, N] per-image scales
            self._ll_losses(L, gs=g_obj, ghead=ghead_flat, which=(2, 3))
        else:
            ops.bce_logits(L["head_flat"], L["obj_idx"], L["obj_lab"], grad=ghead_flat, gscale=g_obj)
            ops.smooth_l1(L["head_flat"], L["box_idx"], L["rpn_tgt"], 1.0 / 9, L["obj_idx"].numel(), grad=ghead_flat, gscale=g_reg)
        o, ghs = 0, []
        for i, (h, w) in enumerate(level_hw):
            ghs.append(ghead_flat[o:o + L["head_sizes"][i]].view(N, h, w, 16)); o += L["head_sizes"][i]
            self.rpn_head.bwd(ghs[i], need_dx=False, accumulate=i > 0, x=L["tl"][i])
            self.rpn_head._count(L["tl"][i], 1)
        gts_ = ops.conv_group(ghs, self.rpn_head._packed_grad(), masks=L["tl"])       # 1x1 head: data gradient of the five levels + ReLU backward, one launch
        for i in range(5):
            self.rpn_conv.bwd(gts_[i], need_dx=False, accumulate=i > 0, x=P[i])
        return gts_

    def _rpn_branch_data(self, L, gts_):
        """Second half: the 3x3 conv's data gradient on the five levels -> gradients wrt P2..P5 and the pooled level."""
        P = L["P"]
        for i in range(5):
            self.rpn_conv._count(P[i], 1)
        g = ops.conv_group(gts_, self.rpn_conv._packed_grad(), pad=1)       # the five levels in one launch, like the forward
        return g[:4], g[4]

    # ---- backward ----
    def backward(self, gscale=(1.0, 1.0, 1.0, 1.0), g_pooled=None):
        """Gradients of sum_i gscale[i] * loss_i (order: classifier, box_reg, objectness, rpn_box_reg) into the flat gradient buffer.
        loss_mode "ll": gscale is [4][N] (a float or a sequence per loss, or a device tensor) -- one scale per loss and image -- and
        g_pooled (optional, [N, 4, 256]) the gradient LossNet sends into the pooled pyramid vectors; it joins the pyramid's gradient
        inside the kernel that adds the RPN branch's and the box head's maps, so the maps are not passed over again."""
        L = self.last
        ll = self.loss_mode == "ll"
        if ll:
            if not torch.is_tensor(gscale):
                gscale = torch.tensor([[float(v)] * L["N"] if not hasattr(v, "__len__") else [float(x) for x in v] for v in gscale],
                                      dtype=torch.float32)
            gscale = gscale.to(self.dev, torch.float32).contiguous()
            assert tuple(gscale.shape) == (4, L["N"]), "gscale must be [4][N] in loss_mode 'll'"
            if g_pooled is not None:
                g_pooled = g_pooled.to(torch.float32).contiguous()
                assert tuple(g_pooled.shape) == tuple(L["pooled"].shape)
        elif g_pooled is not None:
            raise ValueError("g_pooled belongs to loss_mode 'll'")
        N, R, P, level_hw = L["N"], L["R"], L["P"], L["level_hw"]
        # The box-head branch (predictor -> fc7 -> fc6 -> RoIAlign backward) and the RPN branch meet only at the FPN outputs: the former
        # is issued on the batch-only stream (idle during the backward pass), the latter on the main stream.
        aux = self.aux
        main = torch.cuda.current_stream(self.dev)
        if aux is not None:
            aux[0].wait_stream(main)
        with self._aux_stream():
            gpred = torch.zeros_like(L["pred"])
            if ll:
                self._ll_losses(L, gs=gscale, gpred=gpred.view(R, -1), which=(0, 1))
            else:
                ops.softmax_ce(L["pred"].view(R, -1), L["labels"], self.C, grad=gpred, gscale=gscale[0])
                ops.smooth_l1(L["pred"], L["pred_idx"], L["box_tgt"], 1.0 / 9, R, grad=gpred, gscale=gscale[1])
            g7 = self.pred.bwd(gpred, mask=L["f7"])
            g6 = self.fc7.bwd(g7, mask=L["f6"])
            groi = self.fc6.bwd(g6)
            gP_roi = [torch.zeros_like(p) for p in P[:4]]
            ops.roi_align_bwd_(gP_roi, L["rois"], groi.view(R, 49, -1))
            self._mark("bwd box head (aux)")
        gts_ = self._rpn_branch_weights(L, gscale, None) if ll else self._rpn_branch_weights(L, gscale[2], gscale[3])
        gP, gpool = self._rpn_branch_data(L, gts_)      # on the main stream, beside the box-head branch on the batch-only stream
        self._mark("bwd rpn branch")
        if aux is not None:
            main.wait_stream(aux[0])
            for t in gP_roi:
                t.record_stream(main)
        if g_pooled is not None:
            # LossNet's gradient of level l is g_pooled[n][l][c] / (H_l W_l) at every pixel: it rides in the join of the two branches
            gP = [ops.add_bcast(gP[i], gP_roi[i], g_pooled[:, i, :]) for i in range(4)]
        else:
            gP = [ops.add(gP[i], gP_roi[i]) for i in range(4)]
        gP[3] = ops.add(gP[3], ops.dilate(gpool, 2, P[3].shape[1], P[3].shape[2]))          # LastLevelMaxPool (kernel 1, stride 2)
        # FPN
        ginner = self._fpn_out_bwd(gP[:4])
        for i in range(1, 4):
            ops.upsample_bwd_(ginner[i - 1], ginner[i])
        gC = [None] * 4
        for i in range(4):
            need = self.layers[i][0]                                                       # the body layer producing feats[i] is trainable
            gC[i] = self.lat[i].bwd(ginner[i], need_dx=need)
        self._mark("bwd fpn")
        self._body_backward(gC)
        self._mark("bwd body dgrad")
        self._join_side()
        return self.grads


class RetinaNetTrainer(_TrainerBase):
    """The trainable mirror of detection/retinanet_cal.py RetinaNet (ResNet-50 FPN, P3-P7, 9 anchors per location): training forward
    :545-564, matcher :389-400 (IoU 0.5 / 0.4, low-quality matches), classification loss :100-133 (sigmoid focal loss, sum over the
    anchors outside the ignore band / max(1, #foreground), mean over images), regression loss :185-221 (L1 on the foreground
    anchors / max(1, #foreground), mean over images).  As in the reference, every image must carry at least one box."""
    LOSS_NAMES = ("classification", "bbox_regression")
    ANCHOR_KIND = 1

    def __init__(self, state_dict, num_classes, depth=50, min_size=600, max_size=1000, device="cuda", trainable_layers=3,
                 fg_iou_thresh=0.5, bg_iou_thresh=0.4, generator=None, loss_mode=None):
        if loss_mode is not None:
            raise NotImplementedError("loss_mode=%r: training LossNet beside a RetinaNet (ll_train.py:97-120, retina_ll.py's per-image "
                                      "losses) is outside the scope of the learning-loss training step, which covers Faster R-CNN" % (loss_mode,))
        self.loss_mode = None
        self._init_common(state_dict, num_classes, depth, min_size, max_size, device, trainable_layers, generator)
        self.cfg = dict(fg=fg_iou_thresh, bg=bg_iou_thresh)
        cin = [None, 0, 1, 2]                                    # body layer index -> FPN block index (returned_layers = [2, 3, 4])
        self.lat = [_Conv(self, ["backbone.fpn.inner_blocks.%d.weight" % i], ["backbone.fpn.inner_blocks.%d.bias" % i]) for i in range(3)]
        self.fout = [_Conv(self, ["backbone.fpn.layer_blocks.%d.weight" % i], ["backbone.fpn.layer_blocks.%d.bias" % i], pad=1) for i in range(3)]
        self.p6 = _Conv(self, ["backbone.fpn.extra_blocks.p6.weight"], ["backbone.fpn.extra_blocks.p6.bias"], stride=2, pad=1)
        self.p7 = _Conv(self, ["backbone.fpn.extra_blocks.p7.weight"], ["backbone.fpn.extra_blocks.p7.bias"], stride=2, pad=1)
        tower = lambda head: [_Conv(self, ["head.%s.conv.%d.weight" % (head, 2 * j)], ["head.%s.conv.%d.bias" % (head, 2 * j)], pad=1) for j in range(4)]
        self.cls_tower, self.reg_tower = tower("classification_head"), tower("regression_head")
        self.K = num_classes
        self.cls_ld = ops.round_up(9 * num_classes, 4)
        self.cls_out = _Conv(self, ["head.classification_head.cls_logits.weight"], ["head.classification_head.cls_logits.bias"], pad=1, out_ld=self.cls_ld)
        self.reg_out = _Conv(self, ["head.regression_head.bbox_reg.weight"], ["head.regression_head.bbox_reg.bias"], pad=1)
        assert self.cls_out.Cout == 9 * num_classes and self.reg_out.Cout == 36, "RetinaNet heads must have 9 * num_classes / 36 outputs"

    def forward(self, images, targets):
        N, K, mark = len(images), self.K, self._mark
        mark("start")
        self._begin_step()
        u8, rem = self._prepare_images(images)              # on the main stream: the images may have just been produced there
        # Everything that depends on the batch only (ground-truth upload, anchor matching, regression targets) goes first, on its own
        # stream: the device->host copy of the match results then does not wait for the network's kernels.
        with self._aux_stream():
            u8, rem, Hp, Wp, img_sizes, gts, gt_labels = self._inputs(u8, rem, targets)
            if any(g.shape[0] == 0 for g in gts):
                raise ValueError("RetinaNet training needs at least one ground-truth box per image (retinanet_cal.py:110-124)")
            level_hw = [(Hp // 8, Wp // 8), (Hp // 16, Wp // 16), (Hp // 32, Wp // 32)]
            for _ in range(2):                              # P6, P7: 3x3 stride-2 convs with padding 1
                level_hw.append(((level_hw[-1][0] - 1) // 2 + 1, (level_hw[-1][1] - 1) // 2 + 1))
            level_pix = [h * w for h, w in level_hw]
            cls_sizes, reg_sizes = [N * n * self.cls_ld for n in level_pix], [N * n * 36 for n in level_pix]
            anchors = self.anchors(Hp, Wp, level_hw)
            A_tot = anchors.shape[0]
            matched_dev = torch.empty((N, A_tot), dtype=torch.int32, device=self.dev)
            for i in range(N):
                ops.match(anchors, gts[i], self.cfg["fg"], self.cfg["bg"], True, out=matched_dev[i])
            matched_all = matched_dev.cpu().numpy()
            n_gt = [int(g.shape[0]) for g in gts]
            gt_off = np.cumsum([0] + n_gt)
            gts_all = torch.cat(gts)
            lvl_start = np.cumsum([0] + [n * 9 for n in level_pix])
            reg_off = np.cumsum([0] + reg_sizes)
            lvl_pix = np.array(level_pix)
            box_idx, anc_idx, gt_idx, wts, nfg = [], [], [], [], []
            for i in range(N):
                m = matched_all[i]
                fg = np.flatnonzero(m >= 0)
                l = np.searchsorted(lvl_start, fg, side="right") - 1
                rel = fg - lvl_start[l]
                pix, a = rel // 9, rel % 9
                box_idx.append(reg_off[l] + (i * lvl_pix[l] + pix) * 36 + 4 * a)
                anc_idx.append(fg); gt_idx.append(gt_off[i] + m[fg])
                nfg.append(len(fg)); wts.append(np.full(len(fg), 1.0 / (max(1, len(fg)) * N), np.float32))
            box_idx, anc_idx, gt_idx = [np.concatenate(v).astype(np.int64) for v in (box_idx, anc_idx, gt_idx)]
            packed = torch.from_numpy(np.concatenate([box_idx, anc_idx, gt_idx])).to(self.dev)
            nb = len(box_idx)
            box_idx, anc_sel, gt_sel = packed[:nb], packed[nb:2 * nb], packed[2 * nb:]
            fl = torch.from_numpy(np.concatenate([np.concatenate(wts), np.array([1.0 / (max(1, n) * N) for n in nfg], np.float32)])).to(self.dev)
            box_w, img_w = fl[:nb], fl[nb:]
            reg_tgt = ops.box_encode(gts_all[gt_sel], anchors[anc_sel], (1.0, 1.0, 1.0, 1.0))
            gt_labels_dev = torch.cat(gt_labels).to(self.dev)
            gt_off_dev = torch.from_numpy(gt_off.astype(np.int32)).to(self.dev)
        if self.aux is not None:
            self._main.wait_stream(self.aux[0])
            for t in list(gts) + [gts_all, packed, fl, reg_tgt, matched_dev, gt_labels_dev, gt_off_dev]:
                t.record_stream(self._main)
        mark("targets")
        feats = self._body(u8, rem, Hp, Wp, img_sizes)
        inner = [None] * 3
        inner[2] = self.lat[2].fwd(feats[3])
        for i in (1, 0):
            inner[i] = self.lat[i].fwd(feats[i + 1], up=inner[i + 1])
        P = self._fpn_out_fwd(inner)
        P.append(self.p6.fwd(P[2]))
        p6_relu = ops.relu_bwd_(ops.add(P[3]), P[3])                       # relu(p6): x * (x > 0) on a copy
        P.append(self.p7.fwd(p6_relu))
        assert level_hw == [(p.shape[1], p.shape[2]) for p in P]
        # head outputs of the five levels in ONE buffer each (level block l = [N][pix_l][ld])
        cls_flat = torch.zeros(sum(cls_sizes), dtype=torch.float32, device=self.dev)
        reg_flat = torch.empty(sum(reg_sizes), dtype=torch.float32, device=self.dev)
        # both towers on the five levels: ten problems of one shape per launch (the small levels fill the tail of the large ones)
        acts = {"cls": [[P[l]] for l in range(5)], "reg": [[P[l]] for l in range(5)]}
        for j in range(4):
            xs = [acts["cls"][l][-1] for l in range(5)] + [acts["reg"][l][-1] for l in range(5)]
            ys = ops.conv_group(xs, [self.cls_tower[j]._packed()] * 5 + [self.reg_tower[j]._packed()] * 5, pad=1, relu=True)
            for l in range(5):
                self.cls_tower[j]._count(xs[l], 1); self.reg_tower[j]._count(xs[5 + l], 1)
                acts["cls"][l].append(ys[l]); acts["reg"][l].append(ys[5 + l])
        oc = orr = 0
        cls_views, reg_views = [], []
        for l, (h, w) in enumerate(level_hw):
            cls_views.append(cls_flat[oc:oc + cls_sizes[l]].view(N, h, w, self.cls_ld)); reg_views.append(reg_flat[orr:orr + reg_sizes[l]].view(N, h, w, 36))
            oc += cls_sizes[l]; orr += reg_sizes[l]
            self.cls_out._count(acts["cls"][l][4], 1); self.reg_out._count(acts["reg"][l][4], 1)
        ops.conv_group([acts["cls"][l][4] for l in range(5)], self.cls_out._packed(), pad=1, outs=cls_views, out_ld=self.cls_ld)
        ops.conv_group([acts["reg"][l][4] for l in range(5)], self.reg_out._packed(), pad=1, outs=reg_views, out_ld=36)
        mark("fpn+heads")
        self.last = dict(N=N, P=P, p6_relu=p6_relu, feats=feats, inner=inner, acts=acts, level_hw=level_hw, level_pix=level_pix, cls_flat=cls_flat, reg_flat=reg_flat,
                         cls_sizes=cls_sizes, reg_sizes=reg_sizes, matched=matched_dev, gt_labels=gt_labels_dev, gt_off=gt_off_dev, img_w=img_w, box_idx=box_idx,
                         box_w=box_w, reg_tgt=reg_tgt, matched_host=matched_all)
        losses = {"classification": ops.focal_loss(cls_flat, level_pix, N, 9, K, self.cls_ld, matched_dev, gt_labels_dev, gt_off_dev, img_w),
                  "bbox_regression": ops.smooth_l1(reg_flat, box_idx, reg_tgt, 0.0, 1.0, weights=box_w)}
        mark("losses")
        return losses

    def relu_decisions(self):
        L, out = self.last, self.body_relu_decisions()
        nchw = lambda t: (t > 0).permute(0, 3, 1, 2).cpu()
        for name in ("cls", "reg"):
            for l, xs in enumerate(L["acts"][name]):
                for j in range(4):
                    out["%s.%d.%d" % (name, l, j)] = nchw(xs[j + 1])
        out["p6"] = nchw(L["P"][3])
        return out

    def backward(self, gscale=(1.0, 1.0)):
        L = self.last
        N, P, level_hw = L["N"], L["P"], L["level_hw"]
        gcls = torch.zeros_like(L["cls_flat"]); greg = torch.zeros_like(L["reg_flat"])
        ops.focal_loss(L["cls_flat"], L["level_pix"], N, 9, self.K, self.cls_ld, L["matched"], L["gt_labels"], L["gt_off"], L["img_w"], grad=gcls, gscale=gscale[0])
        ops.smooth_l1(L["reg_flat"], L["box_idx"], L["reg_tgt"], 0.0, 1.0, weights=L["box_w"], grad=greg, gscale=gscale[1])
        # heads: weight gradients level by level (shared weights accumulate; they run on the side stream), data gradients of one layer of
        # BOTH towers on all five levels in one grouped launch
        oc = orr = 0
        g_cls, g_reg = [], []
        for l, (h, w) in enumerate(level_hw):
            g_cls.append(gcls[oc:oc + L["cls_sizes"][l]].view(N, h, w, self.cls_ld)); g_reg.append(greg[orr:orr + L["reg_sizes"][l]].view(N, h, w, 36))
            oc += L["cls_sizes"][l]; orr += L["reg_sizes"][l]
        acts = L["acts"]
        for l in range(5):
            self.cls_out.bwd(g_cls[l], need_dx=False, accumulate=l > 0, x=acts["cls"][l][4])
            self.reg_out.bwd(g_reg[l], need_dx=False, accumulate=l > 0, x=acts["reg"][l][4])
            self.cls_out._count(acts["cls"][l][4], 1); self.reg_out._count(acts["reg"][l][4], 1)
        # every ReLU backward of the towers rides in the epilogue of the data gradient that produces its input gradient
        g_cls = ops.conv_group(g_cls, self.cls_out._packed_grad(), pad=1, masks=[acts["cls"][l][4] for l in range(5)])
        g_reg = ops.conv_group(g_reg, self.reg_out._packed_grad(), pad=1)              # 36 channels: not a tiled-kernel shape
        for l in range(5):
            ops.relu_bwd_(g_reg[l], acts["reg"][l][4])
        for j in (3, 2, 1, 0):
            for l in range(5):
                self.cls_tower[j].bwd(g_cls[l], need_dx=False, accumulate=l > 0, x=acts["cls"][l][j])
                self.reg_tower[j].bwd(g_reg[l], need_dx=False, accumulate=l > 0, x=acts["reg"][l][j])
                self.cls_tower[j]._count(acts["cls"][l][j], 1); self.reg_tower[j]._count(acts["reg"][l][j], 1)
            masks = ([acts["cls"][l][j] for l in range(5)] + [acts["reg"][l][j] for l in range(5)]) if j > 0 else None
            gs = ops.conv_group(g_cls + g_reg, [self.cls_tower[j]._packed_grad()] * 5 + [self.reg_tower[j]._packed_grad()] * 5, pad=1, masks=masks)
            g_cls, g_reg = gs[:5], gs[5:]
        gP = [ops.add(g_cls[l], g_reg[l]) for l in range(5)]
        g6 = self.p7.bwd(gP[4], x=L["p6_relu"])
        ops.relu_bwd_(g6, P[3])
        g6 = ops.add(g6, gP[3])
        gP[2] = ops.add(gP[2], self.p6.bwd(g6, x=P[2]))
        ginner = self._fpn_out_bwd(gP[:3])
        for i in range(1, 3):
            ops.upsample_bwd_(ginner[i - 1], ginner[i])
        gC = [None] * 4
        for i in range(3):
            gC[i + 1] = self.lat[i].bwd(ginner[i], need_dx=self.layers[i + 1][0])
        self._body_backward(gC)
        self._join_side()
        return self.grads


def _backward_into_grads(net, gscale, **kw):
    """net.backward(gscale, **kw) under autograd's rules for ``.grad``: a parameter whose .grad is set (no zero_grad since the last
    backward, or zero_grad(set_to_none=False)) accumulates.  The .grad tensors ARE views of the flat gradient buffer, so accumulation
    happens inside the kernels; a .grad that is some other tensor, or set on some parameters only, is refused."""
    mine = [p.grad is not None and p.grad.data_ptr() == net.grads[k].data_ptr() for k, p in net.params.items()]
    foreign = [k for k, p in net.params.items() if p.grad is not None and p.grad.data_ptr() != net.grads[k].data_ptr()]
    if foreign:
        raise RuntimeError("parameter .grad was replaced by another tensor (%s ...): use zero_grad() between steps" % foreign[0])
    if any(mine) and not all(mine):
        raise RuntimeError("some parameters carry a gradient and some do not: call zero_grad() on all of them")
    net.accumulate_grads = all(mine)
    try:
        net.backward(gscale, **kw)
    finally:
        net.accumulate_grads = False
    for k in net.names:
        if net.params[k].grad is None:
            net.params[k].grad = net.grads[k]


class _LossFn(torch.autograd.Function):
    """Bridges the hand-written backward into torch autograd so that the reference's ``losses.backward()`` works unchanged."""

    @staticmethod
    def forward(ctx, anchor, net, images, targets):
        ctx.net = net
        d = net.forward(images, targets)
        # every forward of the model -- with or without grad -- replaces the layers' ONE set of saved activations, so it bumps the serial:
        # a loss evaluation under no_grad between a forward and its backward invalidates that backward too
        net.forward_serial = ctx.serial = getattr(net, "forward_serial", 0) + 1
        return tuple(d[k].reshape(()) for k in net.LOSS_NAMES)

    @staticmethod
    def backward(ctx, *gs):
        net = ctx.net
        if net.forward_serial != ctx.serial:
            # the layers keep ONE set of saved activations (no per-call graph): differentiating an older forward would silently
            # use the newer one's -- refuse instead
            raise RuntimeError("backward() of a training forward after a later forward of the same model: its saved activations "
                               "were replaced; call backward() before the next model(images, targets)")
        gscale = [0.0 if g is None else float(g) for g in gs]
        _backward_into_grads(net, gscale)           # net.last IS this forward's record (the serial check above)
        return None, None, None, None


class _LossFnLL(torch.autograd.Function):
    """_LossFn for a ``loss_mode="ll"`` trainer: four [N] loss vectors and the pooled pyramid vectors [N, 4, 256] leave the forward; the
    backward takes one gradient per loss and image and -- unless the features were detached (ll_train.py:90-95) -- LossNet's gradient
    of the pooled vectors."""

    @staticmethod
    def forward(ctx, anchor, net, images, targets):
        ctx.net = net
        ctx.set_materialize_grads(False)                   # detached features reach backward() as None, not as a tensor of zeros
        d, pooled = net.forward(images, targets)
        net.forward_serial = ctx.serial = getattr(net, "forward_serial", 0) + 1
        return tuple(d[k] for k in net.LOSS_NAMES) + (pooled,)

    @staticmethod
    def backward(ctx, *gs):
        net = ctx.net
        if net.forward_serial != ctx.serial:
            raise RuntimeError("backward() of a training forward after a later forward of the same model: its saved activations "
                               "were replaced; call backward() before the next model(images, targets)")
        N = net.last["N"]
        zero = None
        rows = []
        for g in gs[:4]:
            if g is None:
                zero = torch.zeros(N, dtype=torch.float32, device=net.dev) if zero is None else zero
                g = zero
            rows.append(g.reshape(N).to(torch.float32))
        _backward_into_grads(net, torch.stack(rows), g_pooled=gs[4])
        return None, None, None, None


class TrainableDetector(object):
    """``task_model`` in train mode: ``model(images, targets) -> {loss name: scalar tensor}`` whose sum can be ``.backward()``-ed.
    Over a ``loss_mode="ll"`` trainer: ``-> (features, {loss name: [N] tensor})`` as detection/frcnn_ll.py returns them, ``features``
    = {'0'..'3'}: [N, 256] views of the pooled pyramid vectors (one autograd tensor), ready for ll_train.LossNet."""

    def __init__(self, net):
        self.net = net
        self._anchor = torch.zeros(1, device=net.dev, requires_grad=True)
        self.training = True

    def parameters(self):
        return self.net.parameters()

    def __call__(self, images, targets):
        if getattr(self.net, "loss_mode", None) == "ll":
            out = _LossFnLL.apply(self._anchor, self.net, images, targets)
            pooled = out[4]
            return {str(k): pooled[:, k, :] for k in range(4)}, dict(zip(self.net.LOSS_NAMES, out[:4]))
        out = _LossFn.apply(self._anchor, self.net, images, targets)
        return dict(zip(self.net.LOSS_NAMES, out))

    def train(self, mode=True):
        self.training = bool(mode)
        return self


class SGD(torch.optim.Optimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay) (cald_train.py:397) with the update done by HIP kernels: ONE launch over the
    trainer's flat parameter / gradient buffers when the optimizer holds exactly the trainer's parameters in one group (the reference's
    setup), one launch per tensor otherwise.  ``param_groups[i]['lr']`` is read every step, so torch's lr schedulers (warmup LambdaLR,
    MultiStepLR) drive it unchanged; ``state[p]['momentum_buffer']`` are views of one flat momentum buffer in the fused case."""

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, net=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self.net = net
        self._mflat = None

    def _fused_ok(self):
        net = self.net
        if net is None or len(self.param_groups) != 1:
            return False
        ps = self.param_groups[0]["params"]
        if len(ps) != len(net.names):
            return False
        for p, k in zip(ps, net.names):
            if p is not net.params[k] or p.grad is None or p.grad.data_ptr() != net.grads[k].data_ptr():
                return False
        started = ["momentum_buffer" in self.state[p] for p in ps]
        if any(started) and not all(started):
            return False                                   # a partial first step: per-tensor path
        if all(started) and ps:
            self._adopt_momentum(ps)
        return True

    @torch.no_grad()
    def _adopt_momentum(self, ps):
        """Every parameter has a momentum buffer.  After ``load_state_dict()`` (resume, cald_train.py:356-360) those are fresh
        tensors, not views of the flat buffer the fused launch updates: copy them in and re-point ``state`` at the views, so the
        loaded momentum is what the next step uses (and what ``state_dict()`` saves afterwards)."""
        net = self.net
        views_ok = self._mflat is not None
        if views_ok:
            base = self._mflat.data_ptr()
            for p, k in zip(ps, net.names):
                if self.state[p]["momentum_buffer"].data_ptr() != base + 4 * net._off[k]:
                    views_ok = False
                    break
        if views_ok:
            return
        flat = torch.zeros_like(net.flat)
        for p, k in zip(ps, net.names):
            view = flat[net._off[k]:net._off[k] + p.numel()].view(p.shape)
            view.copy_(self.state[p]["momentum_buffer"].to(view.device, torch.float32))
            self.state[p]["momentum_buffer"] = view
        self._mflat = flat

    @torch.no_grad()
    def step(self, closure=None):
        if self._fused_ok():
            grp, net = self.param_groups[0], self.net
            first = self._mflat is None
            if first and grp["momentum"] != 0:
                self._mflat = torch.zeros_like(net.flat)
                for k in net.names:
                    p = net.params[k]
                    self.state[p]["momentum_buffer"] = self._mflat[net._off[k]:net._off[k] + p.numel()].view(p.shape)
            # the pad words between tensors hold 0 in all three buffers and stay 0 under the update
            ops.sgd_(net.flat, net.gflat, self._mflat, grp["lr"], grp["momentum"], grp["weight_decay"], first)
            net.parameters_changed()
            return
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                first = "momentum_buffer" not in st
                if first and grp["momentum"] != 0:
                    st["momentum_buffer"] = torch.zeros_like(p)
                ops.sgd_(p.data, p.grad, st.get("momentum_buffer"), grp["lr"], grp["momentum"], grp["weight_decay"], first)
        if self.net is not None:
            self.net.parameters_changed()


TrainableFasterRCNN = TrainableDetector
