"""What the two trainable detectors share (cald_amd/train.py states the semantics): the layer objects over the ``cald_train_*``
operators, parameter storage in one flat buffer, the ResNet body forward + backward, the FPN top-down pass, input preparation,
the samplers, and the host arithmetic that places an anchor's logits in a flat head buffer."""
import contextlib
import os
import time

import numpy as np
import torch

from . import train_ops as ops


def _bn_fold(sd, prefix, eps=1e-5):
    """FrozenBatchNorm2d as y = x * scale + shift (torchvision.ops.misc.FrozenBatchNorm2d, eps 1e-5 in 0.8.x)."""
    w, b = sd[prefix + ".weight"].double(), sd[prefix + ".bias"].double()
    rm, rv = sd[prefix + ".running_mean"].double(), sd[prefix + ".running_var"].double()
    scale = w * (rv + eps).rsqrt()
    return scale.float(), (b - rm * scale).float()


def _bn_fold_f32(sd, prefix, eps=1e-5):
    """The same fold in float32, operation by operation what an inference model's finalize computes (scale = w * (1 / sqrt(var + eps)),
    shift = b - mean * scale): a forward_precision "f16x3" trainer reproduces HipDetector(precision="f16x3") bit for bit."""
    w, b, rm, rv = [sd[prefix + s].float().numpy() for s in (".weight", ".bias", ".running_mean", ".running_var")]
    scale = w * (np.float32(1.0) / np.sqrt(rv + np.float32(eps)))
    return torch.from_numpy(scale), torch.from_numpy(b - rm * scale)


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


def stride2_hw(hw):
    """Output size of a stride-2 level over a level of size hw (kernel 1 without padding, or kernel 3 with padding 1)."""
    return ((hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1)


def anchor_slots(img, idx, level_pix, per_pix, ld, N):
    """Where the anchors `idx` (numbered level, y, x, anchor-in-pixel over one image's pyramid) of image `img` sit in a flat head buffer
    whose level block l is [N][level_pix[l]][ld] floats: (float offset of the pixel's row, anchor-in-pixel number a) per anchor.
    A head with c channels per anchor reads its first one at offset + c * a (+ the channel group's start within the row)."""
    level_pix = np.asarray(level_pix)
    lvl_start = np.cumsum([0] + [n * per_pix for n in level_pix])
    lvl_off = np.cumsum([0] + [N * n * ld for n in level_pix])
    l = np.searchsorted(lvl_start, idx, side="right") - 1
    rel = idx - lvl_start[l]
    pix, a = rel // per_pix, rel % per_pix
    return lvl_off[l] + (img * level_pix[l] + pix) * ld, a


def level_views(flat, sizes, level_hw, N, ld):
    """The per-level [N, h, w, ld] views of a flat buffer made of one block of sizes[l] floats per level."""
    views, o = [], 0
    for n, (h, w) in zip(sizes, level_hw):
        views.append(flat[o:o + n].view(N, h, w, ld)); o += n
    return views


def _nchw_mask(t):
    """Which side the ReLU behind the NHWC activation t took, as a bool NCHW CPU tensor."""
    return (t > 0).permute(0, 3, 1, 2).cpu()


@contextlib.contextmanager
def _issue_on(pair, enter_stream=True):
    """What the block issues through train_ops goes to the context of pair = (stream, context) and, with `enter_stream`, torch's
    own work to the stream as well; pair None: nothing changes.  Without `enter_stream` only the operators that take their stream
    from the context (weight gradients, packing, matching) move, and torch keeps allocating on the current stream."""
    prev = ops._WGRAD_CTX[0]
    if pair is not None:
        ops._WGRAD_CTX[0] = pair[1]
    try:
        with torch.cuda.stream(pair[0]) if pair is not None and enter_stream else contextlib.nullcontext():
            yield
    finally:
        ops._WGRAD_CTX[0] = prev


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
        self.w16_S = None               # forward_precision "f16x3": the weight scale of the forward pack's split twin (refresh_f16x3_scales)
        self.grad16_S = None            # backward_precision "f16x3": the weight scale S_d of the data-gradient pack's split twin (likewise)
        self.name = wnames[0]
        self.idx = len(net.convs)       # names this layer's data-gradient launches in the trainer's table of gradient exponents
        self.x = None
        self.out16 = None               # the split twin of the last forward's output, where fwd(split_out=True) wrote one
        net.convs.append(self)

    def _packed(self):
        if self._pk is None or (self.trainable and self._pk_version != self.net.version):
            buf, buf16 = (self._pk.buf, self._pk.w16) if self._pk is not None else (None, None)
            self._pk = ops.PackedConv(self.w, self.b, self.scale, self.shift, CinK=self.cin_k, mode=self.mode, taps=self.taps, out=buf,
                                      w16_S=self.w16_S, w16_out=buf16)
            self._pk_version = self.net.version
            self._pkd_version = -1
        return self._pk

    def _plan_packs(self):
        """The forward and data-gradient PackedConv of a trainable layer for a PackPlan (allocated, not packed, on first use)."""
        if self._pk is None:
            self._pk = ops.PackedConv(self.w, self.b, self.scale, self.shift, CinK=self.cin_k, mode=self.mode, taps=self.taps, pack=False,
                                      w16_S=self.w16_S)
        if self._pkd is None:
            self._pkd = ops.PackedConv(self.w, scale=self.scale, CinK=self.out_ld, mode=3 if self.mode == 2 else 1, taps=self.taps, pack=False,
                                       grad16_S=self.grad16_S)
        return [self._pk, self._pkd]

    def _packed_grad(self):
        if self._pkd is None or self._pkd_version != self.net.version:
            buf, buf16 = (self._pkd.buf, self._pkd.w16) if self._pkd is not None else (None, None)
            # FrozenBatchNorm layers: the scale rides in the packed filter, so the incoming gradient is the one wrt the BN output
            self._pkd = ops.PackedConv(self.w, scale=self.scale, CinK=self.out_ld, mode=3 if self.mode == 2 else 1, taps=self.taps, out=buf,
                                       grad16_S=self.grad16_S, w16_out=buf16)
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

    def fwd(self, x, relu=False, residual=None, up=None, out=None, x16=None, ex16=None, split_out=False):
        """forward_precision "f16x3" only (ignored otherwise): x16 / ex16 = the split twins of x and of residual / up (train_ops.conv);
        split_out: the output is later ADDED in another layer's epilogue (a residual, the FPN's top-down term), where the inference mode
        adds its split form -- the twin is written beside the fp32 tensor and kept in self.out16."""
        if self.trainable:
            self.x = x
        self._count(x, 1)
        pk = self._packed()
        if pk.w16 is None:
            self.out16 = None
            return ops.conv(x, pk, stride=self.stride, pad=self.pad, relu=relu, residual=residual, up=up, out=out, out_ld=self.out_ld)
        res = ops.conv(x, pk, stride=self.stride, pad=self.pad, relu=relu, residual=residual, up=up, out=out, out_ld=self.out_ld,
                       x16=x16, ex16=ex16, split_out=split_out)
        res, self.out16 = res if split_out else (res, None)
        return res

    def bwd(self, g, need_dx=True, residual=None, accumulate=False, x=None, mask=None):
        """g: gradient wrt this layer's output AFTER its FrozenBatchNorm (if any) and after the ReLU mask, row stride out_ld: the BN
        scale is folded into the packed data-gradient filter and into the weight-gradient reduction.  mask: the saved post-ReLU
        activation the returned data gradient flows into (its ReLU backward is applied in the conv epilogue)."""
        x = self.x if x is None else x
        accumulate = accumulate or self.net.accumulate_grads
        self._count(x, int(bool(need_dx)) + 1)
        side = self.net.side
        if side is not None:            # the weight gradient depends on (x, g) only: issue it beside the data gradient
            side[0].wait_stream(torch.cuda.current_stream(self.net.dev))
            x.record_stream(side[0]); g.record_stream(side[0])
        with _issue_on(side, enter_stream=False):          # the weight-gradient operators take their stream from the context
            if self.mode == 2 or self.w.dim() == 2:
                ops.linear_wgrad(x.view(g.shape[2], -1), g.view(g.shape[2], -1), self.Cout, self.gw, self.gb, taps=self.taps or 1, accumulate=accumulate)
            else:
                ops.conv_wgrad(x, g, self.Cin, self.Cout, self.K, self.K, self.stride, self.pad, self.gw, self.gb, accumulate=accumulate,
                               row_scale=self.scale)
        if not need_dx:
            return None
        pkd = self._packed_grad()
        G = self.net._dgrad_G((self.idx, 0), g)
        if self.mode == 2 or self.w.dim() == 2:
            return ops.conv(g, pkd, residual=residual, mask=mask, G=G)
        return ops.conv_dgrad(g, pkd, x.shape[1], x.shape[2], self.stride, self.pad, residual=residual, mask=mask, G=G)


class _Bottleneck(object):
    def __init__(self, net, prefix, stride, has_down, need_dx):
        self.c1 = _Conv(net, [prefix + ".conv1.weight"], bn=prefix + ".bn1")
        self.c2 = _Conv(net, [prefix + ".conv2.weight"], bn=prefix + ".bn2", stride=stride, pad=1)
        self.c3 = _Conv(net, [prefix + ".conv3.weight"], bn=prefix + ".bn3")
        self.down = _Conv(net, [prefix + ".downsample.0.weight"], bn=prefix + ".downsample.1", stride=stride) if has_down else None
        self.trainable, self.need_dx = self.c1.trainable, need_dx

    def fwd(self, x, x16=None):
        """x16: the split twin of x (forward_precision "f16x3": the previous block's out16), or None.  Sets self.out16 likewise."""
        self.a1 = self.c1.fwd(x, relu=True, x16=x16)
        self.a2 = self.c2.fwd(self.a1, relu=True)
        idt, idt16 = (self.down.fwd(x, x16=x16, split_out=True), self.down.out16) if self.down is not None else (x, x16)
        self.out = self.c3.fwd(self.a2, relu=True, residual=idt, ex16=idt16, split_out=True)
        self.out16 = self.c3.out16
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
    """What the two detectors share: parameter storage, the ResNet body (forward + backward), the FPN top-down pass, input preparation."""
    LOSS_NAMES = ()
    MERGE_GROUPS = ()
    LAT_BODY = ()               # LAT_BODY[i]: the body layer (index into self.layers / feats) that feeds FPN lateral i
    _PACK_PLAN = os.environ.get("CALD_TRAIN_PACK_PLAN", "1") != "0"      # all trainable layers re-packed in two launches per step

    def _init_common(self, state_dict, num_classes, depth, min_size, max_size, device, trainable_layers, generator, sampler="choose_k",
                     forward_precision="fp32", backward_precision="fp32"):
        if sampler not in ("choose_k", "randperm"):
            raise ValueError("sampler must be 'choose_k' or 'randperm', got %r" % (sampler,))
        if forward_precision not in ("fp32", "f16x3"):
            raise ValueError("forward_precision must be 'fp32' or 'f16x3', got %r" % (forward_precision,))
        # "f16x3": every forward conv / linear layer of a shape the split-fp16 kernels take (conv_h3 / conv_h4: three fp16 MFMAs per
        # product, fp32-grade results) runs there, bit for bit what a HipDetector(precision="f16x3") computes; the backward, the weight
        # gradients and SGD stay the exact fp32 ones, on the activations that forward saved.  "fp32" launches exactly what it always did.
        self.forward_precision = forward_precision
        if backward_precision not in ("fp32", "f16x3"):
            raise ValueError("backward_precision must be 'fp32' or 'f16x3', got %r" % (backward_precision,))
        # "f16x3": every data gradient of a shape conv_h3 takes runs there, on the split twin of the data-gradient pack, the gradient staged
        # at its own power of two 2^(4 + G) (per layer and pyramid level; _dgrad_G); the weight gradients, the RoIAlign backward, the losses
        # and SGD stay exact fp32.  Independent of forward_precision; "fp32" launches exactly what it always did.
        self.backward_precision = backward_precision
        self._grad_G = {}               # (layer, level) -> gradient exponent G, fixed between refreshes
        self._grad_max = {}             # (layer, level) -> the max |g| the last calibration step saw
        self._calib = None              # a list while the next / current backward is a calibration step: ((layer, level), max |g| on the device)
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
                sc, sh = (_bn_fold_f32 if forward_precision == "f16x3" else _bn_fold)(sd, p)
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

    def refresh_f16x3_scales(self):
        """forward_precision "f16x3": derives every layer's weight scale 2^S from its CURRENT weights (S = 14 - exponent of max |w|, the
        inference mode's policy) -- at construction, at every TrainableDetector.train() switch, and whenever the caller asks.  One host
        synchronisation; between refreshes S is fixed, so a step neither stops the host nor depends on anything but its inputs.  A weight
        that outgrows fp16's range under a stale S (x 4 from the last refresh at the least) packs as inf and the step's losses turn
        non-finite; one that shrinks keeps fewer bits in its lo half.  Returns the number of layers whose S changed."""
        changed = 0
        convs = [cv for cv in self.convs if cv.mode in (0, 2)]
        if self.forward_precision == "f16x3":
            mx = torch.stack([cv.w.abs().max() for cv in convs]).cpu().tolist()
            for cv, m in zip(convs, mx):
                S = ops.f16x3_scale(m)[0]
                if S != cv.w16_S:
                    cv.w16_S, cv._pk, cv._pk_version = S, None, -1     # a new pack; a frozen layer's is made on its next use
                    changed += 1
        if self.backward_precision == "f16x3":
            # S_d of the data-gradient packs: the same policy on max |w * bn_scale|, what those packs hold.  The gradient exponents are
            # re-derived too: the next backward is a calibration step -- its data gradients run on the exact kernels while the largest
            # |g| of every data gradient's input is collected on the device, read once at its end (_end_backward)
            rows = lambda cv: cv.w if cv.scale is None else cv.w * cv.scale.view((-1,) + (1,) * (cv.w.dim() - 1))
            mx = torch.stack([rows(cv).abs().max() for cv in convs]).cpu().tolist()
            for cv, m in zip(convs, mx):
                S = ops.f16x3_scale(m)[0]
                if S != cv.grad16_S:
                    cv.grad16_S, cv._pkd, cv._pkd_version = S, None, -1
                    changed += 1
            self._grad_G, self._calib = {}, []
        if changed:
            self._pack_plan = None
        return changed

    def _dgrad_G(self, key, g):
        """The gradient exponent of the data-gradient launch `key` = (layer, level) reading g; None = the exact kernels: in the default
        mode, on a calibration step (which records max |g|) and for a launch no calibration step has seen."""
        if self.backward_precision != "f16x3":
            return None
        if self._calib is not None:
            self._calib.append((key, g.abs().max()))
            return None
        return self._grad_G.get(key)

    def _dgrad_Gs(self, keys, gs):
        """_dgrad_G of every problem of a grouped launch; None (the exact kernels) unless every problem has one."""
        Gs = [self._dgrad_G(k, g) for k, g in zip(keys, gs)]
        return None if any(G is None for G in Gs) else Gs

    def _end_backward(self):
        """Closes a calibration step: one read of the collected maxima (the refresh's one synchronisation), G per launch by the policy of
        cald_train_f16x3_grad_scale; a launch that ran several times in the step takes the largest."""
        if self._calib is not None and not self._calib:
            self._calib = None                              # (a backward without a data gradient)
        if self._calib:
            torch.cuda.synchronize(self.dev)                # the maxima were collected on all three streams
            mx = torch.stack([m for _, m in self._calib]).cpu().tolist()
            top = {}
            for (key, _), m in zip(self._calib, mx):
                top[key] = m if key not in top or not (m <= top[key]) else top[key]
            self._grad_G = {k: ops.f16x3_grad_scale(m)[0] for k, m in top.items()}
            self._grad_max = top                            # what the calibration step saw (tools/train_grad_ranges.py)
            self._calib = None

    def _join_side(self):
        if self.side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self.side[0])

    def _aux_stream(self):
        """What the block issues goes to the batch-only stream and its context (to the current stream where there is none)."""
        return _issue_on(self.aux)

    def _hand_to_main(self, tensors):
        """The main stream waits for the batch-only stream and takes over the tensors produced there."""
        if self.aux is not None:
            self._main.wait_stream(self.aux[0])
            for t in tensors:
                t.record_stream(self._main)

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

    def _fpn_top_down_fwd(self, feats):
        """The FPN's lateral 1x1 convs from the top level down, each adding the upsampled level above it in its epilogue."""
        top = len(self.lat) - 1
        inner = [None] * (top + 1)
        f16 = self.split_twins["feats"]
        inner[top] = self.lat[top].fwd(feats[self.LAT_BODY[top]], x16=f16[self.LAT_BODY[top]], split_out=True)
        for i in range(top - 1, -1, -1):
            inner[i] = self.lat[i].fwd(feats[self.LAT_BODY[i]], up=inner[i + 1], x16=f16[self.LAT_BODY[i]], ex16=self.lat[i + 1].out16, split_out=True)
        self.split_twins["inner"] = [cv.out16 for cv in self.lat]
        return inner

    def _fpn_top_down_bwd(self, ginner):
        """Backward of _fpn_top_down_fwd.  Returns gC for _body_backward: the laterals' data gradients by body layer (None where a layer
        feeds no lateral or is frozen)."""
        for i in range(1, len(self.lat)):
            ops.upsample_bwd_(ginner[i - 1], ginner[i])
        gC = [None] * 4
        for i, li in enumerate(self.LAT_BODY):
            gC[li] = self.lat[i].bwd(ginner[i], need_dx=self.layers[li][0])     # the body layer producing feats[li] is trainable
        return gC

    def _fpn_out_fwd(self, inner):
        """The FPN output 3x3 convs (one weight per level) of all levels in one grouped launch."""
        for cv, x in zip(self.fout, inner):
            cv.x = x; cv._count(x, 1)
        i16 = self.split_twins["inner"]
        return ops.conv_group(inner, [cv._packed() for cv in self.fout], pad=1, xs16=i16 if all(t is not None for t in i16) else None)

    def _fpn_out_bwd(self, gP):
        """Weight gradients per level (side stream), data gradients of all levels in one grouped launch."""
        for cv, g in zip(self.fout, gP):
            cv.bwd(g, need_dx=False); cv._count(cv.x, 1)
        return ops.conv_group(gP, [cv._packed_grad() for cv in self.fout], pad=1, Gs=self._dgrad_Gs([(cv.idx, 0) for cv in self.fout], gP))

    def _mark(self, name):
        if self.timing is not None:
            torch.cuda.synchronize(self.dev); self.timing.append((name, time.time()))

    def _repack(self):
        """Forward and data-gradient forms of every trainable weight, packed on the side stream while the main stream runs the
        frozen stem / layer 1 (the packs depend on the parameters only)."""
        if self.side is None:
            return
        st = self.side[0]
        st.wait_stream(self._main)                          # the optimizer's update of the flat parameter buffer
        with _issue_on(self.side):
            planned = [cv for cv in self.convs if cv.trainable] if self._PACK_PLAN else []
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
        feats, x16 = [], None
        self.split_twins = {"feats": [], "inner": []}       # forward_precision "f16x3": the split twins of feats / the laterals (None entries in "fp32")
        waited = self.side is None
        for li, (trainable, blocks) in enumerate(self.layers):
            if trainable and not waited:                    # first layer that reads a freshly packed weight
                self._main.wait_event(self._packs_ready)
                waited = True
            for blk in blocks:
                x = blk.fwd(x, x16)
                x16 = blk.out16
            feats.append(x); self.split_twins["feats"].append(x16)
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
        for li, (trainable, blocks) in enumerate(self.layers):
            for b, blk in enumerate(blocks):
                if trainable:
                    out.update({"layer%d.%d.a1" % (li + 1, b): _nchw_mask(blk.a1), "layer%d.%d.a2" % (li + 1, b): _nchw_mask(blk.a2),
                                "layer%d.%d.out" % (li + 1, b): _nchw_mask(blk.out)})
        return out
