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

The code by concern: ``train_core`` (layers, parameter storage, the body, what both detectors share), ``train_frcnn`` and
``train_retina`` (one detector's step each, as named stages over a step record), ``train_retina_ll`` (the RetinaNet with per-image
losses that trains LossNet beside it), and here the autograd bridge and the optimizer.
"""
import torch

from . import train_ops as ops
from .train_core import choose_k                    # noqa: F401  (every public name still resolves here)
from .train_frcnn import FasterRCNNTrainer          # noqa: F401
from .train_retina import RetinaNetTrainer          # noqa: F401
from .train_retina_ll import RetinaNetLLTrainer     # noqa: F401


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
    """_LossFn for a ``loss_mode="ll"`` trainer: one [N] loss vector per name in LOSS_NAMES and the pooled pyramid vectors [N, 4, 256]
    leave the forward -- between them, for RetinaNetLLTrainer, each loss's mean over the batch (retina_ll.py:132, :220); the backward
    takes one gradient per loss and image (a mean's upstream gradient is folded in as g_mean / N on the device) and -- unless the
    features were detached (ll_train.py:90-95, :107-113) -- LossNet's gradient of the pooled vectors."""

    @staticmethod
    def forward(ctx, anchor, net, images, targets):
        ctx.net = net
        ctx.set_materialize_grads(False)                   # detached features reach backward() as None, not as a tensor of zeros
        d, pooled = net.forward(images, targets)
        net.forward_serial = ctx.serial = getattr(net, "forward_serial", 0) + 1
        means = tuple(net.last["means"][k].reshape(()) for k in net.LOSS_NAMES) if getattr(net, "LL_MEANS", False) else ()
        return tuple(d[k] for k in net.LOSS_NAMES) + means + (pooled,)

    @staticmethod
    def backward(ctx, *gs):
        net = ctx.net
        if net.forward_serial != ctx.serial:
            raise RuntimeError("backward() of a training forward after a later forward of the same model: its saved activations "
                               "were replaced; call backward() before the next model(images, targets)")
        N, n = net.last["N"], len(net.LOSS_NAMES)
        zero = None
        rows = []
        for i, g in enumerate(gs[:n]):
            if g is None:
                zero = torch.zeros(N, dtype=torch.float32, device=net.dev) if zero is None else zero
                g = zero
            g = g.reshape(N).to(torch.float32)
            g_mean = gs[n + i] if len(gs) > n + 1 else None
            if g_mean is not None:                         # mean = sum_n loss_n / N: its upstream gradient reaches every image as g_mean / N
                g = g + g_mean.to(torch.float32) / N
            rows.append(g)
        _backward_into_grads(net, torch.stack(rows), g_pooled=gs[-1])
        return None, None, None, None


class TrainableDetector(object):
    """``task_model`` in train mode: ``model(images, targets) -> {loss name: scalar tensor}`` whose sum can be ``.backward()``-ed.
    Over a ``loss_mode="ll"`` trainer: ``-> (features, {loss name: [N] tensor})`` as detection/frcnn_ll.py returns them, ``features``
    = {'0'..'3'}: [N, 256] views of the pooled pyramid vectors (one autograd tensor), ready for ll_train.LossNet.  Over a
    RetinaNetLLTrainer: ``-> (features, {loss name: (mean, [N scalars])})`` as detection/retina_ll.py returns them, ``features`` a LIST of the
    four views, indexed by int as ll_train.py:110-119 does."""

    def __init__(self, net):
        self.net = net
        self._anchor = torch.zeros(1, device=net.dev, requires_grad=True)
        self.training = True

    def parameters(self):
        return self.net.parameters()

    def __call__(self, images, targets):
        if getattr(self.net, "loss_mode", None) == "ll":
            out = _LossFnLL.apply(self._anchor, self.net, images, targets)
            names, pooled = self.net.LOSS_NAMES, out[-1]
            n = len(names)
            if getattr(self.net, "LL_MEANS", False):        # retina_ll.py:554: features as a list, every loss as (mean, [per image])
                return [pooled[:, k, :] for k in range(4)], {k: (out[n + i], list(out[i].unbind(0))) for i, k in enumerate(names)}
            return {str(k): pooled[:, k, :] for k in range(4)}, dict(zip(names, out[:n]))
        out = _LossFn.apply(self._anchor, self.net, images, targets)
        return dict(zip(self.net.LOSS_NAMES, out))

    def train(self, mode=True):
        """As nn.Module.train().  Over a forward_precision "f16x3" trainer a switch to train mode also re-derives the layers' weight
        scales (refresh_f16x3_scales): the reference's loops switch once per epoch, where the host has synchronised anyway.  Over a
        backward_precision "f16x3" trainer it makes the next backward a calibration step (exact data gradients, new gradient exponents)."""
        self.training = bool(mode)
        if self.training:
            self.net.refresh_f16x3_scales()
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
