"""Training the loss-prediction module (LL4AL's LossNet) beside the detector: ll_train.py:55-142 on the MI355X.

    features, task_loss_dict = task_model(images, targets)       # train.TrainableDetector over FasterRCNNTrainer(loss_mode="ll") or RetinaNetLLTrainer
    ll_pred = ll_model(features)                                   # LossNet below: cald_lossnet_train_fwd
    ll_loss = ll_weight * LossPredLoss(ll_pred, sum of the per-image task losses, margin)      # cald_loss_pred_loss
    (task_losses + ll_loss).backward()                             # cald_lossnet_train_bwd, then the detector's hand-written backward

``LossNet`` keeps its ten tensors in one flat device buffer (like the detector trainer), so ``train.SGD(ll_model.parameters(), ...,
net=ll_model)`` updates them in one launch; its ``state_dict()`` has the reference's keys and goes as it is into
``baselines.ll_get_uncertainty``, whose sweep computes the same prediction chains (lossnet.hip) -- a LossNet trained here is scored by the
sweep on the arithmetic it was trained with.  ``features`` are the POOLED vectors ({'0'..'3'}: [N, 256]): the detector pools its NHWC
pyramid itself (cald_train_gap) because the maps never exist in torch's layout; the reference's ``features['k'].detach()`` lines work on
them unchanged.  torch supplies memory, the autograd / Optimizer interfaces and the initial weights; the arithmetic is libcaldhip's.
No fallback: without the library or an MI355X every compute call raises.
"""
import math
import sys

import torch

from .baselines import LOSSNET_KEYS

CHANNELS = 256


def _ops():
    from . import train_ops
    return train_ops


class _LossNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, anchor, net):
        pred, hidden = _ops().lossnet_fwd(net._plist, pooled, net.D)
        ctx.net, ctx.pooled, ctx.hidden = net, pooled, hidden
        return pred.view(-1, 1)

    @staticmethod
    def backward(ctx, g):
        net = ctx.net
        # autograd semantics as in train._LossFn: a parameter whose .grad is set accumulates; the .grad tensors ARE views of the flat buffer
        mine = [p.grad is not None and p.grad.data_ptr() == net.grads[k].data_ptr() for k, p in net.params.items()]
        foreign = [k for k, p in net.params.items() if p.grad is not None and p.grad.data_ptr() != net.grads[k].data_ptr()]
        if foreign:
            raise RuntimeError("parameter .grad was replaced by another tensor (%s ...): use zero_grad() between steps" % foreign[0])
        if any(mine) and not all(mine):
            raise RuntimeError("some parameters carry a gradient and some do not: call zero_grad() on all of them")
        g_pooled = _ops().lossnet_bwd(net._plist, net._glist, ctx.pooled, ctx.hidden, g.reshape(-1).contiguous(), accumulate=all(mine),
                                      need_g_pooled=ctx.needs_input_grad[0])
        for k in net.names:
            if net.params[k].grad is None:
                net.params[k].grad = net.grads[k]
        return g_pooled, None, None


class LossNet(object):
    """ll4al/models/lossnet.py:31-65 with ``feature_sizes`` already pooled away: four Linear(256, interm_dim) + ReLU, concatenation,
    Linear(4 * interm_dim, 1).  ``state_dict``: the reference module's (or any dict with its ten keys); None draws nn.Linear's default
    initialisation from torch's CPU generator."""

    def __init__(self, interm_dim=128, state_dict=None, device="cuda"):
        if state_dict is not None:
            state_dict = state_dict.state_dict() if hasattr(state_dict, "state_dict") else state_dict
            missing = [k for k in LOSSNET_KEYS if k not in state_dict]
            if missing:
                raise KeyError("LossNet state_dict lacks %s" % missing[0])
            interm_dim = int(state_dict["FC1.weight"].shape[0])
        if not 1 <= int(interm_dim) <= 256:
            raise ValueError("interm_dim must be in 1..256, got %r" % (interm_dim,))
        self.D = D = int(interm_dim)
        self.dev = torch.device(device)
        self.names = list(LOSSNET_KEYS)
        shapes = {}
        for j in range(1, 5):
            shapes["FC%d.weight" % j], shapes["FC%d.bias" % j] = (D, CHANNELS), (D,)
        shapes["linear.weight"], shapes["linear.bias"] = (1, 4 * D), (1,)
        offs, o = {}, 0
        for k in self.names:                               # every tensor 16-byte aligned; the pad words stay 0 under SGD
            offs[k] = o
            n = shapes[k][0] * (shapes[k][1] if len(shapes[k]) > 1 else 1)
            o += n + (-n) % 4
        self._off = offs
        self.flat = torch.zeros(o, dtype=torch.float32, device=self.dev)
        self.gflat = torch.zeros(o, dtype=torch.float32, device=self.dev)
        self.params, self.grads = {}, {}
        for k in self.names:
            n = 1
            for s in shapes[k]:
                n *= s
            v = self.flat[offs[k]:offs[k] + n].view(shapes[k])
            if state_dict is not None:
                src = state_dict[k]
                src = src.detach() if hasattr(src, "detach") else torch.as_tensor(src)
                if tuple(src.shape) != shapes[k]:
                    raise ValueError("%s is %s, expected %s" % (k, tuple(src.shape), shapes[k]))
                v.copy_(src.to(torch.float32))
            else:                                          # nn.Linear.reset_parameters
                fan_in = shapes[k.split(".")[0] + ".weight"][1]
                v.copy_((torch.rand(shapes[k]) * 2 - 1) / math.sqrt(fan_in))
            self.params[k] = torch.nn.Parameter(v, requires_grad=True)
            self.grads[k] = self.gflat[offs[k]:offs[k] + n].view(shapes[k])
        self._plist = [self.params[k].data for k in self.names]
        self._glist = [self.grads[k] for k in self.names]
        self._anchor = torch.zeros(1, device=self.dev, requires_grad=True)
        self.training = True

    # ---- the module surface the reference's loop and train.SGD use ----
    def parameters(self):
        return [self.params[k] for k in self.names]

    def named_parameters(self):
        return [(k, self.params[k]) for k in self.names]

    def state_dict(self):
        return {k: self.params[k].detach().clone() for k in self.names}

    def parameters_changed(self):
        pass                                               # nothing is packed: the kernels read the flat buffer

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        if torch.device(device).type != self.dev.type:
            raise NotImplementedError("LossNet lives on the device it was built on (%s)" % self.dev)
        return self

    def __call__(self, features):
        vecs = []
        for k in ("0", "1", "2", "3"):
            f = features[k]
            if f.dim() == 4 and f.shape[2] == 1 and f.shape[3] == 1:
                f = f.reshape(f.shape[0], f.shape[1])
            if f.dim() != 2 or f.shape[1] != CHANNELS:
                raise ValueError("features[%r] is %s: LossNet takes the pooled vectors [N, %d] the detector returns in ll mode "
                                 "(train_ops.train_gap pools NHWC maps)" % (k, tuple(f.shape), CHANNELS))
            vecs.append(f)
        pooled = torch.stack(vecs, dim=1).to(torch.float32).contiguous()            # [B, 4, 256]: plumbing, 4 KB per image
        if not pooled.is_cuda:
            raise RuntimeError("LossNet runs on the MI355X only (features on %s); there is no CPU fallback" % pooled.device)
        return _LossNetFn.apply(pooled, self._anchor, self)


class _LossPredFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, target, margin, per_pair):
        loss, terms, _ = _ops().loss_pred_loss(inp, target, margin, want_terms=per_pair, want_grad=False)
        ctx.inp, ctx.target, ctx.margin, ctx.per_pair = inp, target, margin, per_pair
        return terms if per_pair else loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        _, _, grad = _ops().loss_pred_loss(ctx.inp, ctx.target, ctx.margin, g_up=g.reshape(-1).to(torch.float32).contiguous(),
                                           per_pair=ctx.per_pair)
        return grad.view(ctx.inp.shape), None, None, None


def LossPredLoss(input, target, margin=1.0, reduction='mean'):
    """ll4al/main.py:64-83: the pairwise hinge on (i, B - 1 - i); ``target`` is detached; value and gradient come from one kernel."""
    if len(input) % 2 != 0:
        raise ValueError("the batch size is not even.")
    if input.shape != target.shape or input.dim() != 1:
        raise ValueError("LossPredLoss takes two vectors of one length, got %s and %s" % (tuple(input.shape), tuple(target.shape)))
    if reduction not in ('mean', 'none'):
        raise NotImplementedError("reduction %r" % (reduction,))
    if not input.is_cuda:
        raise RuntimeError("LossPredLoss runs on the MI355X only (input on %s); there is no CPU fallback" % input.device)
    return _LossPredFn.apply(input.to(torch.float32).contiguous(), target.detach().to(torch.float32).contiguous(), float(margin),
                             reduction == 'none')


def train_one_epoch(task_model, task_optimizer, ll_model, ll_optimizer, data_loader, device, cycle, epoch, print_freq,
                    task_epochs=0, ll_weight=1.0, margin=1.0):
    """ll_train.py:55-142 with the reference's positional signature; ``task_epochs`` / ``ll_weight`` stand for ``args.task_epochs`` /
    ``args.ll_weight`` and ``margin`` for ll4al.config.MARGIN.  ``task_model(images, targets)`` returns ``(features, {name: [N] losses})``
    (train.TrainableDetector over FasterRCNNTrainer(loss_mode="ll")) or ``(feature list, {name: (mean, [N scalars])})`` (over a
    RetinaNetLLTrainer); the loss dict's keys choose the reference's 'faster' or 'retina' branch, not an ``args.model`` string.  Warm-up
    of both optimizers in epoch 0, the finite-loss stop, both zero_grad / step pairs.  Returns one dict per iteration: task_loss, ll_loss, task_lr, ll_lr (the reference
    returns its MetricLogger).  Single process (no reduce_dict)."""
    from .engine import warmup_lr_scheduler
    task_model.train()
    ll_model.train()
    task_sched = ll_sched = None
    if epoch == 0:
        warmup_factor = 1. / 1000
        warmup_iters = min(1000, len(data_loader) - 1)
        if warmup_iters > 0:
            task_sched = warmup_lr_scheduler(task_optimizer, warmup_iters, warmup_factor)
            ll_sched = warmup_lr_scheduler(ll_optimizer, warmup_iters, warmup_factor)
    history = []
    for i, (images, targets) in enumerate(data_loader):
        images = list(image.to(device) for image in images)
        targets = [{k: v.to(device) for k, v in t.items()} for t in targets]
        features, task_loss_dict = task_model(images, targets)
        task_loss_dict = dict(task_loss_dict)
        if 'classification' in task_loss_dict:
            # the 'retina' branch (ll_train.py:97-120): every loss is (mean, [per image]), the features a list indexed by int
            _task_losses = sum(torch.stack(loss[1]) for loss in task_loss_dict.values())
            for k in ('classification', 'bbox_regression'):
                task_loss_dict[k] = task_loss_dict[k][0]
            task_losses = sum(loss for loss in task_loss_dict.values())
            task_loss_value = float(task_losses.detach())
            # After task_epochs epochs, stop the gradient from the loss prediction module propagated to the target model.
            features = {str(k): (features[k].detach() if epoch >= task_epochs else features[k]) for k in range(4)}
        else:
            _task_losses = sum(loss for loss in task_loss_dict.values())
            for k in ('loss_objectness', 'loss_rpn_box_reg', 'loss_classifier', 'loss_box_reg'):
                task_loss_dict[k] = torch.mean(task_loss_dict[k])
            task_losses = sum(loss for loss in task_loss_dict.values())
            task_loss_value = float(task_losses.detach())
            if epoch >= task_epochs:
                # After task_epochs epochs, stop the gradient from the loss prediction module propagated to the target model.
                features = {k: v for k, v in features.items()}
                for k in ('0', '1', '2', '3'):
                    features[k] = features[k].detach()
        ll_pred = ll_model(features)
        ll_pred = ll_pred.view(ll_pred.size(0))
        ll_loss = ll_weight * LossPredLoss(ll_pred, _task_losses, margin=margin)
        losses = task_losses + ll_loss
        if not math.isfinite(task_loss_value):
            print("Loss is {}, stopping training".format(task_loss_value))
            print({k: float(v.detach()) for k, v in task_loss_dict.items()})
            sys.exit(1)
        task_optimizer.zero_grad()
        ll_optimizer.zero_grad()
        losses.backward()
        task_optimizer.step()
        ll_optimizer.step()
        if task_sched is not None:
            task_sched.step()
        if ll_sched is not None:
            ll_sched.step()
        history.append(dict(task_loss=task_loss_value, ll_loss=float(ll_loss.detach()), task_lr=task_optimizer.param_groups[0]["lr"],
                            ll_lr=ll_optimizer.param_groups[0]["lr"]))
        if print_freq and i % print_freq == 0:
            print("Cycle:[{}] Epoch: [{}]  [{}/{}]  task_loss: {:.4f}  ll_loss: {:.4f}  task_lr: {:.6f}  ll_lr: {:.6f}".format(
                cycle, epoch, i, len(data_loader), task_loss_value, history[-1]["ll_loss"], history[-1]["task_lr"], history[-1]["ll_lr"]))
    return history
