"""Float64 restatement of RetinaNet's side of the learning-loss TRAINING step (test infrastructure): the per-image head losses of
detection/retina_ll.py:100-132 and :183-220, the training forward that also hands out the pyramid (:523-554), and the 'retina' branch of
the epoch loop (ll_train.py:97-120).  tests/test_retina_ll_train.py pins it to the executed reference (tests/golden/retina_ll_train.npz);
tests/test_gpu_retina_ll_ops.py and tests/test_gpu_train_retina_ll.py check the HIP path against it.  LossNet, LossPredLoss, the pooling and
the warm-up schedule are those of _ll_train_restatement."""
import torch
import torch.nn.functional as F

from oracle import torch_train as tt

from _ll_train_restatement import f64, loss_pred_loss, lossnet, pooled_of, warmup_factor

LOSS_NAMES = ("classification", "bbox_regression")


def retina_losses_per_image(cls, reg, anchors, gts, labels, matched):
    """retina_ll.py:100-132 and :183-220 with the matcher's decisions given: cls [N][A][K], reg [N][A][4], anchors [A][4], per-image gt
    boxes / labels, matched [N][A] int64 (-1 background, -2 ignored).  Returns ((cls mean, [N]), (reg mean, [N])); a mean is
    ``_sum(losses) / len(targets)``, added in image order."""
    N = len(gts)
    lc, lr = [], []
    for i in range(N):
        m = torch.as_tensor(matched[i]).long()
        fg = m >= 0
        nfg = max(1, int(fg.sum()))
        tgt = torch.zeros_like(cls[i])
        tgt[fg, labels[i].long()[m[fg]]] = 1.0
        valid = m != -2
        lc.append(tt.sigmoid_focal_loss_sum(cls[i][valid], tgt[valid]) / nfg)
        t_reg = tt.encode(gts[i][m.clamp(min=0)][fg].to(reg.dtype), anchors[fg].to(reg.dtype), (1.0, 1.0, 1.0, 1.0))
        lr.append((reg[i][fg] - t_reg).abs().sum() / nfg)
    return (sum(lc) / N, torch.stack(lc)), (sum(lr) / max(1, N), torch.stack(lr))


class TorchTrainRetinaNetLL(tt.TorchTrainRetinaNet):
    """TorchTrainRetinaNet's forward with detection/retina_ll.py's returns: ``losses_ll`` gives {name: [N]}, and in rec the two means and
    the pyramid ``P`` (P3, P4, P5, P6 before its ReLU, P7) whose first four global averages are LossNet's inputs."""

    def losses_ll(self, images, targets, cfg=None, matched=None):
        p, N, K = self.p, len(images), self.C
        batch, gts, Hp, Wp = self.batch(images, targets)
        feats = self.body(batch)
        inner = [None] * 3
        inner[2] = F.conv2d(feats[3], p["backbone.fpn.inner_blocks.2.weight"], p["backbone.fpn.inner_blocks.2.bias"])
        for i in (1, 0):
            lat = F.conv2d(feats[i + 1], p["backbone.fpn.inner_blocks.%d.weight" % i], p["backbone.fpn.inner_blocks.%d.bias" % i])
            inner[i] = lat + F.interpolate(inner[i + 1], size=lat.shape[-2:], mode="nearest")
        P = [F.conv2d(inner[i], p["backbone.fpn.layer_blocks.%d.weight" % i], p["backbone.fpn.layer_blocks.%d.bias" % i], padding=1) for i in range(3)]
        p6 = F.conv2d(P[2], p["backbone.fpn.extra_blocks.p6.weight"], p["backbone.fpn.extra_blocks.p6.bias"], stride=2, padding=1)
        p7 = F.conv2d(self.relu(p6, "p6"), p["backbone.fpn.extra_blocks.p7.weight"], p["backbone.fpn.extra_blocks.p7.bias"], stride=2, padding=1)
        P += [p6, p7]
        cls, reg = [], []
        for l, f in enumerate(P):
            for name, head, outs, last in (("cls", "classification_head", cls, "cls_logits"), ("reg", "regression_head", reg, "bbox_reg")):
                t = f
                for j in range(4):
                    t = self.relu(F.conv2d(t, p["head.%s.conv.%d.weight" % (head, 2 * j)], p["head.%s.conv.%d.bias" % (head, 2 * j)], padding=1), "%s.%d.%d" % (name, l, j))
                o = F.conv2d(t, p["head.%s.%s.weight" % (head, last)], p["head.%s.%s.bias" % (head, last)], padding=1)
                Nn, _, H, W = o.shape
                c = K if name == "cls" else 4
                outs.append(o.view(Nn, -1, c, H, W).permute(0, 3, 4, 1, 2).reshape(Nn, -1, c))
        cls, reg = torch.cat(cls, dim=1), torch.cat(reg, dim=1)
        anchors = []
        for l, f in enumerate(P):
            Hl, Wl = f.shape[-2:]
            x = 32 * 2 ** l
            base = torch.from_numpy(tt.orc.base_anchors([float(x), float(int(x * 2 ** (1.0 / 3))), float(int(x * 2 ** (2.0 / 3)))], [0.5, 1.0, 2.0])).float().reshape(-1, 4)
            ys, xs = torch.meshgrid(torch.arange(Hl) * (Hp // Hl), torch.arange(Wl) * (Wp // Wl), indexing="ij")
            anchors.append((torch.stack([xs, ys, xs, ys], dim=-1).reshape(-1, 1, 4).float() + base[None]).reshape(-1, 4))
        anchors = torch.cat(anchors)
        cfg = dict(dict(fg=0.5, bg=0.4), **(cfg or {}))
        if matched is None:
            matched = [tt.matcher(tt.box_iou(g, anchors), cfg["fg"], cfg["bg"], True) for g in gts]
        (cm, cl), (rm, rl) = retina_losses_per_image(cls, reg, anchors, gts, [t["labels"] for t in targets], matched)
        rec = dict(anchors=anchors, matched=torch.stack([torch.as_tensor(m).long() for m in matched]), P=P,
                   means={"classification": cm, "bbox_regression": rm})
        return {"classification": cl, "bbox_regression": rl}, rec


def train_epoch_retina(sd0, feats, losses, task_epochs, epoch=0, lr=0.01, momentum=0.9, weight_decay=1e-4, ll_weight=1.0, margin=1.0):
    """ll_train.py:55-142 through its 'retina' branch, LossNet's side.  feats[it] = the feature LIST (four or five [B, 256, H, W] maps, the
    loop reads [0..3]), losses[it] = {name: [B]} (the per-image values the task model returned; LossPredLoss's target is their sum over
    the names).  Returns per iteration what _ll_train_restatement.train_epoch returns."""
    sd = {k: f64(v).clone().requires_grad_(True) for k, v in sd0.items()}
    bufs = {}
    n = len(feats)
    warm = min(1000, n - 1) if epoch == 0 else 0
    out = []
    for it in range(n):
        cur_lr = lr * (warmup_factor(it, warm) if warm > 0 else 1.0)
        maps = [f64(f).requires_grad_(True) for f in feats[it][:4]]
        target = sum(torch.stack(list(f64(losses[it][k]).unbind(0))) for k in LOSS_NAMES)
        pooled = pooled_of(maps)
        if epoch >= task_epochs:
            pooled = pooled.detach()
        pred, _ = lossnet(sd, pooled)
        ll_loss = ll_weight * loss_pred_loss(pred, target, margin)
        for v in sd.values():
            v.grad = None
        ll_loss.backward()
        with torch.no_grad():
            for k, v in sd.items():                                   # torch.optim.SGD: weight decay, momentum, no dampening
                g = v.grad + weight_decay * v
                bufs[k] = g.clone() if k not in bufs else momentum * bufs[k] + g
                v -= cur_lr * bufs[k]
        next_lr = lr * (warmup_factor(it + 1, warm) if warm > 0 else 1.0)
        out.append(dict(sd={k: v.detach().clone() for k, v in sd.items()}, ll_loss=float(ll_loss.detach()), lr=next_lr,
                        gfeat=None if epoch >= task_epochs else [m.grad.clone() for m in maps]))
    return out
