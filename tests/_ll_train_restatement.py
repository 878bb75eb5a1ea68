"""Float64 restatement of the learning-loss TRAINING step (test infrastructure): the per-image Faster R-CNN task losses
(detection/frcnn_ll.py:29-64, :243-276), LossNet under autograd (ll4al/models/lossnet.py), LossPredLoss (ll4al/main.py:64-83) and the
epoch loop of ll_train.py:55-142 with SGD + the warm-up schedule.  tests/test_ll_train.py pins it to the executed reference
(tests/golden/lossnet_train.npz, tests/golden/frcnn_losses.npz); tests/test_gpu_ll_train.py checks the HIP path against it.

Decisions a float32 implementation may take differently within its rounding noise -- LossNet's ReLUs, the hinge and the sign of
LossPredLoss -- can be handed in (``relu_masks``) or are guarded: ``guard`` is the distance every hinge / sign decision must keep
from flipping."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_train as tt

LOSS_NAMES = ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")
FC_KEYS = tuple("FC%d" % j for j in range(1, 5))


def f64(a):
    return torch.as_tensor(np.asarray(a)).double()


# ---- per-image task losses -------------------------------------------------------------------------------------------------------
def fastrcnn_loss_per_image(logits, breg, labels, targets, counts):
    """frcnn_ll.py:29-64 on the TRUE per-image row counts: cross entropy = mean over image i's rows, box loss = smooth_l1(beta 1, sum) over
    its foreground rows / its row count.  logits [R][C], breg [R][4 C], labels int64 [R], targets [R][4]."""
    cls, box, o = [], [], 0
    for n in counts:
        sl = slice(o, o + n); o += n
        lab = labels[sl]
        cls.append(F.cross_entropy(logits[sl], lab))
        pos = torch.nonzero(lab > 0).squeeze(1)
        br = breg[sl].reshape(n, -1, 4)
        box.append(F.smooth_l1_loss(br[pos, lab[pos]], targets[sl][pos], reduction="sum") / n)
    return torch.stack(cls), torch.stack(box)


def rpn_loss_per_image(obj, deltas, targets, pos, neg):
    """frcnn_ll.py:243-276 for one image: obj [A], deltas [A][4], targets [A][4], sampled positive / negative anchor indices."""
    samp = torch.cat([pos, neg])
    lab = torch.cat([torch.ones(len(pos)), torch.zeros(len(neg))]).to(obj.dtype)
    box = F.l1_loss(deltas[pos], targets[pos], reduction="sum") / samp.numel()
    return F.binary_cross_entropy_with_logits(obj[samp], lab), box


class TorchTrainFRCNNLL(tt.TorchTrainFRCNN):
    """TorchTrainFRCNN with detection/frcnn_ll.py's per-image losses; ``losses_ll`` also returns the pyramid (rec["P"]) whose global
    averages are LossNet's inputs."""

    def losses_ll(self, images, targets, proposals, cfg=None, samples=None):
        cfg = dict(dict(rpn_fg=0.7, rpn_bg=0.3, rpn_batch=256, rpn_pos=0.5, box_fg=0.5, box_bg=0.5, box_batch=512, box_pos=0.25, w=(10.0, 10.0, 5.0, 5.0)),
                   **(cfg or {}))

        def draw(kind, i, pos, neg, batch, frac):
            sp, sn = [torch.as_tensor(np.asarray(v), dtype=torch.int64) for v in samples[kind][i]]
            num_pos = min(int(batch * frac), pos.numel())
            assert len(sp) == num_pos and len(sn) == min(batch - num_pos, neg.numel()), "sampler sizes"
            assert set(sp.tolist()) <= set(pos.tolist()) and set(sn.tolist()) <= set(neg.tolist()), "sampled outside the candidate sets"
            return sp, sn
        p, N = self.p, len(images)
        batch, gts, Hp, Wp = self.batch(images, targets)
        P = self.backbone(batch)
        obj, deltas, anchors = [], [], []
        for l, f in enumerate(P):
            t = self.relu(F.conv2d(f, p["rpn.head.conv.weight"], p["rpn.head.conv.bias"], padding=1), "rpn.%d" % l)
            o = F.conv2d(t, p["rpn.head.cls_logits.weight"], p["rpn.head.cls_logits.bias"])
            d = F.conv2d(t, p["rpn.head.bbox_pred.weight"], p["rpn.head.bbox_pred.bias"])
            obj.append(o.permute(0, 2, 3, 1).reshape(N, -1)); deltas.append(d.permute(0, 2, 3, 1).reshape(N, -1, 4))
            Hl, Wl = f.shape[-2:]
            base = torch.from_numpy(tt.orc.base_anchors([32.0 * 2 ** l], [0.5, 1.0, 2.0])).float().reshape(-1, 4)
            ys, xs = torch.meshgrid(torch.arange(Hl) * (Hp // Hl), torch.arange(Wl) * (Wp // Wl), indexing="ij")
            anchors.append((torch.stack([xs, ys, xs, ys], dim=-1).reshape(-1, 1, 4).float() + base[None]).reshape(-1, 4))
        obj, deltas, anchors = torch.cat(obj, dim=1), torch.cat(deltas, dim=1), torch.cat(anchors)
        A = anchors.shape[0]
        l_obj, l_rpn = [], []
        for i in range(N):
            m = tt.matcher(tt.box_iou(gts[i], anchors), cfg["rpn_fg"], cfg["rpn_bg"], True) if gts[i].shape[0] else torch.full((A,), -1, dtype=torch.int64)
            pos, neg = torch.nonzero(m >= 0).squeeze(1), torch.nonzero(m == -1).squeeze(1)
            sp, sn = draw("rpn", i, pos, neg, cfg["rpn_batch"], cfg["rpn_pos"])
            sp, sn = sp.sort().values, sn.sort().values
            tgt = torch.zeros(A, 4, dtype=torch.float64)
            if len(sp):
                tgt[sp] = tt.encode(gts[i][m[sp]].double(), anchors[sp].double(), (1.0, 1.0, 1.0, 1.0))
            a, b = rpn_loss_per_image(obj[i], deltas[i], tgt, sp, sn)
            l_obj.append(a); l_rpn.append(b)
        r_img, r_box, r_lab, r_tgt, counts = [], [], [], [], []
        for i in range(N):
            pr = torch.cat([proposals[i].float(), gts[i]]) if gts[i].shape[0] else proposals[i].float()
            if gts[i].shape[0] == 0:
                m = torch.full((pr.shape[0],), -1, dtype=torch.int64); labels = torch.zeros(pr.shape[0], dtype=torch.int64)
            else:
                m = tt.matcher(tt.box_iou(gts[i], pr), cfg["box_fg"], cfg["box_bg"], False)
                labels = targets[i]["labels"].long()[m.clamp(min=0)].clone()
                labels[m == -1] = 0
                labels[m == -2] = -1
            pos, neg = torch.nonzero(labels >= 1).squeeze(1), torch.nonzero(labels == 0).squeeze(1)
            sp, sn = draw("box", i, pos, neg, cfg["box_batch"], cfg["box_pos"])
            keep = torch.cat([sp, sn]).sort().values
            counts.append(len(keep))
            r_img.append(torch.full((len(keep),), i, dtype=torch.int64)); r_box.append(pr[keep]); r_lab.append(labels[keep])
            mg = gts[i][m[keep].clamp(min=0)] if gts[i].shape[0] else torch.zeros(len(keep), 4)
            r_tgt.append(tt.encode(mg.double(), pr[keep].double(), cfg["w"]))
        r_img, r_box, r_lab, r_tgt = torch.cat(r_img), torch.cat(r_box), torch.cat(r_lab), torch.cat(r_tgt)
        feat = tt.roi_align(P[:4], r_img, r_box)
        h = self.relu(F.linear(feat.flatten(1), p["roi_heads.box_head.fc6.weight"], p["roi_heads.box_head.fc6.bias"]), "fc6")
        h = self.relu(F.linear(h, p["roi_heads.box_head.fc7.weight"], p["roi_heads.box_head.fc7.bias"]), "fc7")
        logits = F.linear(h, p["roi_heads.box_predictor.cls_score.weight"], p["roi_heads.box_predictor.cls_score.bias"])
        breg = F.linear(h, p["roi_heads.box_predictor.bbox_pred.weight"], p["roi_heads.box_predictor.bbox_pred.bias"])
        l_cls, l_box = fastrcnn_loss_per_image(logits, breg, r_lab, r_tgt, counts)
        rec = dict(P=P, roi_labels=r_lab, counts=counts)
        return {"loss_classifier": l_cls, "loss_box_reg": l_box, "loss_objectness": torch.stack(l_obj), "loss_rpn_box_reg": torch.stack(l_rpn)}, rec


# ---- LossNet and LossPredLoss --------------------------------------------------------------------------------------------------
def pooled_of(maps):
    """AdaptiveAvgPool2d(1) of four [B, 256, H, W] maps -> [B, 4, 256]"""
    return torch.stack([m.mean(dim=(2, 3)) for m in maps], dim=1)


def lossnet(sd, pooled, relu_masks=None):
    """ll4al/models/lossnet.py:46-65 on pooled [B, 4, 256] (float64).  relu_masks: None or [B, 4, D] bool -- the ReLU decisions of the
    implementation under test (see TorchTrainFRCNN.relu).  Returns (pred [B], hidden [B, 4, D])."""
    hs = []
    for j, fc in enumerate(FC_KEYS):
        z = F.linear(pooled[:, j], sd[fc + ".weight"], sd[fc + ".bias"])
        hs.append(z * relu_masks[:, j].to(z.dtype) if relu_masks is not None else F.relu(z))
    pred = F.linear(torch.cat(hs, dim=1), sd["linear.weight"], sd["linear.bias"])
    return pred.view(-1), torch.stack(hs, dim=1)


def loss_pred_loss(inp, target, margin=1.0, reduction="mean", guard=None):
    """ll4al/main.py:64-83.  guard: every sign decision |t_i - t_(B-1-i)| (ties excepted: a tie is -1 on both sides) and every hinge
    decision |margin - one * diff| must be at least this far from flipping."""
    if len(inp) % 2:
        raise ValueError("the batch size is not even.")
    half = len(inp) // 2
    d = (inp - inp.flip(0))[:half]
    t = (target - target.flip(0))[:half].detach()
    one = 2 * torch.sign(torch.clamp(t, min=0)) - 1
    x = margin - one * d
    if guard is not None:
        assert bool(((t.abs() >= guard) | (t == 0)).all()), "a sign decision of LossPredLoss is within %g of flipping" % guard
        assert bool((x.detach().abs() >= guard).all()), "a hinge decision of LossPredLoss is within %g of flipping" % guard
    terms = torch.clamp(x, min=0)
    return terms if reduction == "none" else terms.sum() / half


# ---- the epoch loop ---------------------------------------------------------------------------------------------------------------
def warmup_factor(x, warmup_iters, factor=1.0 / 1000):
    if x >= warmup_iters:
        return 1.0
    a = float(x) / warmup_iters
    return factor * (1 - a) + a


def train_epoch(sd0, feats, losses, task_epochs, epoch=0, lr=0.01, momentum=0.9, weight_decay=1e-4, ll_weight=1.0, margin=1.0):
    """ll_train.py:55-142 for LossNet's side.  feats[it] = four [B, 256, H, W] maps, losses[it] = {name: [B]} (the values the task model
    returned).  Returns per iteration: LossNet's state after the step, ll_loss, the lr the reference logs (after the scheduler's step), and
    the maps' gradients (None when detached)."""
    sd = {k: f64(v).clone().requires_grad_(True) for k, v in sd0.items()}
    bufs = {}
    n = len(feats)
    warm = min(1000, n - 1) if epoch == 0 else 0
    out = []
    for it in range(n):
        cur_lr = lr * (warmup_factor(it, warm) if warm > 0 else 1.0)
        maps = [f64(f).requires_grad_(True) for f in feats[it]]
        target = sum(f64(losses[it][k]) for k in LOSS_NAMES)
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
