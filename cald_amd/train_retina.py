"""The RetinaNet training step (detection/retinanet_cal.py): four forward stages over one _RetinaStep record, the hand-written
backward of the heads and of the FPN."""
import numpy as np
import torch

from . import train_ops as ops
from .train_core import _Conv, _TrainerBase, _nchw_mask, anchor_slots, level_views, stride2_hw


class _RetinaStep(object):
    """What the stages of one RetinaNetTrainer.forward hand to each other.  KEPT: the fields that become ``self.last`` (what backward(),
    the tests and the tools read of the last forward) -- all but the prepared input, which only _targets and _fpn read."""
    KEPT = ("N", "level_hw", "level_pix", "cls_sizes", "reg_sizes", "matched", "matched_host", "gt_labels", "gt_off", "box_idx", "box_w", "img_w",
            "reg_tgt", "nfg",                               # set by _targets
            "feats", "inner", "P", "p6_relu",               # by _fpn
            "acts", "cls_flat", "reg_flat")                 # by _heads
    __slots__ = KEPT + ("u8", "rem", "Hp", "Wp", "img_sizes")


class RetinaNetTrainer(_TrainerBase):
    """The trainable mirror of detection/retinanet_cal.py RetinaNet (ResNet-50 FPN, P3-P7, 9 anchors per location): training forward
    :545-564, matcher :389-400 (IoU 0.5 / 0.4, low-quality matches), classification loss :100-133 (sigmoid focal loss, sum over the
    anchors outside the ignore band / max(1, #foreground), mean over images), regression loss :185-221 (L1 on the foreground
    anchors / max(1, #foreground), mean over images).  As in the reference, every image must carry at least one box."""
    LOSS_NAMES = ("classification", "bbox_regression")
    ANCHOR_KIND = 1
    LAT_BODY = (1, 2, 3)        # returned_layers = [2, 3, 4]

    def __init__(self, state_dict, num_classes, depth=50, min_size=600, max_size=1000, device="cuda", trainable_layers=3,
                 fg_iou_thresh=0.5, bg_iou_thresh=0.4, generator=None, loss_mode=None, forward_precision="fp32",
                 backward_precision="fp32"):
        if loss_mode not in (None, "ll"):
            raise ValueError("loss_mode must be None or 'll', got %r" % (loss_mode,))
        if loss_mode is not None:
            raise NotImplementedError("loss_mode=%r: the RetinaNet that trains LossNet beside it (ll_train.py:97-120, retina_ll.py's per-image "
                                      "losses) is a model of its own, as in the reference: build a RetinaNetLLTrainer" % (loss_mode,))
        self.loss_mode = None
        self._init_common(state_dict, num_classes, depth, min_size, max_size, device, trainable_layers, generator, forward_precision=forward_precision,
                          backward_precision=backward_precision)
        self.cfg = dict(fg=fg_iou_thresh, bg=bg_iou_thresh)
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
        self.refresh_f16x3_scales()

    def forward(self, images, targets):
        """Training forward.  Returns the two losses as 1-element device tensors (no autograd) and keeps what backward needs."""
        s = _RetinaStep()
        s.N = len(images)
        self._mark("start")
        self._begin_step()
        s.u8, s.rem = self._prepare_images(images)          # on the main stream: the images may have just been produced there
        self._targets(s, targets)
        self._fpn(s)
        self._heads(s)
        return self._losses(s)

    def _targets(self, s, targets):
        """Stage 1, on the batch-only stream: input sizes, ground truth (at least one box per image), anchor matching -- whose copy to the
        host is the forward's one host stop -- the regression loss's index list, targets and normalisers, handed to the main stream."""
        N = s.N
        with self._aux_stream():        # first and on its own stream: the copy of the match results does not wait for the network's kernels
            s.u8, s.rem, Hp, Wp, s.img_sizes, gts, gt_labels = self._inputs(s.u8, s.rem, targets)
            s.Hp, s.Wp = Hp, Wp
            if any(g.shape[0] == 0 for g in gts):
                raise ValueError("RetinaNet training needs at least one ground-truth box per image (retinanet_cal.py:110-124)")
            level_hw = [(Hp // 8, Wp // 8), (Hp // 16, Wp // 16), (Hp // 32, Wp // 32)]
            for _ in range(2):                              # P6, P7: 3x3 stride-2 convs with padding 1
                level_hw.append(stride2_hw(level_hw[-1]))
            s.level_hw, s.level_pix = level_hw, [h * w for h, w in level_hw]
            s.cls_sizes, s.reg_sizes = [N * n * self.cls_ld for n in s.level_pix], [N * n * 36 for n in s.level_pix]
            anchors = self.anchors(Hp, Wp, level_hw)
            s.matched = torch.empty((N, anchors.shape[0]), dtype=torch.int32, device=self.dev)
            for i in range(N):
                ops.match(anchors, gts[i], self.cfg["fg"], self.cfg["bg"], True, out=s.matched[i])
            s.matched_host = s.matched.cpu().numpy()
            n_gt = [int(g.shape[0]) for g in gts]
            gt_off = np.cumsum([0] + n_gt)
            gts_all = torch.cat(gts)
            box_idx, anc_idx, gt_idx, wts, nfg = [], [], [], [], []
            for i in range(N):
                m = s.matched_host[i]
                fg = np.flatnonzero(m >= 0)
                row, a = anchor_slots(i, fg, s.level_pix, 9, 36, N)      # reg_flat: 9 anchors per pixel, rows of 36 floats
                box_idx.append(row + 4 * a)
                anc_idx.append(fg); gt_idx.append(gt_off[i] + m[fg])
                nfg.append(len(fg)); wts.append(np.full(len(fg), 1.0 / (max(1, len(fg)) * N), np.float32))
            box_idx, anc_idx, gt_idx = [np.concatenate(v).astype(np.int64) for v in (box_idx, anc_idx, gt_idx)]
            packed = torch.from_numpy(np.concatenate([box_idx, anc_idx, gt_idx])).to(self.dev)
            nb = len(box_idx)
            s.box_idx, anc_sel, gt_sel = packed[:nb], packed[nb:2 * nb], packed[2 * nb:]
            fl = torch.from_numpy(np.concatenate([np.concatenate(wts), np.array([1.0 / (max(1, n) * N) for n in nfg], np.float32)])).to(self.dev)
            s.box_w, s.img_w = fl[:nb], fl[nb:]
            s.nfg = nfg                                     # host: the per-image losses' segments and normalisers (RetinaNetLLTrainer)
            s.reg_tgt = ops.box_encode(gts_all[gt_sel], anchors[anc_sel], (1.0, 1.0, 1.0, 1.0))
            s.gt_labels = torch.cat(gt_labels).to(self.dev)
            s.gt_off = torch.from_numpy(gt_off.astype(np.int32)).to(self.dev)
        self._hand_to_main(list(gts) + [gts_all, packed, fl, s.reg_tgt, s.matched, s.gt_labels, s.gt_off])
        self._mark("targets")

    def _fpn(self, s):
        """Stage 2, on the main stream: body, FPN (top-down) P3..P5, P6 from P5, P7 from relu(P6)."""
        s.feats = self._body(s.u8, s.rem, s.Hp, s.Wp, s.img_sizes)
        s.inner = self._fpn_top_down_fwd(s.feats)
        s.P = P = self._fpn_out_fwd(s.inner)
        P.append(self.p6.fwd(P[2]))
        s.p6_relu = ops.relu_bwd_(ops.add(P[3]), P[3])                     # relu(p6): x * (x > 0) on a copy
        P.append(self.p7.fwd(s.p6_relu))
        assert s.level_hw == [(p.shape[1], p.shape[2]) for p in P]

    def _heads(self, s):
        """Stage 3, on the main stream: both four-conv towers on the five levels (one grouped launch per tower layer), then each head's
        output conv on the five levels (one grouped launch each) into its flat buffer."""
        P = s.P
        # head outputs of the five levels in ONE buffer each (level block l = [N][pix_l][ld])
        s.cls_flat = torch.zeros(sum(s.cls_sizes), dtype=torch.float32, device=self.dev)
        s.reg_flat = torch.empty(sum(s.reg_sizes), dtype=torch.float32, device=self.dev)
        # both towers on the five levels: ten problems of one shape per launch (the small levels fill the tail of the large ones)
        s.acts = acts = {"cls": [[P[l]] for l in range(5)], "reg": [[P[l]] for l in range(5)]}
        for j in range(4):
            xs = [acts["cls"][l][-1] for l in range(5)] + [acts["reg"][l][-1] for l in range(5)]
            ys = ops.conv_group(xs, [self.cls_tower[j]._packed()] * 5 + [self.reg_tower[j]._packed()] * 5, pad=1, relu=True)
            for l in range(5):
                self.cls_tower[j]._count(xs[l], 1); self.reg_tower[j]._count(xs[5 + l], 1)
                acts["cls"][l].append(ys[l]); acts["reg"][l].append(ys[5 + l])
        for l in range(5):
            self.cls_out._count(acts["cls"][l][4], 1); self.reg_out._count(acts["reg"][l][4], 1)
        ops.conv_group([acts["cls"][l][4] for l in range(5)], self.cls_out._packed(), pad=1,
                       outs=level_views(s.cls_flat, s.cls_sizes, s.level_hw, s.N, self.cls_ld), out_ld=self.cls_ld)
        ops.conv_group([acts["reg"][l][4] for l in range(5)], self.reg_out._packed(), pad=1,
                       outs=level_views(s.reg_flat, s.reg_sizes, s.level_hw, s.N, 36), out_ld=36)
        self._mark("fpn+heads")

    def _losses(self, s):
        """Stage 4, on the main stream: the step's record for backward() and inspection, then the focal and the L1 loss."""
        self.last = {k: getattr(s, k) for k in _RetinaStep.KEPT}
        losses = {"classification": ops.focal_loss(s.cls_flat, s.level_pix, s.N, 9, self.K, self.cls_ld, s.matched, s.gt_labels, s.gt_off, s.img_w),
                  "bbox_regression": ops.smooth_l1(s.reg_flat, s.box_idx, s.reg_tgt, 0.0, 1.0, weights=s.box_w)}
        self._mark("losses")
        return losses

    def relu_decisions(self):
        L, out = self.last, self.body_relu_decisions()
        for name in ("cls", "reg"):
            for l, xs in enumerate(L["acts"][name]):
                for j in range(4):
                    out["%s.%d.%d" % (name, l, j)] = _nchw_mask(xs[j + 1])
        out["p6"] = _nchw_mask(L["P"][3])
        return out

    def backward(self, gscale=(1.0, 1.0)):
        """Gradients of gscale[0] * classification + gscale[1] * bbox_regression into the flat gradient buffer."""
        self._fpn_backward(self._heads_backward(gscale))
        self._end_backward()
        self._join_side()
        return self.grads

    def _loss_grads(self, L, gscale, gcls, greg):
        """The two losses' gradients into the zeroed head-output gradient buffers."""
        ops.focal_loss(L["cls_flat"], L["level_pix"], L["N"], 9, self.K, self.cls_ld, L["matched"], L["gt_labels"], L["gt_off"], L["img_w"], grad=gcls, gscale=gscale[0])
        ops.smooth_l1(L["reg_flat"], L["box_idx"], L["reg_tgt"], 0.0, 1.0, weights=L["box_w"], grad=greg, gscale=gscale[1])

    def _heads_backward(self, gscale, g_pooled=None):
        """Both losses' gradients, then the output convs and the towers backwards: weight gradients level by level (shared weights
        accumulate; they run on the side stream), data gradients of one layer of BOTH towers on all five levels in one grouped launch.
        Returns the gradients wrt P3..P7; g_pooled ([N, 4, 256], RetinaNetLLTrainer) joins those of P3..P6 in the same pass."""
        L = self.last
        N, level_hw, acts = L["N"], L["level_hw"], L["acts"]
        gcls = torch.zeros_like(L["cls_flat"]); greg = torch.zeros_like(L["reg_flat"])
        self._loss_grads(L, gscale, gcls, greg)
        g_cls = level_views(gcls, L["cls_sizes"], level_hw, N, self.cls_ld)
        g_reg = level_views(greg, L["reg_sizes"], level_hw, N, 36)
        for l in range(5):
            self.cls_out.bwd(g_cls[l], need_dx=False, accumulate=l > 0, x=acts["cls"][l][4])
            self.reg_out.bwd(g_reg[l], need_dx=False, accumulate=l > 0, x=acts["reg"][l][4])
            self.cls_out._count(acts["cls"][l][4], 1); self.reg_out._count(acts["reg"][l][4], 1)
        # every ReLU backward of the towers rides in the epilogue of the data gradient that produces its input gradient
        g_cls = ops.conv_group(g_cls, self.cls_out._packed_grad(), pad=1, masks=[acts["cls"][l][4] for l in range(5)],
                               Gs=self._dgrad_Gs([(self.cls_out.idx, l) for l in range(5)], g_cls))
        g_reg = ops.conv_group(g_reg, self.reg_out._packed_grad(), pad=1)              # 36 channels: not a tiled-kernel shape
        for l in range(5):
            ops.relu_bwd_(g_reg[l], acts["reg"][l][4])
        for j in (3, 2, 1, 0):
            for l in range(5):
                self.cls_tower[j].bwd(g_cls[l], need_dx=False, accumulate=l > 0, x=acts["cls"][l][j])
                self.reg_tower[j].bwd(g_reg[l], need_dx=False, accumulate=l > 0, x=acts["reg"][l][j])
                self.cls_tower[j]._count(acts["cls"][l][j], 1); self.reg_tower[j]._count(acts["reg"][l][j], 1)
            masks = ([acts["cls"][l][j] for l in range(5)] + [acts["reg"][l][j] for l in range(5)]) if j > 0 else None
            keys = [(self.cls_tower[j].idx, l) for l in range(5)] + [(self.reg_tower[j].idx, l) for l in range(5)]
            gs = ops.conv_group(g_cls + g_reg, [self.cls_tower[j]._packed_grad()] * 5 + [self.reg_tower[j]._packed_grad()] * 5, pad=1, masks=masks,
                                Gs=self._dgrad_Gs(keys, g_cls + g_reg))
            g_cls, g_reg = gs[:5], gs[5:]
        if g_pooled is None:
            return [ops.add(g_cls[l], g_reg[l]) for l in range(5)]
        return [ops.add_bcast(g_cls[l], g_reg[l], g_pooled[:, l, :]) for l in range(4)] + [ops.add(g_cls[4], g_reg[4])]

    def _fpn_backward(self, gP):
        """P7 and P6 backwards into P5's gradient, the FPN output convs and the top-down pass backwards, then the body."""
        L = self.last
        P = L["P"]
        g6 = self.p7.bwd(gP[4], x=L["p6_relu"])
        ops.relu_bwd_(g6, P[3])
        g6 = ops.add(g6, gP[3])
        gP[2] = ops.add(gP[2], self.p6.bwd(g6, x=P[2]))
        self._body_backward(self._fpn_top_down_bwd(self._fpn_out_bwd(gP[:3])))
