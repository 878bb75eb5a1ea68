"""The Faster R-CNN training step (cald_amd/train.py states torchvision's semantics): six forward stages over one _Step record, the
hand-written backward with the box-head branch beside the RPN branch."""
import numpy as np
import torch

from . import train_ops as ops
from .train_core import _Conv, _LazyDict, _TrainerBase, _nchw_mask, anchor_slots, level_views, stride2_hw


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
    LAT_BODY = (0, 1, 2, 3)     # returned_layers = [1, 2, 3, 4]

    def __init__(self, state_dict, num_classes, depth=50, min_size=600, max_size=1000, device="cuda", trainable_layers=3,
                 rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=2000, rpn_nms_thresh=0.7, rpn_fg_iou=0.7, rpn_bg_iou=0.3,
                 rpn_batch=256, rpn_pos_fraction=0.5, box_fg_iou=0.5, box_bg_iou=0.5, box_batch=512, box_pos_fraction=0.25,
                 bbox_reg_weights=(10.0, 10.0, 5.0, 5.0), generator=None, sampler="choose_k", loss_mode=None, forward_precision="fp32",
                 backward_precision="fp32"):
        if loss_mode not in (None, "ll"):
            raise ValueError("loss_mode must be None or 'll', got %r" % (loss_mode,))
        # "ll": the learning-loss baseline's task model (detection/frcnn_ll.py): one loss per IMAGE (frcnn_ll.py:29-64, :243-276) and the
        # four pooled pyramid vectors LossNet reads (ll_train.py:77); None launches exactly what it always launched
        self.loss_mode = loss_mode
        self._init_common(state_dict, num_classes, depth, min_size, max_size, device, trainable_layers, generator, sampler,
                          forward_precision=forward_precision, backward_precision=backward_precision)
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
        self.refresh_f16x3_scales()

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
            level_hw.append(stride2_hw(level_hw[3]))
            head_sizes = [N * h * w * 16 for h, w in level_hw]
            anchors = self.anchors(Hp, Wp, level_hw)
            A_img = anchors.shape[0]
            # ---- RPN targets and sampling (anchor order: level, y, x, anchor).  One device->host copy of all match results, host-side
            # sampling (torch CPU generator), one host->device copy of every index the loss kernels need. ----
            slots = ([h * w for h, w in level_hw], 3, 16, N)             # head_flat: 3 anchors per pixel, rows of 16 floats
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
                rowp, ap_ = anchor_slots(i, sp, *slots); rown, an_ = anchor_slots(i, sn, *slots)
                obj_idx += [rowp + ap_, rown + an_]                      # channel a: anchor a's objectness logit
                obj_lab += [np.ones(len(sp), np.float32), np.zeros(len(sn), np.float32)]
                box_idx.append(rowp + 3 + 4 * ap_)                       # channel 3 + 4a of the same pixel
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
        self._hand_to_main(list(gts) + [s.gts_all, packed, s.obj_lab, s.rpn_tgt])    # what the main stream consumes from the batch-only stream

    def _fpn_rpn_head(self, s):
        """Stage 2: body, FPN (top-down), LastLevelMaxPool, the RPN head on the five levels."""
        s.feats = self._body(s.u8, s.rem, s.Hp, s.Wp, s.img_sizes)
        s.inner = self._fpn_top_down_fwd(s.feats)
        s.P = P = self._fpn_out_fwd(s.inner)
        P.append(ops.subsample2(P[3]))
        assert s.level_hw == [(p.shape[1], p.shape[2]) for p in P]
        # RPN head on the five levels: outputs in ONE buffer so that the loss kernels address (level, pixel, channel) by offset
        s.head_flat = torch.zeros(sum(s.head_sizes), dtype=torch.float32, device=self.dev)
        s.heads = []
        s.tl = tl = ops.conv_group(P, self.rpn_conv._packed(), pad=1, relu=True)     # shared 3x3 conv on the five levels: one launch
        for i, out in enumerate(level_views(s.head_flat, s.head_sizes, s.level_hw, s.N, 16)):
            s.heads.append(ops.conv(tl[i], self.rpn_head._packed(), out=out, out_ld=16))
            self.rpn_conv._count(P[i], 1); self.rpn_head._count(tl[i], 1)
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
        for i, t in enumerate(L["tl"]):
            out["rpn.%d" % i] = _nchw_mask(t)
        out["fc6"] = (L["f6"] > 0).view(L["R"], -1).cpu(); out["fc7"] = (L["f7"] > 0).view(L["R"], -1).cpu()
        return out

    def _rpn_branch_weights(self, L, g_obj, g_reg):
        """First half of the RPN branch: RPN losses -> gradient of the 1x1 head's output -> the weight gradients of the head and of the
        3x3 conv (shared weights: they accumulate over the five levels) and the head's data gradient (with the conv's ReLU backward).
        Returns that gradient per level -- what the 3x3 conv's data gradient (_rpn_branch_data) starts from."""
        P = L["P"]
        ghead_flat = torch.zeros_like(L["head_flat"])
        if self.loss_mode == "ll":                           # g_obj: the [4, N] per-image scales
            self._ll_losses(L, gs=g_obj, ghead=ghead_flat, which=(2, 3))
        else:
            ops.bce_logits(L["head_flat"], L["obj_idx"], L["obj_lab"], grad=ghead_flat, gscale=g_obj)
            ops.smooth_l1(L["head_flat"], L["box_idx"], L["rpn_tgt"], 1.0 / 9, L["obj_idx"].numel(), grad=ghead_flat, gscale=g_reg)
        ghs = level_views(ghead_flat, L["head_sizes"], L["level_hw"], L["N"], 16)
        for i in range(5):
            self.rpn_head.bwd(ghs[i], need_dx=False, accumulate=i > 0, x=L["tl"][i])
            self.rpn_head._count(L["tl"][i], 1)
        gts_ = ops.conv_group(ghs, self.rpn_head._packed_grad(), masks=L["tl"],       # 1x1 head: data gradient of the five levels + ReLU backward, one launch
                              Gs=self._dgrad_Gs([(self.rpn_head.idx, i) for i in range(5)], ghs))
        for i in range(5):
            self.rpn_conv.bwd(gts_[i], need_dx=False, accumulate=i > 0, x=P[i])
        return gts_

    def _rpn_branch_data(self, L, gts_):
        """Second half: the 3x3 conv's data gradient on the five levels -> gradients wrt P2..P5 and the pooled level."""
        P = L["P"]
        for i in range(5):
            self.rpn_conv._count(P[i], 1)
        g = ops.conv_group(gts_, self.rpn_conv._packed_grad(), pad=1,       # the five levels in one launch, like the forward
                           Gs=self._dgrad_Gs([(self.rpn_conv.idx, i) for i in range(5)], gts_))
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
        R, P = L["R"], L["P"]
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
        gC = self._fpn_top_down_bwd(self._fpn_out_bwd(gP[:4]))
        self._mark("bwd fpn")
        self._body_backward(gC)
        self._mark("bwd body dgrad")
        self._end_backward()
        self._join_side()
        return self.grads
