"""The RetinaNet that trains LossNet beside it (detection/retina_ll.py; ll_train.py:97-120): RetinaNetTrainer with one loss per IMAGE
and the four pooled pyramid vectors LossNet reads.  Only the loss stage and the two ends of the heads' backward differ from the parent."""
import torch

from . import train_ops as ops
from .train_retina import RetinaNetTrainer, _RetinaStep


class RetinaNetLLTrainer(RetinaNetTrainer):
    """detection/retina_ll.py RetinaNet in train mode: the classification loss of image n = focal sum / max(1, #fg_n) (:127-131), its
    regression loss = L1 sum / max(1, #fg_n) (:215-219), their means over the batch (:132, :220) and ``features[0..3]`` (:529) -- P3, P4,
    P5 and P6 before its ReLU, pooled here because the maps never exist in torch's layout."""
    loss_mode = "ll"
    LL_MEANS = True             # the autograd bridge also hands out the two means (retina_ll.py returns (mean, [per image]))

    def __init__(self, state_dict, num_classes, **kw):
        if kw.pop("loss_mode", "ll") != "ll":
            raise ValueError("RetinaNetLLTrainer is the loss_mode 'll' model; the plain one is RetinaNetTrainer")
        RetinaNetTrainer.__init__(self, state_dict, num_classes, **kw)
        self.loss_mode = "ll"

    def _losses(self, s):
        """Stage 4: the step's record, the per-image focal and L1 losses with their means, the pooled pyramid vectors.
        Returns ({name: [N]}, pooled [N, 4, 256]); ``self.last["means"]``: {name: [1]}."""
        self.last = L = {k: getattr(s, k) for k in _RetinaStep.KEPT}
        L["fg_den"] = [float(max(1, n)) for n in s.nfg]
        means = torch.empty(2, dtype=torch.float32, device=self.dev)
        losses = self._ll_losses(L, means=means)
        L["means"] = {"classification": means[0:1], "bbox_regression": means[1:2]}
        L["pooled"] = ops.train_gap(s.P[:4])               # the batch's PADDED maps, as retina_ll.py:524-529 hands them out
        self._mark("losses")
        return losses, L["pooled"]

    def _ll_losses(self, L, gs=None, gcls=None, greg=None, means=None):
        g = (lambda i: None) if gs is None else (lambda i: gs[i])
        m = (lambda i: None) if means is None else (lambda i: means[i:i + 1])
        return {"classification": ops.focal_loss_seg(L["cls_flat"], L["level_pix"], L["N"], 9, self.K, self.cls_ld, L["matched"], L["gt_labels"],
                                                     L["gt_off"], L["fg_den"], grad=gcls, gscale=g(0), mean_out=m(0)),
                "bbox_regression": ops.smooth_l1_seg(L["reg_flat"], L["box_idx"], L["reg_tgt"], 0.0, L["nfg"], L["fg_den"], grad=greg, gscale=g(1),
                                                     mean_out=m(1))}

    def _loss_grads(self, L, gscale, gcls, greg):
        self._ll_losses(L, gs=gscale, gcls=gcls, greg=greg)

    def backward(self, gscale=(1.0, 1.0), g_pooled=None):
        """Gradients of sum_n gscale[0][n] * classification_n + gscale[1][n] * bbox_regression_n into the flat gradient buffer.  gscale is
        [2][N]: a float or a sequence per loss, or a device tensor (never read back).  g_pooled (optional, [N, 4, 256]): the gradient LossNet
        sends into the pooled vectors; it joins the gradients of P3..P6 in the kernel that adds the two towers' maps."""
        L = self.last
        if not torch.is_tensor(gscale):
            gscale = torch.tensor([[float(v)] * L["N"] if not hasattr(v, "__len__") else [float(x) for x in v] for v in gscale], dtype=torch.float32)
        gscale = gscale.to(self.dev, torch.float32).contiguous()
        assert tuple(gscale.shape) == (2, L["N"]), "gscale must be [2][N] in loss_mode 'll'"
        if g_pooled is not None:
            g_pooled = g_pooled.to(torch.float32).contiguous()
            assert tuple(g_pooled.shape) == tuple(L["pooled"].shape)
        self._fpn_backward(self._heads_backward(gscale, g_pooled))
        self._end_backward()
        self._join_side()
        return self.grads
