"""An independent statement of the SSM tail (detection/frcnn_ssm.py:44-102 + transform.postprocess) for tests/test_ssm.py and
tests/test_gpu_ssm.py, and the scripted scenes of image_cross_validation that tools/make_golden_ssm.py runs through the reference.

The tail's float arithmetic comes from the `oracle` fixture, never from the library under test:
  * oracle.frcnn_postprocess on ONE proposal with a score threshold below every probability (-1) and an NMS threshold above every IoU
    (2), resized size == original size, returns all C - 1 (class, box) pairs of that proposal: the bit-exact softmax row (scores_cls) and
    the decoded, clipped boxes (times a ratio of exactly 1.0);
  * oracle.batched_nms with every group equal to c is the per-class NMS: boxes + c * (max over the class's boxes + 1) in float32,
    (score desc, index asc), greedy, the first max_keep;
  * oracle.resize_boxes scales to the original image.
What is stated HERE is the bookkeeping the issue describes: the al flag, the class loop, the cut at det_max, the score cut, the row order,
the labels.  nms_margins repeats the greedy pass in float32 numpy only to MEASURE how far every IoU decision lies from the threshold.
"""
import random

import numpy as np

F32 = np.float32


def check_exp(orc):
    """The exp behind the oracle's softmax: exactly 1 at 0 and exactly 0 at -200 (the al-boundary cases are built on both)."""
    y = orc.exp_array(np.array([0.0, -200.0], F32))
    assert y[0] == F32(1.0) and y[1] == F32(0.0), y


def rows(orc, logits, deltas, props, Hr, Wr):
    """prob [R][C] (softmax) and cbox [R][C-1][4] (decoded with (10, 10, 5, 5), clipped to (Hr, Wr)), one oracle call a proposal."""
    logits = np.ascontiguousarray(logits, F32); deltas = np.ascontiguousarray(deltas, F32); props = np.ascontiguousarray(props, F32).reshape(-1, 4)
    R, C = logits.shape
    prob = np.zeros((R, C), F32); cbox = np.zeros((R, C - 1, 4), F32)
    for r in range(R):
        o = orc.frcnn_postprocess(logits[r:r + 1], deltas[r:r + 1], props[r:r + 1], Hr, Wr, Hr, Wr, score_thr=-1.0, nms_thr=2.0, det_max=C - 1)
        assert len(o["labels"]) == C - 1 and sorted(o["labels"].tolist()) == list(range(1, C))
        prob[r] = o["scores_cls"][0]
        cbox[r, o["labels"] - 1] = o["boxes"]
    return prob, cbox


def nms_margins(boxes, scores, c, thr, max_keep):
    """Greedy NMS on boxes + c * (max + 1) in float32, order (score desc, index asc): (keep, the smallest |IoU - thr| over every pair the
    greedy pass compares).  The IoU expression is torchvision's: inter / ((area_i + area_j) - inter)."""
    b = np.ascontiguousarray(boxes, F32)
    n = b.shape[0]
    off = F32(c) * F32(b.max() + F32(1.0))
    b = (b + off).astype(F32)
    order = np.array(sorted(range(n), key=lambda i: (-float(scores[i]), i)), np.int64)
    b = b[order]
    area = ((b[:, 2] - b[:, 0]).astype(F32) * (b[:, 3] - b[:, 1]).astype(F32)).astype(F32)
    dead = np.zeros(n, bool)
    keep, margin = [], np.inf
    for i in range(n):
        if dead[i]:
            continue
        keep.append(int(order[i]))
        if len(keep) >= max_keep:
            break
        rest = np.nonzero(~dead[i + 1:])[0] + i + 1
        if rest.size == 0:
            continue
        w = np.maximum(F32(0), (np.minimum(b[i, 2], b[rest, 2]) - np.maximum(b[i, 0], b[rest, 0])).astype(F32))
        h = np.maximum(F32(0), (np.minimum(b[i, 3], b[rest, 3]) - np.maximum(b[i, 1], b[rest, 1])).astype(F32))
        inter = (w * h).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = (inter / ((area[i] + area[rest]).astype(F32) - inter).astype(F32)).astype(F32)
        fin = np.isfinite(iou)
        if fin.any():
            margin = min(margin, float(np.abs(iou[fin].astype(np.float64) - float(F32(thr))).min()))
        dead[rest[iou > F32(thr)]] = True
    return keep, margin


def ssm_tail(orc, logits, deltas, props, Hr, Wr, Ho, Wo, score_thr=0.05, det_max=100, nms_thr=0.3, conf=0.5, margins=None):
    """dict(al, boxes [n][4], scores [n][C-1], labels [n][C-1] int8, prop [n], cls [n]); margins (a dict) receives the smallest distances
    of the NMS, score-cut and 0.5 decisions from their thresholds."""
    logits = np.ascontiguousarray(logits, F32)
    R, C = logits.shape
    K = C - 1
    empty = dict(al=1, boxes=np.zeros((0, 4), F32), scores=np.zeros((0, K), F32), labels=np.zeros((0, K), np.int8),
                 prop=np.zeros(0, np.int64), cls=np.zeros(0, np.int64))
    if R == 0:                                   # the reference raises on torch.max of an empty tensor; the library answers al = 1
        return empty
    prob, cbox = rows(orc, logits, deltas, props, Hr, Wr)
    if margins is not None:
        margins["thr"] = float(np.abs(prob[:, 1:].astype(np.float64) - float(F32(score_thr))).min())
        margins["half"] = float(np.abs(prob[:, 1:].astype(np.float64) - 0.5).min())
        margins["iou"] = np.inf
    if prob[:, 1:].max() < F32(conf):
        return empty
    prop, cls = [], []
    for c in range(1, C):
        keep = orc.batched_nms(cbox[:, c - 1], prob[:, c], np.full(R, c, np.int32), nms_thr, det_max)
        if margins is not None:
            k2, m = nms_margins(cbox[:, c - 1], prob[:, c], c, nms_thr, det_max)
            assert k2 == keep.tolist(), "the margin pass and the oracle's NMS disagree on class %d" % c
            margins["iou"] = min(margins["iou"], m)
        for k in keep:
            if prob[k, c] > F32(score_thr):
                prop.append(int(k)); cls.append(c)
    prop = np.array(prop, np.int64); cls = np.array(cls, np.int64)
    boxes = orc.resize_boxes(cbox[prop, cls - 1], Hr, Wr, Ho, Wo) if len(prop) else np.zeros((0, 4), F32)
    scores = prob[prop, 1:].reshape(-1, K)
    return dict(al=0, boxes=boxes, scores=scores, labels=np.where(scores > F32(conf), 1, -1).astype(np.int8), prop=prop, cls=cls)


def integer_case(R, C, Hr, Wr, boxes, cls_logit, background=0.0):
    """Inputs whose decoded boxes ARE `boxes` (integers inside the image: zero deltas decode a proposal to itself, centre + half the size
    being exact for integers) and whose logits are `cls_logit` [R][C-1] beside a background logit."""
    logits = np.full((R, C), background, F32)
    logits[:, 1:] = cls_logit
    return logits, np.zeros((R, 4 * C), F32), np.ascontiguousarray(boxes, F32).reshape(R, 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# image_cross_validation: scripted scenes.  The candidate's image is (250, 255, 240) everywhere; labeled image k is (10, k + 1, 30), so a
# scripted model finds the pasted patch (channel 0 == 250) and the image's identity (the smallest value of channel 1) in what it is given.
# ---------------------------------------------------------------------------------------------------------------------------------
PATCH_RGB = (250, 255, 240)


def labeled_image(k, H, W):
    img = np.empty((H, W, 3), np.uint8)
    img[..., 0] = 10; img[..., 1] = k + 1; img[..., 2] = 30
    return img


def curr_image(H, W):
    img = np.empty((H, W, 3), np.uint8)
    img[...] = PATCH_RGB
    return img


# per scene: the candidate image's size, pre_box, pre_cls, the labeled images (H, W, labels) in loader order, and per labeled image what
# the scripted detector answers for class pre_cls: None (no detection of the class), or (score, "hit" | "miss") -- "hit" answers the
# pasted rectangle itself, "miss" a box in the far corner; every answer also carries a detection of another class.
SCENES = [
    dict(name="five_straight", seed=11, curr_hw=(40, 50), pre_box=[4.7, 6.2, 20.9, 30.1], pre_cls=3,
         labeled=[(60, 80, [1, 2]), (64, 64, [5]), (48, 90, [7, 8]), (70, 70, [2]), (55, 66, [9]), (80, 80, [1]), (90, 90, [4])],
         answers=[(0.9, "hit"), (0.8, "hit"), (0.7, "hit"), (0.95, "hit"), (0.6, "hit"), (0.9, "hit"), (0.9, "hit")]),
    dict(name="rounds_5_2_1", seed=12, curr_hw=(40, 50), pre_box=[0.0, 0.0, 10.0, 12.0], pre_cls=2,
         labeled=[(30, 30, [1]), (30, 40, [2, 4]), (32, 32, [3]), (9, 40, [1]), (36, 36, [5]), (40, 11, [6]), (33, 33, [7]), (34, 34, [8]),
                  (35, 35, [2]), (36, 37, [9]), (37, 38, [1]), (38, 39, [3]), (39, 40, [4]), (41, 41, [5])],
         answers=[(0.9, "hit"), None, None, None, (0.4, "hit"), None, (0.9, "miss"), None,
                  None, (0.9, "hit"), None, (0.7, "hit"), (0.9, "hit"), (0.9, "hit")]),
    dict(name="loader_ends", seed=13, curr_hw=(20, 20), pre_box=[2.0, 3.0, 9.0, 11.0], pre_cls=1,
         labeled=[(30, 30, [2]), (30, 30, [1]), (31, 31, [3]), (32, 32, [4])],
         answers=[(0.9, "hit"), None, None, (0.9, "hit")]),
    dict(name="empty_patch", seed=14, curr_hw=(20, 20), pre_box=[5.9, 3.0, 5.2, 11.0], pre_cls=1,
         labeled=[(30, 30, [2]), (30, 30, [3])], answers=[(0.9, "hit"), (0.9, "hit")]),
]


class ScriptedModel:
    """Answers by the scene's script.  Accepts what the reference hands a model ([float CHW tensor]) and what the library does (a list of
    uint8 HWC tensors); logs per call the identities of the images, and per image the pasted rectangle it found."""

    def __init__(self, scene, torch):
        self.scene, self.torch = scene, torch
        self.calls, self.pastes, self.modes = [], [], []

    def eval(self):
        return self

    def ssm_mode(self, flag):
        self.modes.append(bool(flag))

    def _hwc(self, img):
        t = img.detach().cpu()
        if t.dtype != self.torch.uint8:
            t = (t * 255.0).round().clamp(0, 255).to(self.torch.uint8)
        if t.shape[-1] != 3:
            t = t.permute(1, 2, 0)
        return t.numpy()

    def __call__(self, images):
        torch = self.torch
        ids, out = [], []
        for img in images:
            a = self._hwc(img)
            k = int(a[..., 1].min()) - 1
            ys, xs = np.nonzero(a[..., 0] == PATCH_RGB[0])
            rect = [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]
            inside = a[rect[1]:rect[3], rect[0]:rect[2]]
            assert (inside == np.array(PATCH_RGB, np.uint8)).all() and (a[..., 0] == PATCH_RGB[0]).sum() == inside.shape[0] * inside.shape[1]
            ids.append(k); self.pastes.append((k, rect))
            ans = self.scene["answers"][k]
            labels, boxes, scores = [self.scene["pre_cls"] + 1], [[0.0, 0.0, 5.0, 5.0]], [0.99]
            if ans is not None:
                labels += [self.scene["pre_cls"], self.scene["pre_cls"]]
                boxes += [[float(v) for v in rect] if ans[1] == "hit" else [0.0, 0.0, 1.0, 1.0], [1.0, 1.0, 3.0, 3.0]]
                scores += [ans[0], ans[0] / 2]
            out.append(dict(labels=torch.tensor(labels, dtype=torch.int64), boxes=torch.tensor(boxes, dtype=torch.float32),
                            scores=torch.tensor(scores, dtype=torch.float32)))
        self.calls.append(ids)
        return out


def scene_loaders(scene, torch, as_float):
    """(curr_loader, labeled_loader) as lists of (images, targets).  as_float: float32 CHW in [0, 1], what the reference's loader yields
    (to_tensor); else uint8 HWC."""
    def conv(a):
        t = torch.from_numpy(a)
        return t.permute(2, 0, 1).contiguous().to(torch.float32).div(255) if as_float else t
    curr = [([conv(curr_image(*scene["curr_hw"]))], [{}])]
    labeled = [([conv(labeled_image(k, H, W))], [{"labels": torch.tensor(lab, dtype=torch.int64)}]) for k, (H, W, lab) in enumerate(scene["labeled"])]
    return curr, labeled


def run_scene(fn, scene, torch, as_float):
    """fn = an image_cross_validation; returns (flag, score, model, the generator's state after)."""
    model = ScriptedModel(scene, torch)
    curr, labeled = scene_loaders(scene, torch, as_float)
    random.seed(scene["seed"])
    flag, score = fn(model, curr, labeled, scene["pre_box"], torch.tensor([scene["pre_cls"]]))
    return bool(flag), float(score), model, np.array(random.getstate()[1], np.int64)


def pair_iou(b2, off):
    """IoU in float32 of the two boxes b2 [2][4] shifted by `off`, torchvision's expression: what one NMS comparison evaluates."""
    b = (np.ascontiguousarray(b2, F32) + F32(off)).astype(F32)
    area = ((b[:, 2] - b[:, 0]).astype(F32) * (b[:, 3] - b[:, 1]).astype(F32)).astype(F32)
    w = max(F32(0), F32(min(b[0, 2], b[1, 2]) - max(b[0, 0], b[1, 0])))
    h = max(F32(0), F32(min(b[0, 3], b[1, 3]) - max(b[0, 1], b[1, 1])))
    inter = F32(w * h)
    return F32(inter / F32(F32(area[0] + area[1]) - inter))


def frcnn_tail_min(orc, logits, deltas, props, Hr, Wr, Ho, Wo, score_thr=0.05, nms_thr=0.5, det_max=100, min_size=1e-2):
    """torchvision's stock postprocess_detections + transform.postprocess: candidates (proposal, class) above the score threshold in
    (proposal, class) order, remove_small_boxes (both sides >= min_size), batched_nms over the rest -- its maximum coordinate is taken
    AFTER the removal --, the first det_max.  The outputs of cald_op_frcnn_postprocess."""
    logits = np.ascontiguousarray(logits, F32); props = np.ascontiguousarray(props, F32).reshape(-1, 4)
    R, C = logits.shape
    prob, cbox = rows(orc, logits, deltas, props, Hr, Wr)
    cand = [(r, c) for r in range(R) for c in range(1, C) if prob[r, c] > F32(score_thr)]
    cand = [(r, c) for r, c in cand if (cbox[r, c - 1, 2] - cbox[r, c - 1, 0]) >= F32(min_size) and (cbox[r, c - 1, 3] - cbox[r, c - 1, 1]) >= F32(min_size)]
    r = np.array([x[0] for x in cand], np.int64); c = np.array([x[1] for x in cand], np.int64)
    keep = orc.batched_nms(cbox[r, c - 1], prob[r, c], c.astype(np.int32), nms_thr, det_max) if len(cand) else np.zeros(0, np.int64)
    r, c = r[keep], c[keep]
    return dict(boxes=orc.resize_boxes(cbox[r, c - 1], Hr, Wr, Ho, Wo).reshape(-1, 4), scores=prob[r, c], labels=c,
                props=orc.resize_boxes(props[r], Hr, Wr, Ho, Wo).reshape(-1, 4), prob_max=prob[r, 1:].max(axis=1) if len(r) else np.zeros(0, F32),
                scores_cls=prob[r].reshape(-1, C))
