"""SSM (self-supervised sample mining) on the HIP detector: the pool sweep with the per-class NMS tail, and stage 2's host logic.

``fasterrcnn_resnet50_fpn_ssm(num_classes, min_size, max_size)``  -- detection/frcnn_ssm.py's factory: ``ssm_mode(flag)`` switches
    ``model([img])`` between the SSM result dict (``boxes`` [n, 4], ``scores`` [n, C-1], ``labels`` n lists of +-1, ``al``) and the stock
    torchvision tail (small boxes removed, ``box_min_size=1e-2``) that image_cross_validation reads.
``ssm_sweep_device_images(task_model, images)``                   -- the sweep over uint8 HWC images resident in HBM (cald_sweep_ssm)
``get_uncertainty(task_model, unlabeled_loader)``                 -- drop-in for ssm/ssm_helper.py:9-33
``judge_uv`` / ``calcu_iou`` / ``softmax``                        -- ssm_helper.py:36-54, :114-125, ssm_train.py:95-99
``image_cross_validation(model, curr_loader, labeled_sampler, pre_box, pre_cls)`` -- ssm_helper.py:58-111, its forwards batched
``ssm_select(...)``                                               -- the stage-2 loop of ssm_train.py:200-274 as one function

Faster R-CNN only: detection/retina_ssm.py sub-samples its candidates with ``random.shuffle`` inside the tail, which would tie a list
on the GPU to Python's global generator.  All detector arithmetic runs in libcaldhip.so; there is no CPU path.
"""
import ctypes as C
import random

import numpy as np
import torch

from . import _ffi
from .baselines import _arrays
from .detector import HipDetector
from .sweep import _to_u8_cuda

TOTAL_SELECT = 5          # ssm_helper.py:65: pasted images a candidate box is judged on
SWEEP_CHUNK = 64          # images whose worst-case rows the host buffers of the sweep hold


class HipDetectorSSM(HipDetector):
    """The library's Faster R-CNN with the two tails of detection/frcnn_ssm.py."""

    def __init__(self, num_classes, **kw):
        kw.setdefault("box_min_size", 1e-2)          # torchvision's stock postprocess_detections, which ssm_mode(False) selects
        super().__init__(num_classes, **kw)
        if self.arch != 0:
            raise NotImplementedError("the SSM tail covers Faster R-CNN only")
        self._ssm = False

    def ssm_mode(self, flag):
        self._ssm = bool(flag)

    def __call__(self, images, targets=None):
        if self.training or not self._ssm:
            return super().__call__(images, targets)
        dev = torch.device("cuda", self._device if self._device is not None else torch.cuda.current_device())
        u8 = [_to_u8_cuda(img, dev) for img in images]
        al, counts, boxes, scores, labels = ssm_sweep_device_images(self, u8, batch_images=len(u8))
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return [{"boxes": torch.from_numpy(boxes[off[i]:off[i + 1]]).to(dev), "scores": torch.from_numpy(scores[off[i]:off[i + 1]]).to(dev),
                 "labels": labels[off[i]:off[i + 1]].astype(np.int64).tolist(), "al": int(al[i])} for i in range(len(u8))]


def fasterrcnn_resnet50_fpn_ssm(pretrained=False, progress=True, num_classes=91, pretrained_backbone=True, **kwargs):
    """detection/frcnn_ssm.py's factory (call sites ssm_train.py:157, :162).  Weights arrive through load_state_dict()."""
    return HipDetectorSSM(num_classes, depth=50, **kwargs)


def ssm_sweep_device_images(task_model, images, batch_images=0):
    """The SSM pool pass over uint8 HWC CUDA tensors: (al [n] int32, counts [n] int32, boxes [rows, 4] float32, scores [rows, C-1]
    float32, labels [rows, C-1] int8), the rows of all images consecutively in image order.  An image with al == 1 has no rows.  The
    images go through cald_sweep_ssm in chunks of SWEEP_CHUNK, whose worst case ((C - 1) * detections_per_img rows an image) sizes the
    host buffers; a chunk's used rows are copied out before the next one runs."""
    K = task_model.num_classes - 1
    per_image = K * task_model.cfg.detections_per_img
    n = len(images)
    al = np.zeros(n, np.int32); counts = np.zeros(n, np.int32)
    parts = []
    handle = task_model.handle()
    cap = min(n, SWEEP_CHUNK) * per_image
    boxes = np.empty((cap, 4), np.float32); scores = np.empty((cap, K), np.float32); labels = np.empty((cap, K), np.int8)
    for i0 in range(0, n, SWEEP_CHUNK):
        chunk = images[i0:i0 + SWEEP_CHUNK]
        for im in chunk:
            assert im.dtype == torch.uint8 and im.is_cuda and im.is_contiguous() and im.dim() == 3 and im.shape[2] == 3
        ptrs, Hs, Ws = _arrays(chunk)
        need = C.c_int64(0)
        _ffi.check(_ffi.lib().cald_sweep_ssm(handle, len(chunk), ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i), int(batch_images),
                                             cap, _ffi.ptr(al[i0:], _ffi.c_i), _ffi.ptr(counts[i0:], _ffi.c_i), _ffi.ptr(boxes),
                                             _ffi.ptr(scores), _ffi.ptr(labels, _ffi.c_i8), C.byref(need)))
        r = int(need.value)
        parts.append((boxes[:r].copy(), scores[:r].copy(), labels[:r].copy()))
    if not parts:
        return al, counts, np.zeros((0, 4), np.float32), np.zeros((0, K), np.float32), np.zeros((0, K), np.int8)
    return (al, counts) + tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def get_uncertainty(task_model, unlabeled_loader, batch_images=0):
    """Drop-in for ssm_helper.py:9-33: (allScore, allBox, allY, al_idx).  allScore / allBox: one CUDA tensor [n, C-1] / [n, 4] per image
    with al == 0, in loader order; allY: per such image n lists of +-1; al_idx: the loader positions with al == 1.  One image per loader
    item, as the reference requires."""
    if not hasattr(task_model, "handle"):
        from .detector import from_torch_module
        task_model = from_torch_module(task_model)
    task_model.eval()
    if hasattr(task_model, "ssm_mode"):
        task_model.ssm_mode(True)
    dev = torch.device("cuda", torch.cuda.current_device())
    images = []
    for imgs, _ in unlabeled_loader:
        if len(imgs) != 1:
            raise ValueError("get_uncertainty supports batch_size=1 only (ssm_helper.py:20)")
        images.append(_to_u8_cuda(imgs[0], dev))
    al, counts, boxes, scores, labels = ssm_sweep_device_images(task_model, images, batch_images)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    allScore, allBox, allY, al_idx = [], [], [], []
    for i in range(len(images)):
        if al[i] == 1:
            al_idx.append(i)
            continue
        allBox.append(torch.from_numpy(boxes[off[i]:off[i + 1]]).to(dev))
        allScore.append(torch.from_numpy(scores[off[i]:off[i + 1]]).to(dev))
        allY.append(labels[off[i]:off[i + 1]].astype(np.int64).tolist())
    return allScore, allBox, allY, al_idx


# ---- host functions ----
def softmax(ary):
    e = np.exp(ary.flatten())
    return e / np.sum(e)


def judge_uv(loss, gamma, clslambda):
    """(u, v): u False when the summed loss exceeds gamma (v zeros); below gamma v[i] = 1 - loss[i] / clslambda[i], or 0 where loss[i] is
    above clslambda[i].  A sum equal to gamma -- or NaN -- is neither: (True, zeros), as in the reference."""
    total = np.sum(loss)
    v = np.zeros((loss.shape[0],))
    if total > gamma:
        return False, v
    if total < gamma:
        for i, l in enumerate(loss):
            v[i] = 0 if l > clslambda[i] else 1 - l / clslambda[i]
    return True, v


def calcu_iou(A, B):
    """ssm_helper.py:114-125 as it is: the intersection and the heights count pixels (+1), the widths of the areas do not."""
    w = min(A[2], B[2]) - max(A[0], B[0]) + 1
    h = min(A[3], B[3]) - max(A[1], B[1]) + 1
    if w <= 0 or h <= 0:
        return 0
    area_a = (A[2] - A[0]) * (A[3] - A[1] + 1)
    area_b = (B[2] - B[0]) * (B[3] - B[1] + 1)
    inter = w * h
    return inter / (area_a + area_b - inter)


def box_loss(score, label):
    """ssm_train.py:228-229: the per-class loss of one box in the reference's mixed arithmetic -- score float32 [K], label int64 [K] of
    +-1; the logs are float32, the label factors float64.  A score of 0 under a label of -1 gives 0 * -inf = NaN, as there."""
    score = np.asarray(score, np.float32); label = np.asarray(label, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -((1 + label) / 2 * np.log(score) + (1 - label) / 2 * np.log(1 - score + 1e-30))


@torch.no_grad()
def image_cross_validation(model, curr_loader, labeled_sampler, pre_box, pre_cls):
    """ssm_helper.py:58-111, same signature, returns (bool, score).  The candidate's patch is cropped [:, int(b0):int(b2), int(b1):int(b3)]
    -- x indexes rows, as in the reference -- and pasted at a random place into labeled images that do not hold class pre_cls and are
    large enough; for each such image start_y, then start_x, is drawn with random.randint.  The paste is a slice assignment on a copy of
    the uint8 image; the loader's tensor is not written.

    Batching.  The reference runs one forward per pasted image and stops once five of them held a detection of the class.  Here a round
    collects 5 - curr_select eligible images, runs them as ONE forward and consumes the results in order.  A round can raise curr_select
    by at most its own size, so the count reaches five, if at all, on the round's LAST image: no image is pasted, and no random number
    drawn, that the reference would not have reached.  Rounds repeat until five images counted or the loader ends."""
    model.eval()
    model.ssm_mode(False)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    for images, _ in curr_loader:
        curr = _to_u8_cuda(images[0], dev)
    patch = curr[int(pre_box[0]):int(pre_box[2]), int(pre_box[1]):int(pre_box[3]), :]
    ph, pw = patch.shape[0], patch.shape[1]
    if ph <= 0 or pw <= 0:
        return False, 0
    cls = int(pre_cls)
    curr_select, cross_validation, avg_score = 0, 0, 0
    it = iter(labeled_sampler)
    ended = False
    while curr_select < TOTAL_SELECT and not ended:
        pasted, origin = [], []
        while len(pasted) < TOTAL_SELECT - curr_select:
            try:
                images, targets = next(it)
            except StopIteration:
                ended = True
                break
            labeled_cls = targets[0]["labels"]
            labeled_cls = labeled_cls.cpu().numpy() if hasattr(labeled_cls, "cpu") else np.asarray(labeled_cls)
            if cls in labeled_cls:
                continue
            img = _to_u8_cuda(images[0], dev)
            if ph > img.shape[0] or pw > img.shape[1]:
                continue
            start_y = random.randint(0, img.shape[0] - ph)
            start_x = random.randint(0, img.shape[1] - pw)
            canvas = img.clone()
            canvas[start_y:start_y + ph, start_x:start_x + pw, :] = patch
            pasted.append(canvas); origin.append([start_x, start_y, start_x + pw, start_y + ph])
        if not pasted:
            break
        for det, original_box in zip(model(pasted), origin):
            same = det["labels"] == cls
            boxes, scores = det["boxes"][same], det["scores"][same]
            if len(boxes) == 0:
                continue
            index = torch.argmax(scores)
            score, box = scores[index], boxes[index]
            curr_select += 1
            if score > 0.5 and calcu_iou(original_box, box) > 0.5:
                cross_validation += 1
                avg_score += score
    if cross_validation > TOTAL_SELECT / 2:
        return True, avg_score / cross_validation
    return False, 0


def ssm_select(task_model, dataset_loader_factory, subset, labeled_set, allScore, allBox, allY, al_idx, budget_num, gamma, clslambda):
    """Stage 2 of an SSM cycle (ssm_train.py:200-274): returns (al_idx, gamma, clslambda) -- the pool indices to label and the updated
    pace parameters.  subset: the pool indices get_uncertainty swept, in its order; al_idx: those it flagged, as pool indices
    (ssm_train.py:198); labeled_set is read only (the caller extends it).  dataset_loader_factory(indices, shuffle) returns a batch-size-1
    loader over those dataset indices, in order (shuffle False: the candidate's own image) or in random order (True: the labeled set).

    As in the reference: `subset` loses the flagged images BEFORE the loop, while allBox / allScore / allY keep get_uncertainty's
    positions; the class handed to the cross-validation is the index into the C - 1 score vector (one less than the label), and a box
    whose only +1 sits at index 0 is skipped by the `!= 0` test; sharding over ranks does not apply -- the loop is sequential."""
    K = len(clslambda)
    al_idx = list(al_idx)
    cls_sum = 0
    cls_loss_sum = np.zeros((K,))

    def pace():
        with np.errstate(divide="ignore", invalid="ignore"):
            return 0.9 * clslambda - 0.1 * np.log(softmax(cls_loss_sum / (cls_sum + 1e-30))), min(gamma + 0.05, 1)

    if len(al_idx) >= budget_num:
        lam, gam = pace()
        return al_idx[:budget_num], gam, lam
    subset = list(set(subset) - set(al_idx))
    for i in range(len(subset)):
        if len(al_idx) >= budget_num:
            break
        cls_sum += len(allBox[i])
        for j, box in enumerate(allBox[i]):
            if len(al_idx) >= budget_num:
                break
            score = allScore[i][j]
            score = score.cpu().numpy() if hasattr(score, "cpu") else np.asarray(score, np.float32)
            label = np.asarray(allY[i][j], np.int64)
            loss = box_loss(score, label)
            cls_loss_sum += loss
            v, _ = judge_uv(loss, gamma, clslambda)
            if not v:
                al_idx.append(subset[i])
                break
            ones = np.nonzero(label == 1)[0]
            if not (len(ones) == 1 and ones[0] != 0):
                continue
            ok, _ = image_cross_validation(task_model, dataset_loader_factory([subset[i]], False), dataset_loader_factory(labeled_set, True),
                                           box, int(ones[0]))
            if not ok:
                al_idx.append(subset[i])
                break
    subset = list(set(subset) - set(al_idx))
    if len(al_idx) > budget_num:
        al_idx = al_idx[:budget_num]
    if len(al_idx) < budget_num:
        al_idx += list(set(subset) - set(al_idx))[:budget_num - len(al_idx)]
    lam, gam = pace()
    return al_idx, gam, lam
