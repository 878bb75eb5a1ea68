"""SSM (self-supervised sample mining) on the HIP detectors: the pool sweep with the per-class NMS tail, and stage 2's host logic.

``fasterrcnn_resnet50_fpn_ssm(num_classes, min_size, max_size)``  -- detection/frcnn_ssm.py's factory: ``ssm_mode(flag)`` switches
    ``model([img])`` between the SSM result dict (``boxes`` [n, 4], ``scores`` [n, C-1], ``labels`` n lists of +-1, ``al``) and the stock
    torchvision tail (small boxes removed, ``box_min_size=1e-2``) that image_cross_validation reads.
``retinanet_resnet50_fpn_ssm(num_classes, min_size, max_size)``   -- detection/retina_ssm.py's factory (50 detections per class): in SSM mode
    ``scores`` is 1-D [n] (the score of the row's class) and ``labels`` holds n lists of K - 1 entries (classes 1..K-1);
    ``ssm_mode(False)`` gives the stock RetinaNet tail.
``ssm_sweep_device_images(task_model, images)``                   -- the sweep over uint8 HWC images resident in HBM (cald_sweep_ssm /
    cald_sweep_ssm_retina, by ``task_model.arch``)
``get_uncertainty(task_model, unlabeled_loader)``                 -- drop-in for ssm/ssm_helper.py:9-33
``judge_uv`` / ``calcu_iou`` / ``softmax``                        -- ssm_helper.py:36-54, :114-125, ssm_train.py:95-99
``image_cross_validation(model, curr_loader, labeled_sampler, pre_box, pre_cls)`` -- ssm_helper.py:58-111, its forwards batched
``ssm_select(...)``                                               -- the stage-2 loop of ssm_train.py:200-274 as one function

RetinaNet.  detection/retina_ssm.py:540-542 sub-samples every class's candidates with ``random.shuffle`` on Python's global generator, in
the middle of the tail.  The tail therefore runs as two device phases around one host stop (retina_ssm.hip): the
device counts and lists the candidates, the host draws ``keep = list(range(n)); random.shuffle(keep); keep[:500]`` per class exactly as
the reference would, the device finishes.  The draw is either a ctypes callback on the ``random`` module (``_python_pick``, the plain
statement) or the library's ``cald_ssm_pick_mt19937`` on a copy of ``random.getstate()`` that is put back, advanced, afterwards -- the
same numbers without the interpreter's time per candidate; it is used once a self-check against ``random.shuffle`` has passed, and
``CALD_SSM_PICK=python`` selects the callback.  Either way a seeded run leaves the generator where the reference leaves it, so the
``random.randint`` draws of image_cross_validation land where they would there.  Every image of a batch gets its own rows: the
reference's accumulators are not reset between the images of a batch (image i's dict would repeat the rows of the images before it),
which is not reproduced -- its sweep runs batch 1 (ssm_helper.py:20), where the two agree.

All detector arithmetic runs in libcaldhip.so; there is no CPU path.
"""
import ctypes as C
import os
import random

import numpy as np
import torch

from . import _ffi
from .baselines import _arrays
from .detector import HipDetector
from .sweep import _to_u8_cuda

TOTAL_SELECT = 5          # ssm_helper.py:65: pasted images a candidate box is judged on
SWEEP_CHUNK = 64          # images whose worst-case rows the host buffers of the sweep hold
TAKE = _ffi.SSM_RETINA_TAKE   # retina_ssm.py:542: candidates of a class that survive the shuffle


class HipDetectorSSM(HipDetector):
    """The library's Faster R-CNN (arch=0) or RetinaNet (arch=1) with the two tails of detection/frcnn_ssm.py / detection/retina_ssm.py.  In
    SSM mode every image of ``model(images)`` gets its own rows (the reference's RetinaNet tail would repeat earlier images' rows)."""

    def __init__(self, num_classes, **kw):
        if kw.get("arch", 0) == 0:
            kw.setdefault("box_min_size", 1e-2)      # torchvision's stock postprocess_detections, which ssm_mode(False) selects
        super().__init__(num_classes, **kw)
        if self.arch == 1 and num_classes < 2:
            raise ValueError("the RetinaNet SSM tail needs at least two classes (labels have K - 1 columns)")
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


def retinanet_resnet50_fpn_ssm(pretrained=False, progress=True, num_classes=91, pretrained_backbone=True,
                               score_thresh=0.05, nms_thresh=0.5, detections_per_img=50, **kwargs):
    """detection/retina_ssm.py's factory (call sites ssm_train.py:158-164; constructor defaults retina_ssm.py:331-342: 50 detections per
    class).  Weights arrive through load_state_dict()."""
    return HipDetectorSSM(num_classes, depth=50, box_score_thresh=score_thresh, box_nms_thresh=nms_thresh,
                          box_detections_per_img=detections_per_img, arch=1, **kwargs)


# ---- the host stop of the RetinaNet tail: which candidates of a class survive (retina_ssm.py:540-542) ----
def _shuffle_picks(rng, K, counts, picks, n_picks):
    """Per class `keep = list(range(n)); rng.shuffle(keep); keep[:TAKE]` into the callback's arrays (cald_ssm_pick_fn)."""
    out = np.ctypeslib.as_array(picks, shape=(K * TAKE,))
    for k in range(K):
        keep = list(range(counts[k]))
        rng.shuffle(keep)
        keep = keep[:TAKE]
        out[k * TAKE:k * TAKE + len(keep)] = keep
        n_picks[k] = len(keep)


@_ffi.PICK_FN
def _python_pick(user, image, K, counts, picks, n_picks):
    """The plain statement: the reference's lines on the global `random` module.  An exception becomes a non-zero return (the library then
    ends the sweep with CALD_ERR_INVALID); ctypes would otherwise print it and return 0 with the picks half written."""
    try:
        _shuffle_picks(random, K, counts, picks, n_picks)
        return 0
    except BaseException:
        return 1


def _c_pick(state, counts):
    """cald_ssm_pick_mt19937 on `state` (uint32 [625], advanced in place): (picks [K][TAKE] int32, n_picks [K] int32)."""
    counts = np.ascontiguousarray(counts, np.int32)
    K = len(counts)
    picks = np.zeros((K, TAKE), np.int32); n_picks = np.zeros(K, np.int32)
    rc = _ffi.lib().cald_ssm_pick_mt19937(state.ctypes.data, 0, K, _ffi.ptr(counts, _ffi.c_i), _ffi.ptr(picks, _ffi.c_i), _ffi.ptr(n_picks, _ffi.c_i))
    if rc:
        raise RuntimeError("cald_ssm_pick_mt19937 returned %d" % rc)
    return picks, n_picks


_C_PICK_OK = None


def _c_pick_checked():
    """True once cald_ssm_pick_mt19937 has reproduced random.shuffle -- picks and end state -- on a few class lists from a private
    generator (the global one is not touched), with a state regeneration inside a shuffle.  Checked at first use."""
    global _C_PICK_OK
    if _C_PICK_OK is None:
        ok = True
        for seed, counts in ((20, [0, 1, 2, 3, 257]), (21, [501, 0, 1500, 7])):
            rng = random.Random(seed)
            ver, words, gauss = rng.getstate()
            state = np.array(words, np.uint32)
            try:
                picks, n_picks = _c_pick(state, counts)
            except (RuntimeError, AttributeError):
                ok = False
                break
            for k, n in enumerate(counts):
                keep = list(range(n)); rng.shuffle(keep); keep = keep[:TAKE]
                ok = ok and n_picks[k] == len(keep) and picks[k, :len(keep)].tolist() == keep
            ok = ok and tuple(int(x) for x in state) == rng.getstate()[1]
        _C_PICK_OK = bool(ok)
    return _C_PICK_OK


def _with_pick(run):
    """Calls run(pick, user) -- the two arguments of cald_sweep_ssm_retina / cald_op_retina_ssm_postprocess -- with the draw on Python's global
    generator: the C pick on a copy of random.getstate(), written back advanced (version and gauss_next kept) whether or not `run`
    raises, or the Python callback under CALD_SSM_PICK=python or a failed self-check."""
    if os.environ.get("CALD_SSM_PICK", "") == "python" or not _c_pick_checked():
        return run(C.cast(_python_pick, C.c_void_p), None)
    ver, words, gauss = random.getstate()
    state = np.array(words, np.uint32)
    try:
        return run(C.cast(_ffi.lib().cald_ssm_pick_mt19937, C.c_void_p), C.c_void_p(state.ctypes.data))
    finally:
        random.setstate((ver, tuple(int(x) for x in state), gauss))


def ssm_sweep_device_images(task_model, images, batch_images=0):
    """The SSM pool pass over uint8 HWC CUDA tensors: (al [n] int32, counts [n] int32, boxes [rows, 4] float32, scores, labels int8), the
    rows of all images consecutively in image order.  Faster R-CNN: scores / labels [rows, C-1]; RetinaNet: scores [rows], labels
    [rows, K-1].  An image with al == 1 has no rows.  The images go through cald_sweep_ssm / cald_sweep_ssm_retina in chunks of
    SWEEP_CHUNK, whose worst case ((C - 1) or K times detections_per_img rows an image) sizes the host buffers; a chunk's used rows are
    copied out before the next one runs.  RetinaNet: the per-class picks are drawn from Python's global `random` (_with_pick), for the
    images with al == 0 in image order."""
    retina = task_model.arch == 1
    K = task_model.num_classes - 1                   # label columns
    per_image = (K + 1 if retina else K) * task_model.cfg.detections_per_img
    sshape = () if retina else (K,)
    n = len(images)
    al = np.zeros(n, np.int32); counts = np.zeros(n, np.int32)
    parts = []
    handle = task_model.handle()
    cap = min(n, SWEEP_CHUNK) * per_image
    boxes = np.empty((cap, 4), np.float32); scores = np.empty((cap,) + sshape, np.float32); labels = np.empty((cap, K), np.int8)

    def run(pick, user):
        for i0 in range(0, n, SWEEP_CHUNK):
            chunk = images[i0:i0 + SWEEP_CHUNK]
            for im in chunk:
                assert im.dtype == torch.uint8 and im.is_cuda and im.is_contiguous() and im.dim() == 3 and im.shape[2] == 3
            ptrs, Hs, Ws = _arrays(chunk)
            need = C.c_int64(0)
            head = (handle, len(chunk), ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i), int(batch_images))
            tail = (cap, _ffi.ptr(al[i0:], _ffi.c_i), _ffi.ptr(counts[i0:], _ffi.c_i), _ffi.ptr(boxes), _ffi.ptr(scores), _ffi.ptr(labels, _ffi.c_i8),
                    C.byref(need))
            if retina:
                _ffi.check(_ffi.lib().cald_sweep_ssm_retina(*(head + (pick, user) + tail)))
            else:
                _ffi.check(_ffi.lib().cald_sweep_ssm(*(head + tail)))
            r = int(need.value)
            parts.append((boxes[:r].copy(), scores[:r].copy(), labels[:r].copy()))

    if retina:
        _with_pick(run)
    else:
        run(None, None)
    if not parts:
        return al, counts, np.zeros((0, 4), np.float32), np.zeros((0,) + sshape, np.float32), np.zeros((0, K), np.int8)
    return (al, counts) + tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def get_uncertainty(task_model, unlabeled_loader, batch_images=0):
    """Drop-in for ssm_helper.py:9-33: (allScore, allBox, allY, al_idx).  allScore / allBox: one CUDA tensor [n, C-1] (RetinaNet: [n], the
    score of the row's class) / [n, 4] per image with al == 0, in loader order; allY: per such image n lists of +-1 (C - 1 entries;
    RetinaNet: K - 1); al_idx: the loader positions with al == 1.  One image per loader item, as the reference requires."""
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
    """ssm_train.py:228-229: the per-class loss of one box in the reference's mixed arithmetic -- score float32 [K] (RetinaNet: a float32
    scalar, which broadcasts against the K labels as it does there), label int64 [K] of +-1; the logs are float32, the label factors float64.  A score of 0 under a label of -1 gives 0 * -inf = NaN, as there."""
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
