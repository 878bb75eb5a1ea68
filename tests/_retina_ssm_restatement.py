"""An independent statement of the RetinaNet SSM tail (detection/retina_ssm.py:487-584 + transform.postprocess) in numpy float32, for
tests/test_retina_ssm.py, tests/test_gpu_retina_ssm.py and tools/make_golden_retina_ssm.py.

``tail(scores, boxes, picks, ...)`` takes the sigmoid scores [N][K] and the decoded, clipped boxes [N][4] of all N anchors in anchor order
(level P3..P7, pixel row-major, anchor) plus the picks -- per class the positions into the class's candidate list, in shuffled order, or a
callable ``pick(k, n)`` that draws them (``shuffle_pick`` is the reference's own lines) -- and returns the rows and the margins the
decisions met.  ``scores_of`` / ``grid_anchors`` / ``decode`` make those inputs from logits, deltas and base anchors; the exponential is
an argument, so a caller can pass the oracle's (the library's bits) or numpy's.

What is stated here is the bookkeeping of the tail: the al flag over ALL K classes, `>` at the score threshold, the cut at 500 BEFORE
the small boxes leave, NMS order (score desc, then the earlier pick), the first per_class survivors, the labels over classes 1..K-1.
``mutate`` switches exactly one of those statements to a plausible wrong one; tests/test_retina_ssm.py asserts that the fixture tells
each of them apart.
"""
import random

import numpy as np

F32 = np.float32
TAKE = 500
BBOX_XFORM_CLIP = F32(np.log(1000.0 / 16.0))
MUTATIONS = ("ge_threshold", "al_over_foreground", "labels_over_all", "small_before_cut")


def scores_of(logits, exp=np.exp):
    """sigmoid in float32 as the library states it: 1 / (1 + exp(-x))."""
    x = np.ascontiguousarray(logits, F32)
    e = np.asarray(exp((-x).astype(F32).reshape(-1)), F32).reshape(x.shape)
    return (F32(1.0) / (F32(1.0) + e).astype(F32)).astype(F32)


def grid_anchors(base, level_hw, Hp, Wp):
    """[N][4]: base [5][A][4] shifted to every pixel of the five levels; strides Hp // H_l, Wp // W_l; anchor order."""
    out = []
    for l, (h, w) in enumerate(level_hw):
        sh, sw = Hp // h, Wp // w
        ys, xs = np.meshgrid(np.arange(h) * sh, np.arange(w) * sw, indexing="ij")
        shifts = np.stack([xs, ys, xs, ys], -1).reshape(-1, 1, 4).astype(F32)
        out.append((shifts + np.asarray(base[l], F32)[None]).reshape(-1, 4))
    return np.concatenate(out).astype(F32)


def decode(deltas, anchors, Hr, Wr, exp=np.exp):
    """BoxCoder(1, 1, 1, 1).decode_single + clip_boxes_to_image in float32, operation by operation."""
    d = np.ascontiguousarray(deltas, F32).reshape(-1, 4); a = np.ascontiguousarray(anchors, F32).reshape(-1, 4)
    w = (a[:, 2] - a[:, 0]).astype(F32); h = (a[:, 3] - a[:, 1]).astype(F32)
    cx = (a[:, 0] + (F32(0.5) * w).astype(F32)).astype(F32); cy = (a[:, 1] + (F32(0.5) * h).astype(F32)).astype(F32)
    dw = np.minimum(d[:, 2], BBOX_XFORM_CLIP); dh = np.minimum(d[:, 3], BBOX_XFORM_CLIP)
    pcx = ((d[:, 0] * w).astype(F32) + cx).astype(F32); pcy = ((d[:, 1] * h).astype(F32) + cy).astype(F32)
    pw = (np.asarray(exp(dw), F32) * w).astype(F32); ph = (np.asarray(exp(dh), F32) * h).astype(F32)
    hw_, hh_ = (F32(0.5) * pw).astype(F32), (F32(0.5) * ph).astype(F32)
    b = np.stack([pcx - hw_, pcy - hh_, pcx + hw_, pcy + hh_], 1).astype(F32)
    b[:, 0::2] = np.clip(b[:, 0::2], F32(0), F32(Wr)); b[:, 1::2] = np.clip(b[:, 1::2], F32(0), F32(Hr))
    return b


def shuffle_pick(k, n):
    """retina_ssm.py:540-542 on Python's global generator."""
    keep = [i for i in range(n)]
    random.shuffle(keep)
    return keep[:TAKE]


def nms_margins(boxes, scores, thr, max_keep):
    """Greedy NMS in float32 over boxes in LIST order with ties going to the earlier entry: (keep, the smallest |IoU - thr| over every
    pair the greedy pass compares).  torchvision's IoU: inter / ((area_i + area_j) - inter)."""
    b = np.ascontiguousarray(boxes, F32).reshape(-1, 4)
    n = b.shape[0]
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


def _away(values, thr):
    """Smallest distance of `values` from `thr`, the values EQUAL to it left out (an exact tie is a case's design, and exact in any
    arithmetic; a near miss would hang on a rounding)."""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[v != float(F32(thr))]
    return float(np.abs(v - float(F32(thr))).min()) if v.size else np.inf


def tail(scores, boxes, picks, Hr, Wr, Ho, Wo, score_thr=0.05, nms_thr=0.5, per_class=50, conf=0.5, min_box=1e-2, mutate=None):
    """dict(al, counts [K], picks (per class, as used), boxes [n][4], scores [n], labels [n][K-1] int8, cls [n], anchor [n], margins)."""
    assert mutate is None or mutate in MUTATIONS
    s = np.ascontiguousarray(scores, F32); b = np.ascontiguousarray(boxes, F32).reshape(-1, 4)
    N, K = s.shape
    L = K if mutate == "labels_over_all" else K - 1
    margins = dict(thr=_away(s, score_thr), half=_away(s, conf), iou=np.inf)
    out = dict(al=0, counts=np.zeros(K, np.int64), picks=[np.zeros(0, np.int64)] * K, boxes=np.zeros((0, 4), F32), scores=np.zeros(0, F32),
               labels=np.zeros((0, L), np.int8), cls=np.zeros(0, np.int64), anchor=np.zeros(0, np.int64), margins=margins)
    top = s[:, 1:].max() if mutate == "al_over_foreground" else s.max()
    if top < F32(conf):
        out["al"] = 1
        return out
    rows_anchor, rows_cls, used = [], [], []
    for k in range(K):
        cand = np.nonzero(s[:, k] >= F32(score_thr) if mutate == "ge_threshold" else s[:, k] > F32(score_thr))[0]
        if mutate == "small_before_cut":
            cand = cand[((b[cand, 2] - b[cand, 0]) >= F32(min_box)) & ((b[cand, 3] - b[cand, 1]) >= F32(min_box))]
        out["counts"][k] = cand.size
        keep = np.asarray(picks(k, int(cand.size)) if callable(picks) else picks[k], np.int64).reshape(-1)
        assert keep.size <= min(cand.size, TAKE) and (keep.size == 0 or (keep.min() >= 0 and keep.max() < cand.size)), (k, keep.size, cand.size)
        used.append(keep)
        sel = cand[keep]                                              # the picked anchors, in shuffled order
        big = ((b[sel, 2] - b[sel, 0]) >= F32(min_box)) & ((b[sel, 3] - b[sel, 1]) >= F32(min_box))
        sel = sel[big]                                                # a small box has used up its pick
        kept, m = nms_margins(b[sel], s[sel, k], nms_thr, per_class)
        margins["iou"] = min(margins["iou"], m)
        rows_anchor += [int(sel[i]) for i in kept]; rows_cls += [k] * len(kept)
    anchor = np.array(rows_anchor, np.int64); cls = np.array(rows_cls, np.int64)
    rh, rw = F32(Ho) / F32(Hr), F32(Wo) / F32(Wr)                     # stock resize_boxes: float32 ratios
    bx = (b[anchor] * np.array([rw, rh, rw, rh], F32)).astype(F32)
    lab_src = s[anchor] if mutate == "labels_over_all" else s[anchor, 1:]
    out.update(picks=used, boxes=bx.reshape(-1, 4), scores=s[anchor, cls].astype(F32), labels=np.where(lab_src > F32(conf), 1, -1).astype(np.int8).reshape(-1, L),
               cls=cls, anchor=anchor)
    return out


def pack_picks(picks, K):
    """per-class pick lists -> (picks [K][TAKE] int32 padded with -1, n_picks [K] int32): the arrays of cald_ssm_pick_fn / the fixture."""
    arr = np.full((K, TAKE), -1, np.int32); n = np.zeros(K, np.int32)
    for k in range(K):
        p = np.asarray(picks[k], np.int32).reshape(-1)
        arr[k, :p.size] = p; n[k] = p.size
    return arr, n


def unpack_picks(arr, n):
    return [np.asarray(arr[k, :int(n[k])], np.int64) for k in range(len(n))]
