"""Plain numpy float64 restatement of the DECISIONS of the detection tail, for tests/test_gpu_tail_edges.py.

Only the discrete steps are restated, from their published definitions, sharing no code with the product or the oracle:

  - stable top-k by (score desc, index asc);
  - clip_boxes_to_image, remove_small_boxes (both sides >= min_size);
  - greedy NMS with a strict `>` (torchvision nms) and batched_nms' separation of groups;
  - the first-n cut of the kept list;
  - RetinaNet's per-class loop and class-order concatenation;
  - the scoring loop's IoU argmax with the first index winning ties.

Everything returns indices.  The tests feed integer boxes whose areas stay below 2^24: intersection, union and the comparison
IoU > num / den are then evaluated exactly here (integers in float64, compared as inter * den > union * num), and the float32 side
computes the correctly rounded quotient of the same two integers.  Every NMS also reports the smallest non-zero |IoU - thr| it met,
every argmax the smallest non-zero gap between the best and the second best IoU: the tests assert that these margins are far above a
float32 rounding error, so that no decision depends on the precision it is taken in.
"""
import numpy as np

THR = {0.5: (1, 2), 0.7: (7, 10)}      # the thresholds as rationals


def stable_order(scores):
    """indices by (score desc, index asc)"""
    scores = np.asarray(scores, np.float64)
    return np.lexsort((np.arange(scores.size), -scores))


def grid_anchors(base, H, W, sth, stw):
    """AnchorGenerator for one level: anchor i = (y * W + x) * A + a = base[a] shifted by (x * stw, y * sth).  [H * W * A, 4] float64."""
    base = np.asarray(base, np.float64).reshape(-1, 4)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64) * sth, np.arange(W, dtype=np.float64) * stw, indexing="ij")
    shift = np.stack([xs, ys, xs, ys], -1).reshape(-1, 1, 4)
    return (shift + base[None]).reshape(-1, 4)


def clip(boxes, Hr, Wr):
    b = np.array(boxes, np.float64).reshape(-1, 4)
    b[:, 0::2] = np.clip(b[:, 0::2], 0.0, float(Wr))
    b[:, 1::2] = np.clip(b[:, 1::2], 0.0, float(Hr))
    return b


def not_small(boxes, min_size):
    return ((boxes[:, 2] - boxes[:, 0]) >= min_size) & ((boxes[:, 3] - boxes[:, 1]) >= min_size)


def _inter_union(a, b):
    w = np.maximum(0.0, np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    h = np.maximum(0.0, np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = w * h
    return inter, (a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter


def nms(boxes, thr, max_keep=None):
    """Greedy NMS over boxes in score order: keep i, drop every later j with IoU(i, j) > thr; stop after max_keep.
    Returns (kept positions, smallest non-zero |IoU - thr| over the pairs (kept box, later box still alive))."""
    num, den = THR[thr]
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = boxes.shape[0]
    dead = np.zeros(n, bool)
    keep, margin = [], np.inf
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        if max_keep is not None and len(keep) >= max_keep:
            break
        rest = np.nonzero(~dead[i + 1:])[0] + i + 1
        if rest.size == 0:
            continue
        inter, union = _inter_union(boxes[i], boxes[rest])
        ok = union > 0.0                                  # 0 / 0 is NaN on the float32 side: never `>`
        lhs, rhs = inter * den, union * num
        off = ok & (lhs != rhs)
        if off.any():
            margin = min(margin, float(np.abs(inter[off] / union[off] - num / den).min()))
        dead[rest[ok & (lhs > rhs)]] = True
    return np.array(keep, np.int64), margin


def batched_nms(boxes, groups, thr):
    """batched_nms over boxes in score order: boxes of different groups never suppress each other.  Kept positions, ascending."""
    groups = np.asarray(groups)
    keep, margin = [], np.inf
    for g in np.unique(groups):
        pos = np.nonzero(groups == g)[0]
        k, m = nms(boxes[pos], thr)
        keep.append(pos[k]); margin = min(margin, m)
    return (np.sort(np.concatenate(keep)) if keep else np.zeros(0, np.int64)), margin


def rpn(logits, anchors, Hr, Wr, pre_n, post_n, thr=0.7, min_size=1e-3):
    """filter_proposals with zero deltas (box = anchor).  logits[l]: flat, anchor order; anchors[l]: [n_l, 4].
    Returns ((level, anchor index) per proposal in output order, their boxes, the NMS margin)."""
    lv, ix, sc, bx = [], [], [], []
    for l, (lg, an) in enumerate(zip(logits, anchors)):
        lg = np.asarray(lg, np.float64).reshape(-1)
        top = stable_order(lg)[:min(lg.size, pre_n)]
        b = clip(an[top], Hr, Wr)
        ok = not_small(b, min_size)
        lv.append(np.full(int(ok.sum()), l)); ix.append(top[ok]); sc.append(lg[top][ok]); bx.append(b[ok])
    lv, ix, sc, bx = np.concatenate(lv), np.concatenate(ix), np.concatenate(sc), np.concatenate(bx)
    order = stable_order(sc)                      # candidates are laid out level by level, rank by rank: index asc = (level, rank) asc
    keep, margin = batched_nms(bx[order], lv[order], thr)
    sel = order[keep[:post_n]]
    return np.stack([lv[sel], ix[sel]], 1), bx[sel], margin


def frcnn(prob, boxes, Hr, Wr, score_thr, thr, det_max):
    """postprocess_detections with zero deltas (every class's box = the proposal).  prob [R, C] float64, boxes [R, 4].
    Returns ((proposal, label) per detection in output order, the NMS margin, the number of candidates)."""
    R, C = prob.shape
    r, c = np.nonzero(prob[:, 1:] > score_thr)
    c = c + 1
    order = stable_order(prob[r, c])              # np.nonzero is row-major: index asc = (proposal, class) asc
    r, c = r[order], c[order]
    keep, margin = batched_nms(clip(boxes, Hr, Wr)[r], c, thr)
    keep = keep[:det_max]
    return np.stack([r[keep], c[keep]], 1), margin, int(order.size)


def retina(scores, boxes, score_thr, thr, per_class, min_box):
    """RetinaNet.postprocess_detections, decisions only.  scores [n, K] float64, boxes [n, 4] decoded and clipped.
    Returns ((anchor, class) per detection in output order, the NMS margin, candidates per class)."""
    out, margin, ncand = [], np.inf, []
    ok = not_small(boxes, min_box)
    for k in range(scores.shape[1]):
        above = scores[:, k] > score_thr
        ncand.append(int(above.sum()))
        idx = np.nonzero(above & ok)[0]
        idx = idx[stable_order(scores[idx, k])]
        keep, m = nms(boxes[idx], thr, per_class)
        margin = min(margin, m)
        out += [(int(i), k) for i in idx[keep]]
    return np.array(out, np.int64).reshape(-1, 2), margin, ncand


def iou_argmax(ref_boxes, boxes):
    """cald_train.py:203-210 per reference box: IoU row against every detection (0 where the boxes do not meet), first maximum.
    Returns (argmax per reference box, smallest non-zero gap between a row's best and second best distinct IoU)."""
    ref_boxes = np.asarray(ref_boxes, np.float64).reshape(-1, 4); boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    arg, gap = [], np.inf
    for a in ref_boxes:
        w = np.minimum(a[2], boxes[:, 2]) - np.maximum(a[0], boxes[:, 0])
        h = np.minimum(a[3], boxes[:, 3]) - np.maximum(a[1], boxes[:, 1])
        inter = w * h
        iou = inter / ((a[2] - a[0]) * (a[3] - a[1]) + (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) - inter)
        iou[(w < 0) | (h < 0)] = 0.0
        j = int(np.argmax(iou))
        arg.append(j)
        lower = iou[iou < iou[j]]
        if lower.size:
            gap = min(gap, float(iou[j] - lower.max()))
    return np.array(arg, np.int64), gap
