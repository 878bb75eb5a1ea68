"""Plain numpy restatement of the scoring stage (cald_amd/csrc/score.hip and the host tail of the ls_c sweep): float32 arithmetic in the
operation order the kernels state, every decision written out.  No GPU, no library, no oracle: the Jensen-Shannon divergence, the one
piece with a polynomial logarithm, is passed in by the caller (`js`, a function of two class vectors).

The pair audit has no oracle function; pair_audit() below is its specification, written from score.hip's comment and the margin
definitions of include/cald_hip.h: per pair, `gap` is the smallest (best IoU - best IoU among detections whose proposal differs from the
winner's) over the reference boxes with a positive best IoU, and `zero` says that some reference box has no positive IoU at all.

`wrong` names deliberately wrong variants (WRONG below).  They exist so that the tests can assert that the constructed cases would notice
each of those mistakes; the product is compared with wrong = () only.
"""
import math

import numpy as np

F32 = np.float32
CHUNK = 2048          # detections the consistency kernel stages at a time
WRONG = ("identity_sel", "ref_n_ignored", "chunk_local_index", "last_maximum", "rotate_no_clamp", "flip_w_minus_1", "ref_view_all",
         "label0_dropped", "audit_no_filter", "lt_no_plus_1", "ls_ties_reversed")


def subsample_indices(n):
    """cald_train.py:110-113"""
    return np.arange(n) if n <= 40 else np.round(np.linspace(0, n - 1, 50)).astype(int)


# ---------------------------------------------------------------------------------------------------------------------------
# pair parameters
# ---------------------------------------------------------------------------------------------------------------------------
def rotate_canvas(H, W, angle_deg):
    """(width, height) of PIL's Image.rotate(angle, expand=True) result"""
    angle = math.fmod(angle_deg, 360.0)
    if angle < 0:
        angle += 360.0
    if angle in (90.0, 270.0):
        return H, W
    w, h = float(W), float(H)
    cx, cy = w / 2.0, h / 2.0
    ang = -(angle * (math.pi / 180.0))
    m = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
    m[2] = (m[0] * -cx + m[1] * -cy + m[2]) + cx
    m[5] = (m[3] * -cx + m[4] * -cy + m[5]) + cy
    xs = [m[0] * x + m[1] * y + m[2] for x, y in ((0.0, 0.0), (w, 0.0), (w, h), (0.0, h))]
    ys = [m[3] * x + m[4] * y + m[5] for x, y in ((0.0, 0.0), (w, 0.0), (w, h), (0.0, h))]
    return math.ceil(max(xs)) - math.floor(min(xs)), math.ceil(max(ys)) - math.floor(min(ys))


def pair_params(kind, H, W, param=0.0):
    """the 12 floats a pair carries: 1 flip {W}, 2 resize {ratio}, 3 rotate {a00 a01 a02 a10 a11 a12 sx sy W H} (cald_helper.py:135-222)"""
    p = np.zeros(12, F32)
    if kind == 1:
        p[0] = F32(W)
    elif kind == 2:
        p[0] = F32(param)
    elif kind == 3:
        pw, ph = rotate_canvas(H, W, param)
        ang = param * (math.pi / 180.0)
        alpha, beta, cx, cy = math.cos(ang), math.sin(ang), W / 2.0, H / 2.0
        m02, m12 = (1 - alpha) * cx - beta * cy, beta * cx + (1 - alpha) * cy
        nW, nH = int(H * abs(beta) + W * abs(alpha)), int(H * abs(alpha) + W * abs(beta))
        m02 += nW / 2.0 - cx
        m12 += nH / 2.0 - cy
        p[:10] = [alpha, beta, m02, -beta, alpha, m12, pw / W, ph / H, W, H]
    return p


def aug_box(boxes, kind, par, wrong=()):
    """the reference boxes as the augmented view sees them; boxes [N][4] float32"""
    b = np.array(boxes, F32).reshape(-1, 4)
    par = np.asarray(par, F32)
    if kind == 1:
        Wd = par[0] - F32(1) if "flip_w_minus_1" in wrong else par[0]
        b = np.stack([Wd - b[:, 2], b[:, 1], Wd - b[:, 0], b[:, 3]], 1)
    elif kind == 2:
        b = b * par[0]
    elif kind == 3:
        bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        xs = np.stack([b[:, 0], b[:, 0] + bw, b[:, 0], b[:, 2]], 1)
        ys = np.stack([b[:, 1], b[:, 1], b[:, 1] + bh, b[:, 3]], 1)
        X = (par[0] * xs + par[1] * ys) + par[2] * F32(1)
        Y = (par[3] * xs + par[4] * ys) + par[5] * F32(1)
        r = np.stack([X.min(1) / par[6], Y.min(1) / par[7], X.max(1) / par[6], Y.max(1) / par[7]], 1)
        if "rotate_no_clamp" not in wrong:
            r = np.stack([np.clip(r[:, 0], F32(0), par[8]), np.clip(r[:, 1], F32(0), par[9]),
                          np.clip(r[:, 2], F32(0), par[8]), np.clip(r[:, 3], F32(0), par[9])], 1)
        b = r
    return b.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# IoU rows and their argmax
# ---------------------------------------------------------------------------------------------------------------------------
def iou_matrix(a, b):
    """cald_train.py:203-210: [N][M] float32"""
    a = np.asarray(a, F32).reshape(-1, 4)[:, None, :]
    b = np.asarray(b, F32).reshape(-1, 4)[None, :, :]
    with np.errstate(all="ignore"):
        w = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
        h = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
        aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        ba = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        inter = w * h
        iou = inter / ((aa + ba) - inter)
    iou[w < 0] = 0
    iou[h < 0] = 0
    return iou.astype(F32)


def argmax_first(row, wrong=()):
    """torch.argmax: the first maximum, NaN is maximal.  Returns (value, index)"""
    nan = np.isnan(row)
    tied = np.flatnonzero(nan) if nan.any() else np.flatnonzero(row == row.max())
    if "last_maximum" in wrong:
        j = tied[-1]
    elif "chunk_local_index" in wrong:          # ties go to the smallest index within the staged chunk
        j = min(tied, key=lambda t: (t % CHUNK, t))
    else:
        j = tied[0]
    return row[j], int(j)


def second_gap(iou):
    """smallest (best - runner-up) over the rows of an IoU matrix with at least two columns (the cases assert it)"""
    s = np.sort(iou.astype(np.float64), axis=1)
    return float((s[:, -1] - s[:, -2]).min())


# ---------------------------------------------------------------------------------------------------------------------------
# the five kernels
# ---------------------------------------------------------------------------------------------------------------------------
def consistency(ab, ref_scls, ref_pm, boxes, scls, pm, bp, js, wrong=(), detail=None):
    """cald_train.py:189-224 for one pair: min over the reference boxes of |max IoU + 0.5 (1 - JS)(p_ref + p_det) - bp|, initial 1.0;
    an empty view gives 0.0"""
    if len(boxes) == 0:
        return F32(0)
    iou = iou_matrix(ab, boxes)
    cons = F32(1)
    for i in range(len(ab)):
        best, j = argmax_first(iou[i], wrong)
        t = F32(0.5) * (F32(1) - F32(js(ref_scls[i], scls[j])))
        u = F32(ref_pm[i]) + F32(pm[j])
        s = np.abs((best + t * u) - F32(bp))
        if s < cons:
            cons = s
        if detail is not None:
            detail.append((best, j, s))
    return F32(cons)


def pair_audit(ab, boxes, props, wrong=()):
    """(gap, zero) of one pair; the module docstring is the specification"""
    if len(boxes) == 0:
        return F32(np.inf), F32(0)
    iou = iou_matrix(ab, boxes)
    props = np.asarray(props, F32).reshape(-1, 4)
    gap, zero = F32(np.inf), F32(0)
    for i in range(len(ab)):
        best, j = argmax_first(iou[i])
        if not best > 0:
            zero = F32(1)
            continue
        other = (props != props[j]).any(1)
        if "audit_no_filter" in wrong:
            other = np.arange(len(boxes)) != j
        vals = iou[i][other]
        vals = vals[vals > 0]
        second = vals.max() if len(vals) else F32(0)
        gap = min(gap, F32(best - second))
    return F32(gap), zero


def max_iou_rows(refs, boxes):
    """ls_c_train.py:136-150: the largest IoU of every reference box in one view (NaN is maximal); 0 for an empty view"""
    refs = np.asarray(refs, F32).reshape(-1, 4)
    if len(boxes) == 0:
        return np.zeros(len(refs), F32)
    iou = iou_matrix(refs, boxes)
    return np.array([argmax_first(r)[0] for r in iou], F32).reshape(len(refs))


def lt_uncertainty(boxes, props, pm, wrong=()):
    """lt_c_train.py:92-121: min over detections of |calcu_iou(box, proposal) + prob_max - 1|, initial 1.0; calcu_iou counts pixels
    (+ 1) in the overlap and in the heights, not in the widths of the areas"""
    one = F32(0) if "lt_no_plus_1" in wrong else F32(1)
    unc = F32(1)
    A, B = np.asarray(boxes, F32).reshape(-1, 4), np.asarray(props, F32).reshape(-1, 4)
    for i in range(len(A)):
        width = (min(A[i, 2], B[i, 2]) - max(A[i, 0], B[i, 0])) + one
        height = (min(A[i, 3], B[i, 3]) - max(A[i, 1], B[i, 1])) + one
        iou = F32(0)
        if not (width <= 0 or height <= 0):
            aa = (A[i, 2] - A[i, 0]) * ((A[i, 3] - A[i, 1]) + one)
            ba = (B[i, 2] - B[i, 0]) * ((B[i, 3] - B[i, 1]) + one)
            iner = width * height
            with np.errstate(all="ignore"):
                iou = iner / ((aa + ba) - iner)
        u = np.abs((iou + F32(pm[i])) - F32(1))
        if u < unc:                 # a NaN never wins
            unc = u
    return F32(unc)


def cls_corr(scores, labels, C, sel=None, wrong=()):
    """cald_train.py:114-117, :194-197: per class the largest score; label 0 wraps to the last slot (python's negative index), labels
    beyond the table are skipped.  sel: the detections that count (a reference view's sub-sample)"""
    out = np.zeros(C - 1, F32)
    for d in (range(len(scores)) if sel is None else sel):
        l = int(labels[d]) - 1
        if l < 0:
            if "label0_dropped" in wrong:
                continue
            l += C - 1
        if l < 0 or l >= C - 1:
            continue
        if scores[d] > out[l]:
            out[l] = scores[d]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# ls_c host tail
# ---------------------------------------------------------------------------------------------------------------------------
def ls_select(pm, wrong=()):
    """the scored reference boxes: all while n <= 30, else torch.topk(prob_max, 30) with ties to the lower index"""
    n = len(pm)
    if n <= 30:
        return list(range(n))
    sign = -1 if "ls_ties_reversed" in wrong else 1
    return sorted(range(n), key=lambda i: (-float(pm[i]), sign * i))[:30]


def ls_tail(pm_sel, rows):
    """ls_c_train.py:151-153: rows [n_views][N] float32 max-IoU rows of the noisy views -> the float64 score"""
    pm_sel = np.asarray(pm_sel, F32)
    if len(pm_sel) == 0:
        return 0.0
    U = float(np.max(F32(1) - pm_sel))
    stab = [0.0] * len(pm_sel)
    for r in rows:
        for k in range(len(pm_sel)):
            stab[k] += float(r[k])
    st = np.array(stab) / 6.0
    return float(np.sum(pm_sel * st) / np.sum(pm_sel) - U)


# ---------------------------------------------------------------------------------------------------------------------------
# one batch in the sweep's layout (the arrays of cald_score_probe) -> every output of cald_op_score_batch
# ---------------------------------------------------------------------------------------------------------------------------
def selection(case, img, wrong=()):
    n = 50 if "ref_n_ignored" in wrong else int(case["ref_n"][img])
    return list(range(n)) if "identity_sel" in wrong else [int(x) for x in case["ref_sel"][img][:n]]


def score_batch(case, js, wrong=(), max_iou_fill=None):
    """case: dict of the probe's input arrays ([V][cap]... as in include/cald_hip.h).  max_iou slots from ref_n on keep max_iou_fill"""
    V, P, C = case["V"], case["P"], case["C"]
    cnt = case["count"]
    out = dict(cons=np.zeros(P, F32), cls_corr=np.zeros((V, C - 1), F32), pair_audit=np.zeros((P, 2), F32),
               max_iou=np.zeros((P, 50), F32) if max_iou_fill is None else max_iou_fill.copy(), lt=np.zeros(V, F32))
    for p in range(P):
        rv, av, img = int(case["ref_view"][p]), int(case["aug_view"][p]), int(case["pair_img"][p])
        sel = selection(case, img, wrong)
        M = int(cnt[av])
        refs = case["boxes"][rv][sel]
        ab = aug_box(refs, int(case["aug_kind"][p]), case["aug_param"][p], wrong)
        out["cons"][p] = consistency(ab, case["scores_cls"][rv][sel], case["prob_max"][rv][sel], case["boxes"][av][:M],
                                     case["scores_cls"][av][:M], case["prob_max"][av][:M], case["bp"], js, wrong)
        out["pair_audit"][p] = pair_audit(ab, case["boxes"][av][:M], case["props"][av][:M], wrong)
        out["max_iou"][p, :len(sel)] = max_iou_rows(refs, case["boxes"][av][:M])
    for v in range(V):
        n = int(cnt[v])
        sel = None
        if case["view_isref"][v] and "ref_view_all" not in wrong:
            sel = selection(case, int(case["view_img"][v]), wrong)
        out["cls_corr"][v] = cls_corr(case["scores"][v][:n], case["labels"][v][:n], C, sel, wrong)
        out["lt"][v] = lt_uncertainty(case["boxes"][v][:n], case["props"][v][:n], case["prob_max"][v][:n], wrong)
    return out
