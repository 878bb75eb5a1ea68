"""An independent statement of the RetinaNet decision-margin audit (cald_sweep_audit on a RetinaNet, cald_op_retina_audit) in numpy float32,
for tests/test_retina_audit.py and tests/test_gpu_retina_audit.py, and the constructed cases both run.

``records(scores, boxes, ...)`` takes the sigmoid scores [N][K] and the decoded, clipped boxes [N][4] of all N anchors in anchor order
(``scores_of`` / ``grid_anchors`` / ``decode`` of tests/_retina_ssm_restatement.py make them from logits, deltas and base anchors, with the
exponential passed in), runs the tail's decisions itself -- per class: `>` at the threshold, small boxes out, greedy NMS in the order (score
descending, on equal scores the lower anchor index), the first per_class survivors; the list is the classes' lists one after the other --
and returns the seven records in the public numbering, every one a float32 expression in a stated order:

  7  post_thr    d = |s - thr| < 1e-3 of an (anchor, class), unless the class holds per_class detections, the box is small, or ANOTHER kept
                 detection of the class has IoU > nms_thr + 0.01 with it
  15 post_small  min(|w - 1e-2|, |h - 1e-2|) of every (anchor, class) with s > thr
  10 post_cap    class full: s_last - s of every candidate (s > thr, not small) that the last kept detection precedes
  8  post_iou    every other candidate: |mx - nms_thr|, mx = the largest IoU with the kept boxes of the class that precede it (0 without)
  9  post_order  ... and s_kept - s for each of those with IoU > nms_thr
  13 zero_row    scores[0] - scores[1] of the list if both rows are of one class (the hook's slot for the top-2 gap)
  11 ref_subsample  n > 40: the smallest gap of neighbouring rows of one class of which np.round(np.linspace(0, n - 1, 50)) picks exactly one

NaN or a negative value counts as 0; everything else +inf.  ``wrong=`` replaces one rule by a plausible wrong one; tests/test_retina_audit.py
asserts that the cases tell each of them apart.
"""
import numpy as np

import _retina_ssm_restatement as R

F32 = np.float32
N_MARGINS = 16
THR, IOU, ORDER, CAP, SUB, TOP2, SMALL = 7, 8, 9, 10, 11, 13, 15
WRONG = ("ge_window", "cross_class_iou", "small_in_nms", "cap_ignored", "top2_across_classes")
INF = F32(np.inf)


def iou(kb, b):
    """torchvision's nms IoU of every row of kb with b: inter / ((area_i + area_j) - inter), float32 operation by operation."""
    kb = np.ascontiguousarray(kb, F32).reshape(-1, 4); b = np.asarray(b, F32)
    w = np.maximum(F32(0), (np.minimum(kb[:, 2], b[2]) - np.maximum(kb[:, 0], b[0])).astype(F32))
    h = np.maximum(F32(0), (np.minimum(kb[:, 3], b[3]) - np.maximum(kb[:, 1], b[1])).astype(F32))
    inter = (w * h).astype(F32)
    ai = ((kb[:, 2] - kb[:, 0]).astype(F32) * (kb[:, 3] - kb[:, 1]).astype(F32)).astype(F32)
    aj = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / ((ai + aj).astype(F32) - inter).astype(F32)).astype(F32)


def precedes(si, ai, s, a):
    """The tail's sort order (key orderable(score) << 32 | ~anchor, descending)."""
    return si > s or (si == s and ai < a)


def heads_to_inputs(logits, deltas, base, level_hw, sizes, exp):
    """(scores [N][K], boxes [N][4]) from the head tensors in anchor order; sizes = (Hp, Wp, Hr, Wr)."""
    Hp, Wp, Hr, Wr = sizes
    anchors = R.grid_anchors(base, level_hw, Hp, Wp)
    return R.scores_of(logits, exp=exp), R.decode(deltas, anchors, Hr, Wr, exp=exp)


def records(scores, boxes, score_thr=0.05, nms_thr=0.5, per_class=300, min_box=1e-2, wrong=None):
    """dict(margins float32 [16], n, anchor [n], cls [n], scores [n])."""
    assert wrong is None or wrong in WRONG
    s = np.ascontiguousarray(scores, F32); b = np.ascontiguousarray(boxes, F32).reshape(-1, 4)
    N, K = s.shape
    thr, nt, mb = F32(score_thr), F32(nms_thr), F32(min_box)
    cover = F32(nt + F32(0.01))
    w = (b[:, 2] - b[:, 0]).astype(F32); h = (b[:, 3] - b[:, 1]).astype(F32)
    small = ~((w >= mb) & (h >= mb))
    if wrong == "small_in_nms":
        small = np.zeros(N, bool)
    cap = N + 1 if wrong == "cap_ignored" else per_class
    m = np.full(N_MARGINS, INF, F32)

    def upd(q, v):
        v = F32(v)
        if not v >= 0:
            v = F32(0)
        if v < m[q]:
            m[q] = v

    # the tail's own decisions
    kept = []
    for k in range(K):
        cand = [int(a) for a in np.nonzero(s[:, k] > thr)[0] if not small[a]]
        cand.sort(key=lambda a: (-float(s[a, k]), a))
        keep = []
        for a in cand:
            if len(keep) >= cap:
                break
            if keep:
                v = iou(b[keep], b[a])
                if (v > nt).any():
                    continue
            keep.append(a)
        kept.append(keep)
    # the records
    for k in range(K):
        keep = kept[k]
        full = len(keep) >= cap
        if wrong == "cross_class_iou":
            ca = np.array([a for q in range(K) for a in kept[q]], np.int64); cc = np.array([q for q in range(K) for _ in kept[q]], np.int64)
        else:
            ca = np.array(keep, np.int64); cc = np.full(len(keep), k, np.int64)
        cs = s[ca, cc] if ca.size else np.zeros(0, F32)
        cb = b[ca] if ca.size else np.zeros((0, 4), F32)
        d = np.abs((s[:, k] - thr).astype(F32))
        is_cand = s[:, k] > thr
        window = d <= F32(1e-3) if wrong == "ge_window" else d < F32(1e-3)
        for a in np.nonzero(is_cand | window)[0]:
            a = int(a); sa = s[a, k]
            if is_cand[a]:
                upd(SMALL, min(np.abs(F32(w[a] - mb)), np.abs(F32(h[a] - mb))))
            if small[a]:
                continue
            if window[a] and not full:
                other = ~((ca == a) & (cc == k))
                if not (iou(cb[other], b[a]) > cover).any():
                    upd(THR, d[a])
            if not is_cand[a]:
                continue
            if full and precedes(s[keep[-1], k], keep[-1], sa, a):
                upd(CAP, F32(s[keep[-1], k] - sa))
                continue
            pre = np.array([precedes(cs[j], int(ca[j]), sa, a) for j in range(ca.size)], bool)
            v = iou(cb[pre], b[a])
            ok = ~np.isnan(v)                                        # (0 / 0 of two empty boxes: `iou > mx` is false)
            v, vs = v[ok], cs[pre][ok]
            mx = F32(max(F32(0), v.max())) if v.size else F32(0)
            upd(IOU, np.abs(F32(mx - nt)))
            for j in np.nonzero(v > nt)[0]:
                upd(ORDER, F32(vs[j] - sa))
    anchor = np.array([a for k in range(K) for a in kept[k]], np.int64); cls = np.array([k for k in range(K) for _ in kept[k]], np.int64)
    sc = s[anchor, cls].astype(F32) if anchor.size else np.zeros(0, F32)
    n = int(anchor.size)
    if n >= 2 and (cls[0] == cls[1] or wrong == "top2_across_classes"):
        upd(TOP2, F32(sc[0] - sc[1]))
    if n > 40:
        picked = np.zeros(n, bool)
        picked[np.round(np.linspace(0, n - 1, 50)).astype(np.int64)] = True
        for i in range(n - 1):
            if picked[i] != picked[i + 1] and cls[i] == cls[i + 1]:
                upd(SUB, F32(sc[i] - sc[i + 1]))
    return dict(margins=m, n=n, anchor=anchor, cls=cls, scores=sc)


# ---------------------------------------------------------------------------------------------------------------------------
# constructed cases: K = 3, five levels of 1 x 1 pixels (anchor i = level * A + a sits at the origin, so its box is base[level][a] moved
# by its deltas), a 64 x 64 image, zero deltas and integer boxes unless a case says otherwise.  Each builder returns the head tensors, the
# hook's arguments and `design`: what the case was built to show, as a function of the scores and boxes the restatement sees.
# ---------------------------------------------------------------------------------------------------------------------------
ONES = ((1, 1),) * 5
FAR = -10.0                                      # sigmoid 4.5e-5: below the threshold and outside its window


def logit(p):
    return F32(np.log(p / (1.0 - p)))


class Case:
    def __init__(self, K=3, A=9, level_hw=ONES, sizes=(64, 64, 64, 64), per_class=10, score_thr=0.05, nms_thr=0.5):
        self.K, self.A, self.level_hw, self.sizes, self.per_class, self.score_thr, self.nms_thr = K, A, level_hw, sizes, per_class, score_thr, nms_thr
        self.N = sum(hh * ww for hh, ww in level_hw) * A
        self.logits = np.full((self.N, K), FAR, F32)
        self.deltas = np.zeros((self.N, 4), F32)
        self.base = np.tile(np.array([0, 0, 4, 4], F32), (5, A, 1))
        self.design = lambda s, b: {}
        self.n = None                             # detections the case was built to give (None: not stated)

    def put(self, i, box, **cls_p):
        """anchor i (1 x 1 levels only) gets `box` and, per class c<k>=p, the logit of probability p."""
        self.base[i // self.A, i % self.A] = np.asarray(box, F32)
        for name, p in cls_p.items():
            self.logits[i, int(name[1:])] = logit(p)

    def heads(self):
        """(cls, reg): per level [H][W][A * K] and [H][W][A * 4], the hook's layout."""
        cls, reg, off = [], [], 0
        for hh, ww in self.level_hw:
            n = hh * ww * self.A
            cls.append(np.ascontiguousarray(self.logits[off:off + n].reshape(hh, ww, self.A * self.K)))
            reg.append(np.ascontiguousarray(self.deltas[off:off + n].reshape(hh, ww, self.A * 4)))
            off += n
        return cls, reg

    def inputs(self, exp):
        return heads_to_inputs(self.logits, self.deltas, self.base, self.level_hw, self.sizes, exp)

    def restate(self, exp, wrong=None):
        s, b = self.inputs(exp)
        return records(s, b, self.score_thr, self.nms_thr, self.per_class, wrong=wrong)


def _d(s, thr=0.05):
    return np.abs(F32(F32(s) - F32(thr)))


def case_thr_window():
    """Scores at thr + 3e-4 (kept) and thr - 3e-4 count; thr - 1e-4 inside a kept detection of its class (IoU 0.81 > 0.51) does not;
    thr + 2e-3 is outside the window."""
    c = Case()
    c.put(0, [0, 0, 20, 20], c0=0.9)
    c.put(1, [30, 0, 40, 10], c0=0.05 + 3e-4)
    c.put(2, [30, 20, 40, 30], c0=0.05 - 3e-4)
    c.put(3, [1, 1, 19, 19], c0=0.05 - 1e-4)
    c.put(4, [42, 0, 52, 10], c0=0.05 + 2e-3)
    c.design = lambda s, b: {THR: min(_d(s[1, 0]), _d(s[2, 0])), CAP: INF, ORDER: INF}
    c.n = 3
    return c


def case_thr_other_class():
    """... and the same covered box with the same score in ANOTHER class counts: nothing of class 1 covers it."""
    c = case_thr_window()
    c.put(3, [1, 1, 19, 19], c0=0.05 - 1e-4, c1=0.05 - 1e-4)
    c.design = lambda s, b: {THR: _d(s[3, 1]), CAP: INF, ORDER: INF}
    return c


def case_iou():
    """Class 0: Q has IoU 600 / 1170 with the kept P (suppressed: an order record), R has 600 / 1230 (kept).  The boxes of P and Q again in
    classes 1 and 2: no record between classes, whatever their scores."""
    c = Case()
    c.put(0, [0, 0, 30, 30], c0=0.9)
    c.put(1, [0, 10, 30, 39], c0=0.8)
    c.put(2, [0, 10, 30, 41], c0=0.7)
    c.put(3, [0, 0, 30, 30], c1=0.9)
    c.put(4, [0, 10, 30, 39], c2=0.85)
    c.design = lambda s, b: {IOU: np.abs(F32(F32(F32(600) / F32(1230)) - F32(0.5))), ORDER: F32(s[0, 0] - s[1, 0]), CAP: INF, THR: INF, TOP2: F32(s[0, 0] - s[2, 0])}
    c.n = 4
    return c


def case_iou_tie():
    """Two candidates of one class with the same logit and IoU 360 / 440: the lower anchor index is kept, the order margin is 0."""
    c = Case()
    c.put(7, [40, 40, 60, 60], c1=0.6)
    c.put(5, [40, 42, 60, 62], c1=0.6)
    c.put(0, [0, 0, 30, 30], c0=0.9)
    c.design = lambda s, b: {ORDER: F32(0), IOU: np.abs(F32(F32(F32(360) / F32(440)) - F32(0.5))), TOP2: INF}
    c.n = 2
    return c


def case_cap():
    """per_class = 2.  Class 0: four disjoint candidates and one just above the threshold -- the cap record is second - third, and the
    class gives no threshold record.  Class 1: exactly two candidates (full, nothing behind the cut) and a score just below the threshold."""
    c = Case(per_class=2)
    for i, p in enumerate((0.9, 0.8, 0.7, 0.6)):
        c.put(i, [16 * i, 0, 16 * i + 10, 10], c0=p)
    c.put(4, [0, 20, 10, 30], c0=0.05 + 2e-4)
    c.put(5, [0, 40, 10, 50], c1=0.9)
    c.put(6, [20, 40, 30, 50], c1=0.85)
    c.put(7, [40, 40, 50, 50], c1=0.05 - 2e-4)
    c.design = lambda s, b: {CAP: F32(s[1, 0] - s[2, 0]), THR: INF, ORDER: INF, IOU: F32(0.5)}
    c.n = 4
    return c


def case_small(step):
    """A box of width 1e-2 + step float32 steps (step -1: small, no detection; 0 and +1: kept), clipped at the bottom; a box whose deltas
    move it above the image (height 0 after the clip)."""
    c = Case()
    x2 = F32(1e-2)
    for _ in range(abs(step)):
        x2 = np.nextafter(x2, F32(1) if step > 0 else F32(0), dtype=F32)
    c.put(0, [0, 50, x2, 70], c0=0.9)
    c.put(1, [10, 10, 30, 30], c1=0.9)
    c.deltas[1, 1] = -3.0
    spacing = np.spacing(F32(1e-2))
    c.design = lambda s, b: {SMALL: F32(abs(step) * spacing), THR: INF, ORDER: INF, CAP: INF, IOU: INF if step < 0 else F32(0.5)}
    c.n = 0 if step < 0 else 1
    return c


def case_small_pair():
    """Two boxes 0.005 wide with IoU 39 / 40, both above the threshold: small boxes take no part in NMS -- no IoU record, no detection."""
    c = Case()
    c.put(0, [0, 0, 0.005, 40], c2=0.9)
    c.put(1, [0, 1, 0.005, 40], c2=0.8)
    c.design = lambda s, b: {SMALL: np.abs(F32(F32(0.005) - F32(1e-2))), IOU: INF, ORDER: INF, TOP2: INF}
    c.n = 0
    return c


def case_nothing():
    c = Case()
    c.design = lambda s, b: {q: INF for q in range(N_MARGINS)}
    c.n = 0
    return c


def _cells(n, pitch=7, side=6, per_row=9):
    return [[(i % per_row) * pitch, (i // per_row) * pitch, (i % per_row) * pitch + side, (i // per_row) * pitch + side] for i in range(n)]


def case_sub_two_classes():
    """60 disjoint detections, n0 of class 0 then 60 - n0 of class 1, A = 16 (80 anchors).  n0 is chosen so that linspace picks exactly one
    of the rows n0 - 1, n0: that pair straddles the class boundary and gives no record; the pairs inside a class do."""
    n = 60
    picked = np.zeros(n, bool); picked[np.round(np.linspace(0, n - 1, 50)).astype(np.int64)] = True
    n0 = next(i for i in range(20, 40) if picked[i - 1] != picked[i])
    c = Case(A=16, per_class=64)
    rs = np.random.RandomState(6)
    gaps = rs.randint(1, 9, n).astype(np.float64) * 0.002
    for cls, rows in ((0, range(n0)), (1, range(n0, n))):
        p = 0.95
        for r in rows:
            p -= gaps[r]
            c.put(r, _cells(n)[r], **{"c%d" % cls: p})

    def design(s, b):
        sc = np.concatenate([s[:n0, 0], s[n0:n, 1]]).astype(F32)
        inside = [F32(sc[i] - sc[i + 1]) for i in range(n - 1) if picked[i] != picked[i + 1] and i + 1 != n0]
        assert sc[n0 - 1] < sc[n0]                # across the boundary the "gap" is negative: counting it would flag 0
        return {SUB: min(inside), TOP2: F32(sc[0] - sc[1]), ORDER: INF, CAP: INF}
    c.design = design
    c.n = n
    return c


def case_sub_41():
    """One class, n = 41: more than 40, so the sub-sample is taken -- and 50 picks over 41 rows take every row: no record."""
    c = Case(per_class=64)
    for r in range(41):
        c.put(r, _cells(41)[r], c1=0.9 - 0.01 * r)
    c.design = lambda s, b: {SUB: INF, TOP2: F32(s[0, 1] - s[1, 1])}
    c.n = 41
    return c


def case_many():
    """Level 0 of 32 x 32 pixels, A = 9: 9 216 candidates of class 0, more than the tail sorts in LDS; seeded anchors, deltas and scores,
    a few equal scores, per_class = 100 (the class is full)."""
    level_hw = ((32, 32), (1, 1), (1, 1), (1, 1), (1, 1))
    c = Case(level_hw=level_hw, sizes=(256, 256, 250, 243), per_class=100)
    rs = np.random.RandomState(7)
    n0 = 32 * 32 * 9
    c.logits[:n0, 0] = np.maximum(rs.randn(n0) * 1.5 + 1.0, -2.5).astype(F32)
    c.logits[100:110, 0] = c.logits[200:210, 0]                      # equal scores: decided by the anchor index
    c.logits[rs.randint(0, n0, 40), 1] = logit(0.05) + (rs.randn(40) * 0.01).astype(F32)
    wh = rs.randint(6, 40, (5, 9, 2)).astype(F32)
    c.base = np.concatenate([-wh / 2, wh / 2], -1).astype(F32)
    c.deltas[:] = (rs.randn(c.N, 4) * 0.3).astype(F32)
    return c


CASES = {
    "thr_window": case_thr_window, "thr_other_class": case_thr_other_class, "iou": case_iou, "iou_tie": case_iou_tie, "cap": case_cap,
    "small_minus": lambda: case_small(-1), "small_exact": lambda: case_small(0), "small_plus": lambda: case_small(1),
    "small_pair": case_small_pair, "nothing": case_nothing, "sub_two_classes": case_sub_two_classes, "sub_41": case_sub_41,
    "many": case_many,
}
