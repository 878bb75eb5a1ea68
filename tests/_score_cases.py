"""Constructed inputs of the scoring-stage tests (test_score_batch.py on the CPU, test_gpu_score_batch.py on the GPU): one batch in the
sweep's layout that reaches every edge of score.hip on purpose, a second tiny batch for lt_uncertainty_kernel, and the ls_c tail cases.

The batch.  Three images.  Image 0 (301 x 401) has 73 reference detections of which subsample_indices(73) picks 50; its augmented views
hold jittered copies of the transformed reference boxes, so its pairs are ordinary work: 13 rounds of the consistency kernel, the last
with two idle waves.  Image 1 (211 x 333) scores three boxes in reversed order -- A, Bc, Cn -- and its views isolate one reference box
each: the other two rows meet nothing (IoU exactly 0, argmax 0, a score of at least 0.3), the row of interest carries the class vector
of its detection (JS = 0) and a prob_max that puts its score below 0.1.  What the pair returns is then a function of that row alone.
Image 2 scores nothing (ref_n = 0).  All boxes are integers; an IoU against an untransformed or flipped box is the correctly rounded
quotient of two exact integers."""
import numpy as np

import _score_restatement as R

F32 = np.float32
CAP = 2112
IMG_HW = [(301, 401), (211, 333), (157, 205)]
A_BOX, BC_BOX, CN_BOX = [70, 90, 130, 190], [0, 0, 50, 211], [140, 40, 190, 80]
SEL1 = [9, 5, 2]                      # image 1's scored detections: A, Bc, Cn
FAR = (75, 0, 135, 36)                # region no transformed box of image 1 reaches
VIEW_COUNTS = dict(ref0=73, ref1=60, ref2=5, g_flip_small=100, g_rot=100, g_rot90_big=100, v0=0, v1=1, v63=63, v64=64, v65=65, v100=100,
                   v2049=2049)
VIEWS = list(VIEW_COUNTS)


def _rand_boxes(rs, n, x0, y0, x1, y1, wmin=8, wmax=60):
    w, h = rs.randint(wmin, wmax, n), rs.randint(wmin, wmax, n)
    x = rs.randint(x0, max(x0 + 1, x1 - wmax), n)
    y = rs.randint(y0, max(y0 + 1, y1 - wmax), n)
    return np.stack([x, y, x + w, y + h], 1).astype(F32)


def _far(rs, n):
    return _rand_boxes(rs, n, *FAR, wmin=5, wmax=12)


def _jitter(rs, b):
    """integer boxes near b, still with positive width and height"""
    b = np.round(np.asarray(b, np.float64))
    j = b + rs.randint(-3, 4, b.shape)
    j[:, 2] = np.maximum(j[:, 2], j[:, 0] + 4)
    j[:, 3] = np.maximum(j[:, 3], j[:, 1] + 4)
    return j.astype(F32)


def batch_case(C):
    rs = np.random.RandomState(100 + C)
    V, n_img = len(VIEWS), 3
    vi = {name: k for k, name in enumerate(VIEWS)}
    count = np.array([VIEW_COUNTS[v] for v in VIEWS], np.int32)
    boxes = np.zeros((V, CAP, 4), F32)
    scls = rs.dirichlet(np.ones(C), (V, CAP)).astype(F32)
    pm = scls[:, :, 1:].max(2).copy()
    scores = (0.05 + 0.85 * rs.rand(V, CAP)).astype(F32)
    labels = rs.randint(1, C, (V, CAP)).astype(np.int64)
    for v in range(V):                      # slots beyond the count hold plausible garbage: a kernel that reads them is noticed
        boxes[v] = _rand_boxes(rs, CAP, 0, 0, 400, 300)

    # ---- reference views and what is scored of them ----
    ref_sel = np.zeros((n_img, 50), np.int32)
    ref_n = np.array([50, 3, 0], np.int32)
    ref_sel[0] = R.subsample_indices(73)
    ref_sel[1] = SEL1 + [k for k in range(60) if k not in SEL1][:47]      # the slots beyond ref_n hold valid indices that must not be read
    ref_sel[2] = np.arange(50) % 5
    boxes[vi["ref0"], :73] = _rand_boxes(rs, 73, 5, 5, 395, 295, 20, 90)
    boxes[vi["ref1"], :60] = _rand_boxes(rs, 60, 150, 0, 330, 210)
    for k, b in zip(SEL1, (A_BOX, BC_BOX, CN_BOX)):
        boxes[vi["ref1"], k] = b
    pm[vi["ref1"], SEL1] = [0.9, 0.4, 0.3]
    sel0 = ref_sel[0]
    refs0 = boxes[vi["ref0"]][sel0]

    pairs = []                              # (image, augmented view, kind, parameter)
    def par(img, kind, prm=0.0):
        return R.pair_params(kind, IMG_HW[img][0], IMG_HW[img][1], prm)

    # ---- image 0: ordinary pairs; a view holds the jittered transformed boxes of two augmentations ----
    for name, augs in (("g_flip_small", ((1, 0.0), (2, 0.8))), ("g_rot", ((3, 5.0), (3, -5.0))), ("g_rot90_big", ((3, 90.0), (2, 1.2)))):
        for half, (kind, prm) in enumerate(augs):
            boxes[vi[name], 50 * half:50 * half + 50] = _jitter(rs, R.aug_box(refs0, kind, par(0, kind, prm)))[rs.permutation(50)]
            pairs.append((0, name, kind, prm))
    pairs.append((0, "g_rot", 0, 0.0))      # boxes unchanged against a view that was not built for it
    pairs.append((0, "v0", 1, 0.0))
    pairs.append((0, "v2049", 0, 0.0))      # the chunked pair, among unchunked ones

    # ---- image 1: one reference box at a time ----
    def tie_to(view, j_first, j_second, ref_k):
        """the upper and the lower half of A: IoU exactly 1/2 each; same class vector as A, different prob_max"""
        boxes[vi[view], j_first] = [70, 90, 130, 140]
        boxes[vi[view], j_second] = [70, 140, 130, 190]
        scls[vi[view], [j_first, j_second]] = scls[vi["ref1"], ref_k]
        pm[vi[view], j_first], pm[vi[view], j_second] = 0.8, 0.5
    for name in ("v1", "v63", "v64", "v65", "v100"):
        boxes[vi[name], :VIEW_COUNTS[name]] = _far(rs, VIEW_COUNTS[name])
    boxes[vi["v2049"], :2049] = _rand_boxes(rs, 2049, 200, 0, 400, 300)
    slots = rs.permutation(np.setdiff1d(np.arange(2049), [0, 1000, 2048]))[:50]
    boxes[vi["v2049"], slots] = _jitter(rs, refs0)
    tie_to("v2049", 1000, 2048, SEL1[0])    # across the chunk boundary: the later one has the smaller index within its chunk
    pairs.append((1, "v2049", 0, 0.0))
    tie_to("v64", 0, 63, SEL1[0])           # lane 0 and lane 63 of one pass
    pairs.append((1, "v64", 0, 0.0))
    ties = [(len(pairs) - 2, 0, 1000, 2048), (len(pairs) - 1, 0, 0, 63)]       # (pair, row, first, second)
    # one pixel apart, one detection
    boxes[vi["v1"], 0] = [71, 91, 131, 191]; scls[vi["v1"], 0] = scls[vi["ref1"], SEL1[0]]; pm[vi["v1"], 0] = 0.1
    pairs.append((1, "v1", 0, 0.0))
    # flip: the last detection of 63 is Cn mirrored, exactly
    boxes[vi["v63"], 62] = R.aug_box([CN_BOX], 1, par(1, 1))[0]; scls[vi["v63"], 62] = scls[vi["ref1"], SEL1[2]]; pm[vi["v63"], 62] = 0.3
    pairs.append((1, "v63", 1, 0.0))
    # best and runner-up from one proposal (64 and 3), the best of another proposal (10) further away
    a = np.array(A_BOX, F32)
    boxes[vi["v65"], 64], boxes[vi["v65"], 3], boxes[vi["v65"], 10] = a, a + [10, 0, 10, 0], a + [30, 0, 30, 0]
    scls[vi["v65"], 64] = scls[vi["ref1"], SEL1[0]]; pm[vi["v65"], 64] = 0.35
    pairs.append((1, "v65", 0, 0.0))
    # rotate: Bc spans the image's height at its left edge, two of its corners leave the image (left and top); the last detection of 100 is the clamped box
    rb = R.aug_box([BC_BOX], 3, par(1, 3, -5.0))[0]
    raw = R.aug_box([BC_BOX], 3, par(1, 3, -5.0), wrong=("rotate_no_clamp",))[0]
    assert (rb != raw).sum() == 2, (rb, raw)
    boxes[vi["v100"], 99] = np.round(rb); scls[vi["v100"], 99] = scls[vi["ref1"], SEL1[1]]; pm[vi["v100"], 99] = 0.4
    pairs.append((1, "v100", 3, -5.0))
    pairs.append((1, "v0", 3, 5.0))
    # ---- image 2: nothing is scored ----
    pairs.append((2, "v100", 2, 0.8))
    pairs.append((2, "v0", 0, 0.0))

    props = boxes + rs.randint(-2, 3, boxes.shape).astype(F32)
    props[vi["v65"], 3] = props[vi["v65"], 64]          # the two detections of one proposal
    # ---- class-max vectors: label 0 (wraps to the last slot) with the view's highest counted score, a label beyond the table with a
    # higher one still, and on the reference views a high score outside the sub-sample ----
    view_img = np.zeros(V, np.int32); view_isref = np.zeros(V, np.int32)
    for i, name in enumerate(("ref0", "ref1", "ref2")):
        view_img[vi[name]] = i; view_isref[vi[name]] = 1
    for img, name, _, _ in pairs:
        if not view_isref[vi[name]]:
            view_img[vi[name]] = img
    for v in range(V):
        n = int(count[v])
        if n < 3:
            continue
        live = list(ref_sel[view_img[v]][:ref_n[view_img[v]]]) if view_isref[v] else list(range(n))
        if len(live) >= 2:
            labels[v, live[-1]] = 0; scores[v, live[-1]] = 0.97
            labels[v, live[-2]] = C + 3; scores[v, live[-2]] = 0.99
        if view_isref[v]:
            out = [k for k in range(n) if k not in live][0]
            labels[v, out] = 5; scores[v, out] = 0.98
    P = len(pairs)
    case = dict(V=V, cap=CAP, C=C, n_img=n_img, P=P, bp=1.3, boxes=boxes, props=props, scores=scores, labels=labels, scores_cls=scls, prob_max=pm,
                count=count, view_img=view_img, view_isref=view_isref, ref_sel=ref_sel, ref_n=ref_n,
                ref_view=np.array([p[0] for p in pairs], np.int32), aug_view=np.array([vi[p[1]] for p in pairs], np.int32),
                pair_img=np.array([p[0] for p in pairs], np.int32), aug_kind=np.array([p[2] for p in pairs], np.int32),
                aug_param=np.stack([par(*(p[0], p[2], p[3])) for p in pairs]).astype(F32), ties=ties, pairs=pairs, vi=vi)
    return case


# ---------------------------------------------------------------------------------------------------------------------------
# lt_uncertainty_kernel: six views, the minimum moved from call to call
# ---------------------------------------------------------------------------------------------------------------------------
LT_COUNTS = [0, 1, 255, 256, 257, 600]
LT_TURNS = [0, 255, 256, -1]           # where the minimum sits (-1: the last detection); clipped to the view


def lt_case(turn):
    """Background detections miss their proposals (IoU 0, |0 + 0.25 - 1| = 0.75).  Detections 1..4 of a view with room for them: equal to
    the proposal (calcu_iou 651 / 589 > 1), an overlap width of exactly 0, of exactly 1, a NaN prob_max.  The minimum: a proposal one
    pixel off, 2400 / 2480, with a prob_max that differs from view to view."""
    V, cap = len(LT_COUNTS), 600
    rs = np.random.RandomState(7)
    boxes = _rand_boxes(rs, V * cap, 0, 0, 500, 500).reshape(V, cap, 4)
    props = boxes + F32(1000)
    pm = np.full((V, cap), 0.25, F32)
    where = []
    for v, n in enumerate(LT_COUNTS):
        if n >= 6:
            boxes[v, 1] = props[v, 1] = [10, 10, 30, 40]; pm[v, 1] = 0.1
            boxes[v, 2] = [10, 10, 30, 40]; props[v, 2] = [31, 10, 50, 40]; pm[v, 2] = 0.3
            boxes[v, 3] = [10, 10, 30, 40]; props[v, 3] = [30, 10, 50, 40]; pm[v, 3] = 0.5
            boxes[v, 4] = props[v, 4] = [10, 10, 30, 40]; pm[v, 4] = np.nan
        if n:
            k = n - 1 if turn < 0 else min(turn, n - 1)
            boxes[v, k] = [100, 100, 140, 160]; props[v, k] = [101, 101, 141, 161]; pm[v, k] = 0.03 + 0.001 * v
            where.append(k)
    z = np.zeros(V, np.int32)
    return dict(V=V, cap=cap, C=2, n_img=1, P=0, bp=1.3, boxes=boxes, props=props.astype(F32), scores=np.zeros((V, cap), F32),
                labels=np.ones((V, cap), np.int64), scores_cls=np.full((V, cap, 2), 0.5, F32), prob_max=pm, count=np.array(LT_COUNTS, np.int32),
                view_img=z, view_isref=z.copy(), ref_sel=np.zeros((1, 50), np.int32), ref_n=np.zeros(1, np.int32),
                ref_view=np.zeros(1, np.int32), aug_view=np.zeros(1, np.int32), pair_img=np.zeros(1, np.int32), aug_kind=np.zeros(1, np.int32),
                aug_param=np.zeros((1, 12), F32), where=where)


# ---------------------------------------------------------------------------------------------------------------------------
# ls_c tail: a reference view's boxes and prob_max, six noisy views
# ---------------------------------------------------------------------------------------------------------------------------
def ls_cases():
    rs = np.random.RandomState(11)
    cases = []
    def add(name, pm):
        n = len(pm)
        ref = _rand_boxes(rs, n, 0, 0, 300, 300, 20, 80)
        views = [_jitter(rs, ref[rs.permutation(n)[:max(1, n - k)]]) if n else np.zeros((0, 4), F32) for k in range(6)]
        views[3] = np.zeros((0, 4), F32)                                       # an empty noisy view: an all-zero row
        cases.append(dict(name=name, pm=np.asarray(pm, F32), ref=ref, views=views))
    for n in (0, 1, 7, 8, 9, 29, 30, 31, 100):
        add("n%d" % n, rs.permutation(n) / F32(max(n, 1)) * F32(0.9) + F32(0.05))
    pm = (np.arange(40)[::-1] / F32(64)).astype(F32)[rs.permutation(40)]       # distinct values ...
    order = np.argsort(-pm, kind="stable")
    pm[order[28:31]] = pm[order[29]]                                           # ... but for ranks 29..31: two of the three are taken
    add("ties_across_rank_30", pm)
    add("all_equal", np.full(50, 0.625, F32))
    return cases
