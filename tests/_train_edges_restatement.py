"""Plain numpy / torch-CPU restatements and the case tables of the training front end, target and loss kernels at their edges (test
infrastructure): Matcher and box_iou of torchvision 0.8.2 in numpy float32, its AnchorGenerator for the two anchor sets the trainers use,
and the inputs of the max-pool, preprocess, BoxCoder, RoI gather and plain focal-loss tests.  tests/test_train_edges.py pins the
restatements to live torch and to the recorded reference (tests/golden/train_losses.npz) and takes the census of the tables on the CPU;
tests/test_gpu_train_edges.py runs the HIP kernels against them.

Every restated rule takes the one-line mistakes a kernel could make as switches (``first_max``, ``below``, ``restore``, ``stride``): the CPU
tests apply each to the restatement and assert that the tables tell it from the correct rule."""
import numpy as np
import torch

SENTINEL = 12345.0

# ---- Matcher -----------------------------------------------------------------------------------------------------------------------
THRESHOLDS = ((0.7, 0.3), (0.5, 0.4))          # the RPN's and RetinaNet's (hi, lo), both with low-quality matches
MATCH_MODES = ((0.7, 0.3, True), (0.5, 0.4, True), (0.5, 0.5, False), (0.7, 0.3, False), (0.5, 0.4, False))


def box_iou_np(gt, boxes):
    """torchvision.ops.box_iou in float32, [n_gt, n_boxes]; the operation order of oracle.torch_train.box_iou"""
    a, b = np.asarray(gt, np.float32), np.asarray(boxes, np.float32)
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]); area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(a[:, None, :2], b[None, :, :2]); rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.maximum(rb - lt, np.float32(0))
    inter = wh[:, :, 0] * wh[:, :, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / ((area1[:, None] + area2[None, :]) - inter)).astype(np.float32)


def matcher_np(iou, hi, lo, allow_low, first_max=">", below="<", restore="all"):
    """det_utils.Matcher of torchvision 0.8.2 on a float32 [n_gt, n_boxes] matrix -> int64 [n_boxes].
    The mistakes: first_max ">=" (the LAST of equal maxima wins); below "<=" (an IoU equal to a threshold falls into the lower class);
    restore "positive" (a ground truth that overlaps nothing restores nobody: the rule repaired), "first" (only the first of the candidates
    that share a ground truth's best IoU is restored)."""
    iou = np.asarray(iou, np.float32)
    hi, lo = np.float32(hi), np.float32(lo)
    nG, nB = iou.shape
    best = np.full(nB, -1.0, np.float32); arg = np.zeros(nB, np.int64)
    for g in range(nG):
        take = iou[g] >= best if first_max == ">=" else iou[g] > best
        best = np.where(take, iou[g], best); arg = np.where(take, g, arg)
    under = (lambda v, t: v <= t) if below == "<=" else (lambda v, t: v < t)
    m = arg.copy()
    m[under(best, hi)] = -2
    m[under(best, lo)] = -1
    if allow_low:
        gtmax = iou.max(axis=1)
        eq = iou == gtmax[:, None]
        if restore == "positive":
            eq &= iou > 0
        elif restore == "first":
            first = np.zeros_like(eq)
            first[np.arange(nG), eq.argmax(axis=1)] = True
            eq &= first
        upd = eq.any(axis=0)
        m[upd] = arg[upd]
    return m


MATCH_MISTAKES = (dict(first_max=">="), dict(below="<="), dict(restore="positive"), dict(restore="first"))

DESIGNED_BOXES = [[0, 0, 10, 10], [0, 0, 10, 7], [0, 0, 10, 3], [0, 0, 5, 10], [0, 0, 4, 10], [20, 20, 30, 30], [0, 0, 10, 6.9], [0, 0, 10, 2.9],
                  [40, 40, 50, 50], [40, 40, 50, 47], [41, 40, 51, 50], [39, 40, 49, 50]]
DESIGNED_GT = [[0, 0, 10, 10], [0, 0, 10, 10], [40, 40, 50, 49]]
DESIGNED_EXPECT = {(0.7, 0.3, True): [0, 0, -2, -2, -2, -1, -2, -1, 2, 2, 2, 2],
                   (0.5, 0.4, True): [0, 0, -1, 0, -2, -1, 0, -1, 2, 2, 2, 2],
                   (0.5, 0.5, False): [0, 0, -1, 0, -1, -1, 0, -1, 2, 2, 2, 2]}
LONELY_GT = [100, 100, 110, 110]                # overlaps nothing: with (0.7, 0.3, low) it "matches" every candidate at IoU 0
LONELY_EXPECT = [0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2]
# the extension, integer boxes: two ground truths whose best IoU is shared by two candidates each -- 0.4 (inside (0.7, 0.3)'s band, equal to
# (0.5, 0.4)'s lo) and 0.2 (below both lo) -- so a restored match is seen to come from -2 and from -1; a candidate that beats neither
EXTRA_BOXES = [[60, 0, 70, 4], [60, 6, 70, 10], [80, 0, 90, 2], [80, 8, 90, 10], [60, 0, 70, 3], [80, 0, 90, 1]]
EXTRA_GT = [[60, 0, 70, 10], [80, 0, 90, 10]]


def designed_table(extended=False, lonely=False):
    boxes = DESIGNED_BOXES + (EXTRA_BOXES if extended else [])
    gt = DESIGNED_GT + (EXTRA_GT if extended else []) + ([LONELY_GT] if lonely else [])
    return np.asarray(gt, np.float32), np.asarray(boxes, np.float32)


MATCH_N_BOXES = (1, 255, 256, 257, 513)
MATCH_N_GT = (1, 2, 3, 65)
MATCH_SEED = 3


def random_match_case(n_boxes, n_gt, seed=MATCH_SEED):
    """Integer boxes on a 64 x 64 canvas, sides 2..12: ground truths anywhere, candidates half anywhere and half a ground truth moved or
    resized by -2..2 pixels per edge, so equal IoUs and IoUs equal to a threshold (7/10, 1/2, 2/5, 3/10 of small integers) are common."""
    rs = np.random.RandomState(seed * 100003 + n_boxes * 131 + n_gt)

    def rnd(n):
        wh = rs.randint(2, 13, (n, 2)); xy = np.stack([rs.randint(0, 65 - wh[:, 0]), rs.randint(0, 65 - wh[:, 1])], axis=1)
        return np.concatenate([xy, xy + wh], axis=1)

    def moved(src, n, d):
        b = src[rs.randint(0, len(src), n)] + rs.randint(-d, d + 1, (n, 4))
        b = np.clip(b, 0, 64)
        b[:, :2] = np.minimum(b[:, :2], 63)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        return b
    gt = rnd(n_gt)
    if n_gt > 1:                                   # the later half: earlier ground truths moved by -1..1 (crowds; some exact duplicates)
        h = (n_gt + 1) // 2
        gt[h:] = moved(gt[:h], n_gt - h, 1)
    boxes = rnd(n_boxes)
    near = moved(gt, n_boxes, 2)
    pick = rs.rand(n_boxes) < 0.5
    boxes[pick] = near[pick]
    return gt.astype(np.float32), boxes.astype(np.float32)


def match_census(gt, boxes, hi, lo):
    """What a table holds for one threshold pair (conditions on the INPUT; nothing here looks at a kernel's output)."""
    iou = box_iou_np(gt, boxes)
    hi32, lo32 = np.float32(hi), np.float32(lo)
    best = iou.max(axis=0); gtmax = iou.max(axis=1)
    n_best = (iou == best[None, :]).sum(axis=0)               # ground truths that share candidate j's best IoU
    shared = iou == gtmax[:, None]
    n_shared = shared.sum(axis=1)                              # candidates that share ground truth g's best IoU
    band = (best >= lo32) & (best < hi32)
    restored = shared.any(axis=0)
    return dict(iou_eq_hi=bool((iou == hi32).any()), iou_eq_lo=bool((iou == lo32).any()),
                best_eq_hi=bool((best == hi32).any()), best_eq_lo=bool((best == lo32).any()),
                cand_tie=bool(((n_best >= 2) & (best > 0)).any()),
                # such a tie where the two rules differ in the OUTPUT: the candidate's match survives the thresholds or is restored
                cand_tie_kept=bool(((n_best >= 2) & (best > 0) & ((best >= hi32) | restored)).any()),
                gt_tie=bool(((n_shared >= 2) & (gtmax > 0)).any()),
                gt_tie_below_hi=bool(((n_shared >= 2) & (gtmax > 0) & (gtmax < hi32)).any()),
                band_restored=bool((band & restored).any()), band_stays=bool((band & ~restored).any()),
                below_restored=bool(((best < lo32) & restored & (best > 0)).any()),
                gt_without_overlap=bool((gtmax == 0).any()))


# ---- AnchorGenerator ---------------------------------------------------------------------------------------------------------------
RATIOS = (0.5, 1.0, 2.0)


def anchor_sizes(kind):
    """kind 0: ((32,), (64,), ..., (512,)) (frcnn); kind 1: (x, int(x 2^(1/3)), int(x 2^(2/3))) for the same five (retinanet)"""
    return [(float(x),) if kind == 0 else (float(x), float(int(x * 2 ** (1.0 / 3))), float(int(x * 2 ** (2.0 / 3)))) for x in (32, 64, 128, 256, 512)]


def base_anchors_np(sizes, ratios=RATIOS):
    """AnchorGenerator.generate_anchors in float32: index = ratio * len(sizes) + size; round half to even, as torch.round"""
    s, r = np.asarray(sizes, np.float32), np.asarray(ratios, np.float32)
    h_r = np.sqrt(r); w_r = np.float32(1) / h_r
    ws = (w_r[:, None] * s[None, :]).reshape(-1); hs = (h_r[:, None] * s[None, :]).reshape(-1)
    return np.round(np.stack([-ws, -hs, ws, hs], axis=1) / np.float32(2)).astype(np.float32)


def anchors_np(kind, Hp, Wp, level_hw, stride="floor"):
    """AnchorGenerator.grid_anchors of one padded image: strides (Hp // Hl, Wp // Wl) per level and AXIS, order (level, y, x, anchor).
    The mistakes: stride "fixed" (the nominal 4 << l, 8 << l for kind 1), "square" (the row stride used for both axes), "ceil" (the quotient rounded up)."""
    out = []
    for l, ((h, w), sizes) in enumerate(zip(level_hw, anchor_sizes(kind))):
        sy, sx = Hp // h, Wp // w
        if stride == "fixed":
            sy = sx = (8 if kind else 4) << l
        elif stride == "square":
            sx = sy
        elif stride == "ceil":
            sy, sx = -(-Hp // h), -(-Wp // w)
        ys, xs = np.meshgrid(np.arange(h, dtype=np.int64) * sy, np.arange(w, dtype=np.int64) * sx, indexing="ij")
        shifts = np.stack([xs, ys, xs, ys], axis=-1).reshape(-1, 1, 4).astype(np.float32)
        out.append((shifts + base_anchors_np(sizes)[None]).reshape(-1, 4))
    return np.concatenate(out).astype(np.float32)


ANCHOR_PAD = (96, 160)
# (kind, Hp, Wp, level_hw): the two uneven pyramids of a 96 x 160 batch (last levels: strides 48 / 53, and 96 / 80), one divisible shape per
# kind, and a coarsest level of one pixel
ANCHOR_CASES = [(0, 96, 160, [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]),
                (1, 96, 160, [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]),
                (0, 64, 128, [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]),
                (1, 128, 128, [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]),
                (0, 32, 32, [(8, 8), (4, 4), (2, 2), (1, 1), (1, 1)])]


# ---- max-pool / LastLevelMaxPool ---------------------------------------------------------------------------------------------------
POOL_HW = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (2, 5), (5, 2), (7, 9), (8, 8), (17, 23))
POOL_C = (4, 64, 256)
POOL_N = (1, 3)
POOL_KINDS = ("gaussian", "negative", "neg_inf", "nan")


def pool_input(kind, N, H, W, C, seed=0):
    """[N, H, W, C] float32.  negative: every value <= -0.5; neg_inf: one pixel (all channels) of every image -inf; nan: one NaN pixel in the
    interior (H // 2, W // 2) and one on the border (0, W - 1) of every image (on maps of one or two pixels the two may be the same)."""
    rs = np.random.RandomState(seed + 7 * H + 131 * W + 17 * C + N)
    x = rs.randn(N, H, W, C).astype(np.float32)
    if kind == "negative":
        x = -np.abs(x) - np.float32(0.5)
    elif kind == "neg_inf":
        x[:, H // 2, (W - 1) // 2, :] = -np.inf
    elif kind == "nan":
        x[:, H // 2, W // 2, :] = np.nan
        x[:, 0, W - 1, 0::2] = np.nan
    return x


def pool_ref(x, window3, pad_value=None):
    """live torch CPU max_pool2d(3, 2, 1) / max_pool2d(1, 2, 0) of an NHWC array; pad_value: the mistake of a border padded with a number"""
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)
    if not window3:
        y = F.max_pool2d(t, 1, 2, 0)
    elif pad_value is None:
        y = F.max_pool2d(t, 3, 2, 1)
    else:
        y = F.max_pool2d(F.pad(t, (1, 1, 1, 1), value=pad_value), 3, 2, 0)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# ---- preprocess --------------------------------------------------------------------------------------------------------------------
# (min_size, max_size, source (H, W) of the three images, index of the image that carries a remainder tensor or None)
PREPROCESS_BATCHES = [(32, 64, ((1, 1), (2, 3), (7, 9)), None),            # up-scaling
                      (31, 40, ((33, 31), (150, 210), (7, 9)), None),      # ratio 1; down-scaling decided by the max_size clamp; up-scaling
                      (20, 30, ((33, 31), (2, 3), (1, 1)), 0),             # a remainder on the first image only
                      (48, 200, ((150, 210), (33, 31), (7, 9)), 1)]        # down-scaling decided by min_size; a remainder on the second


def preprocess_images(sizes, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]


def preprocess_remainder(h, w, seed=0):
    """[3, H, W] float32 in [0, 1/255): what a float input leaves above the uint8 grid"""
    return (np.random.RandomState(1000 + seed).rand(3, h, w) * (0.999 / 255.0)).astype(np.float32)


def preprocess_want(orc, images, min_size, max_size, remainders, Hp, Wp):
    """oracle.preprocess_view per image, embedded at the top left of [N][Hp][Wp][4] zeros; also returns the (Hr, Wr) list"""
    out = np.zeros((len(images), Hp, Wp, 4), np.float32)
    sizes = []
    for i, im in enumerate(images):
        v, (Hr, Wr, _, _) = orc.preprocess_view(im, min_size, max_size, noise=remainders[i] if remainders else None)
        assert not v[Hr:].any() and not v[:, Wr:].any() and not v[..., 3].any()
        out[i, :Hr, :Wr] = v[:Hr, :Wr]
        sizes.append((Hr, Wr))
    return out, sizes


# ---- BoxCoder.encode ---------------------------------------------------------------------------------------------------------------
ENCODE_N = (1, 255, 256, 257)
ENCODE_WEIGHTS = ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0))
ENCODE_SPECIAL = ("same", "wide_ref", "wide_prop", "zero_width_ref")


def encode_rows(n, seed=0):
    """(reference, proposals, kind) of n rows.  Rows 0..3 and the last four of 257 (so both sides of the 256-thread boundary) are: reference
    == proposal; a 1000 : 1 width ratio either way; a reference of width 0 (log 0 = -inf in column 2).  n = 1 keeps row 0 only."""
    rs = np.random.RandomState(40 + seed)
    full = 257
    xy = rs.rand(full, 2).astype(np.float32) * 200; wh = (rs.rand(full, 2) * 90 + 4).astype(np.float32)
    prop = np.concatenate([xy, xy + wh], axis=1)
    ref = prop + (rs.randn(full, 4) * 6).astype(np.float32)
    ref[:, 2:] = np.maximum(ref[:, 2:], ref[:, :2] + 1)
    kind = np.full(full, -1)
    for k, r in enumerate((0, 1, 2, 3)):
        kind[r] = k
    for k, r in enumerate((253, 254, 255, 256)):
        kind[r] = k
    for r in np.flatnonzero(kind >= 0):
        x, y = np.float32(rs.randint(0, 100)), np.float32(rs.randint(0, 100))
        if kind[r] == 0:
            ref[r] = prop[r]
        elif kind[r] == 1:
            ref[r] = [x, y, x + 1000, y + 20]; prop[r] = [x + 3, y, x + 4, y + 25]
        elif kind[r] == 2:
            ref[r] = [x + 3, y, x + 4, y + 25]; prop[r] = [x, y, x + 1000, y + 20]
        else:
            ref[r] = [x + 5, y, x + 5, y + 30]; prop[r] = [x, y, x + 12, y + 20]
    return ref[:n].copy(), prop[:n].copy(), kind[:n].copy()


# ---- RoI gather --------------------------------------------------------------------------------------------------------------------
# name -> (slots, used proposal slots, n_gt, batch, fraction of proposal rows matched to a ground truth)
ROI_CASES = {"no_foreground": ([20], [20], [0], 8, 0.0),
             "R_equals_cap": ([40, 40], [40, 33], [2, 3], 16, 0.3),
             "R_1": ([1], [0], [1], 4, 0.0),
             "R_255": ([400], [400], [4], 255, 0.3),
             "R_257": ([300, 60], [300, 55], [5, 7], 200, 0.3),      # the second image runs out of candidates: 200 + 57 < cap
             "image_without_gt": ([50, 50, 50], [50, 43, 50], [3, 0, 2], 16, 0.3)}
ROI_PRED_LD, ROI_CLASSES = 108, 21


def roi_case(ops, name):
    """The sampler's own int64 block (train_ops.roi_sample_host, host code) over a random candidate table.  Returns a dict with the table
    [T, 4], the ground truths + the extra all-zero row [G + 1, 4], the block, cap, R, n_pos, per-image counts."""
    slots, used, n_gt, batch, frac = ROI_CASES[name]
    rs = np.random.RandomState(sum(ord(ch) for ch in name))
    rows = [s + g for s, g in zip(slots, n_gt)]
    T_ = sum(rows)
    xy = rs.rand(T_, 2).astype(np.float32) * 300
    table = np.concatenate([xy, xy + 5 + rs.rand(T_, 2).astype(np.float32) * 120], axis=1)
    g_xy = rs.rand(sum(n_gt) + 1, 2).astype(np.float32) * 300
    gts = np.concatenate([g_xy, g_xy + 20 + rs.rand(len(g_xy), 2).astype(np.float32) * 100], axis=1)
    gts[-1] = 0
    matched = []
    for s, g in zip(slots, n_gt):
        m = np.where(rs.rand(s) < frac, rs.randint(0, max(g, 1), s), np.where(rs.rand(s) < 0.1, -2, -1)).astype(np.int32) if g else np.full(s, -1, np.int32)
        matched.append(np.concatenate([m, np.arange(g, dtype=np.int32)]))      # a ground-truth row matches itself
    matched = np.concatenate(matched)
    gt_labels = np.concatenate([rs.randint(1, ROI_CLASSES, g).astype(np.int64) for g in n_gt] + [np.zeros(1, np.int64)])
    blk, cap, R, n_pos, per = ops.roi_sample_host(slots, n_gt, used, matched, gt_labels, rs.rand(T_), batch, 0.25, ROI_PRED_LD, ROI_CLASSES)
    return dict(table=table, gts=gts, blk=blk, cap=cap, R=R, n_pos=n_pos, per=per, n_gt=n_gt, slots=slots, matched=matched, gt_labels=gt_labels)


def roi_want(c, weights):
    """numpy gathers of the block + oracle.torch_train.encode in float64: (rois [R, 5] float32, targets [n_pos, 4] float64)"""
    from oracle import torch_train as tt
    blk, cap, R, n_pos = c["blk"], c["cap"], c["R"], c["n_pos"]
    keep, gsel, pos = blk[:R], blk[cap:cap + R], blk[4 * cap:4 * cap + n_pos]
    img = blk[5 * cap:].view(np.float32)[:R]
    rois = np.concatenate([img[:, None], c["table"][keep]], axis=1).astype(np.float32)
    tgt = tt.encode(torch.from_numpy(c["gts"][gsel[pos]]).double(), torch.from_numpy(c["table"][keep[pos]]).double(), weights)
    return rois, tgt.reshape(n_pos, 4)


# ---- plain focal loss --------------------------------------------------------------------------------------------------------------
# tests/test_gpu_retina_ll_ops.py's SHAPES restated (test_train_edges.py asserts the two tables equal): (A, K, ld, level_pix)
FOCAL_SHAPES = [(9, 3, 28, [6, 2, 1, 1, 1]), (1, 1, 4, [249, 3, 2, 1, 1]), (1, 1, 4, [250, 3, 2, 1, 1]), (1, 1, 4, [505, 3, 2, 1, 1]),
                (1, 1, 4, [506, 3, 2, 1, 1]), (9, 20, 180, [640, 160, 40, 12, 4]), (9, 91, 820, [6, 2, 1, 1, 1])]
# 257 and 513 anchors per image with several classes and anchors per pixel would not divide: one anchor per pixel, three classes
FOCAL_STRADDLE = (1, 3, 4, [250, 3, 2, 1, 1])       # A_tot = 257: with N = 2 block 1 holds the last anchor of image 0 and 255 of image 1


def focal_blocks(flat, N, level_pix, ld):
    out, o = [], 0
    for n in level_pix:
        out.append(flat[o:o + N * n * ld].view(N, n, ld)); o += N * n * ld
    return out


def focal_case(A, K, ld, level_pix, N=3, seed=0, pow2=False):
    """The planted case of test_gpu_retina_ll_ops._case: logits gaussian * 3 with 0, -0, +-30 planted, NaN in the pad columns.
    pow2 False: image 0 all background, image 1 all ignored, image 2.. mixed with a foreground anchor first and last.
    pow2 True: every image mixed, image n with exactly 2^(n+1) foreground anchors (its first and its last among them, with different
    classes where K > 1), so every max(1, #fg) is a power of two."""
    g = torch.Generator().manual_seed(seed)
    At = A * sum(level_pix)
    flat = torch.full((N * sum(level_pix) * ld,), float("nan"))
    for b in focal_blocks(flat, N, level_pix, ld):
        b[:, :, :A * K] = torch.randn(b.shape[0], b.shape[1], A * K, generator=g) * 3
    first = focal_blocks(flat, N, level_pix, ld)[0]
    for i in range(N):
        for j, v in enumerate((0.0, -0.0, 30.0, -30.0, 30.0)[:first.shape[1]]):
            first[i, j, 0 if j < 4 else A * K - 1] = v
    n_gt = ([2, 1] + [3] * (N - 2))[:N] if not pow2 else [3] * N
    gt_off = np.cumsum([0] + n_gt)
    gt_labels = torch.randint(0, K, (int(gt_off[-1]),), generator=g, dtype=torch.int64)
    if pow2 and K > 1:
        for i in range(N):
            gt_labels[gt_off[i] + 1], gt_labels[gt_off[i] + 2] = i % K, (i + 1) % K
    matched = torch.full((N, At), -1, dtype=torch.int32)
    if pow2:
        for i in range(N):
            matched[i] = torch.randint(-2, 0, (At,), generator=g, dtype=torch.int32)
            want = 2 ** (i + 1)
            inner = 1 + torch.randperm(At - 2, generator=g)[:want - 2]
            matched[i, inner] = torch.randint(0, 3, (want - 2,), generator=g, dtype=torch.int32)
            matched[i, 0], matched[i, At - 1] = 1, 2
    else:
        if N > 1:
            matched[1] = -2
        for i in range(2, N):
            matched[i] = torch.randint(-2, 3, (At,), generator=g, dtype=torch.int32)
            matched[i, 0], matched[i, At - 1] = 1, 2
    nfg = [int((matched[i] >= 0).sum()) for i in range(N)]
    return dict(flat=flat, matched=matched, gt_labels=gt_labels, gt_off=torch.from_numpy(gt_off.astype(np.int32)), nfg=nfg,
                denom=[float(max(1, n)) for n in nfg], N=N, A=A, K=K, ld=ld, level_pix=list(level_pix), At=At)


def focal_image_logits(flat, c, i):
    return torch.cat([b[i, :, :c["A"] * c["K"]].reshape(-1, c["K"]) for b in focal_blocks(flat, c["N"], c["level_pix"], c["ld"])])


def focal_want(c, gscale=1.0, image_of=None):
    """float64: mean over images of sigmoid_focal_loss_sum / max(1, #fg) and gscale times its gradient with respect to the flat buffer (0 in
    the pad columns).  image_of: the mistake of an image index taken per 256-thread block -- a function (n, anchor) -> the image whose
    weight and labels the anchor is given."""
    from oracle import torch_train as tt
    fd = c["flat"].double().requires_grad_(True)
    total = 0.0
    for i in range(c["N"]):
        logits = focal_image_logits(fd, c, i)
        m = c["matched"][i].long()
        fg, valid = m >= 0, m != -2
        src = torch.full((c["At"],), i, dtype=torch.int64) if image_of is None else torch.tensor([image_of(i, a) for a in range(c["At"])])
        tgt = torch.zeros_like(logits)
        tgt[fg, c["gt_labels"][c["gt_off"].long()[src[fg]] + m[fg]]] = 1.0
        w = torch.tensor([1.0 / (c["denom"][int(s)] * c["N"]) for s in src], dtype=torch.float64)
        x, t = logits[valid], tgt[valid]
        p = torch.sigmoid(x)
        ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
        p_t = p * t + (1 - p) * (1 - t)
        per = (0.25 * t + 0.75 * (1 - t)) * ce * (1 - p_t) ** 2
        if image_of is None:                              # the project's own float64 formula, summed: the reference proper
            total = total + tt.sigmoid_focal_loss_sum(x, t) / c["denom"][i] / c["N"]
        else:
            total = total + (per.sum(dim=1) * w[valid]).sum()
    (gscale * total).backward()
    return total.detach().reshape(1), torch.nan_to_num(fd.grad)


def block_image(c):
    """the mistake: the image of the block's FIRST thread, for every thread of a 256-thread block of the flat (image, anchor) index"""
    return lambda n, a: ((n * c["At"] + a) // 256 * 256) // c["At"]
