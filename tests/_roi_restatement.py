"""Plain numpy restatement of the inference RoIAlign stage (cald_amd/csrc/roi.hip with roi_level / roi_sample of kernels.h and the
split store of h16.h): float32 arithmetic in the operation order the kernels state, every decision written out.  No GPU, no library,
no oracle.

Three things are restated:
  * the values: roi_level (with the fixed polynomial logarithm of common.h, its fused multiply-adds emulated exactly), roi_sample,
    the four weight products and the accumulation in the oracle's order (evaluate), the same in float64 on the float32 sample
    positions and weights (evaluate_f64), the processing order (roi_order) and the split form (split_words / join);
  * the control flow of the row walk (roi_rows_walk) on pixel INDICES: walk_plan replays the row pattern choice, plo / phi and the
    copy / load / alias steps of the four pixel-column slots and returns, for every (bin, sample, corner), the (row, column) whose
    pixel the walk multiplies -- the gather kernel's indices whenever the walk is right (a column of -1 stands for a slot that still
    holds its initial zeros);
  * what a set of RoIs reaches of that control flow (census).

`wrong` names deliberately wrong variants (WRONG below).  They exist so that the tests can assert that the constructed cases would
notice each of those mistakes; the product is compared with wrong = () only.
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
ROI_CAP = 1000
WRONG = ("valid_ge",            # a sample at exactly t == size counts as outside
         "no_min_size",         # rw / rh not raised to 1
         "clamp_keeps_tt",      # the right / bottom clamp leaves tt (and so the weights) as it was
         "weights_swapped",     # lo takes the weight of hi
         "no_level_eps",        # the 1e-6 of the level formula dropped
         "l0_ignores_phi",      # L0 found in the previous bin: always copied from L1, also where c0l == phi
         "l1_alias_l0",         # L1 shared inside the bin: always copied from L0, also where it is H0's column
         "h1_alias_l1",         # H1 shared inside the bin: copied from L1 where it is H0's column
         "pat1_rows01",         # pattern 1: the second sample row reads pixel-row registers (0, 1)
         "pat2_on_r0",          # pattern 2 chosen on r2 == r0 alone
         "split_lo_from_x")     # the split form's lo half taken from x - hi instead of 16 x - hi

SLOTS = ("L0", "H0", "L1", "H1")
# per slot, the ways roi_rows_walk can fill it, in the order the code tests them
DECISIONS = {"L0": ("copy_L1", "copy_H1", "load"),
             "H0": ("alias_L0", "copy_H1", "copy_L1", "load"),
             "L1": ("alias_L0", "alias_H0", "load"),
             "H1": ("alias_L1", "alias_H0", "alias_L0", "load")}
# dead while valid samples are monotone along the axis and an invalid one is (0, 0): never reached by any profile
UNREACHABLE = {("H0", "copy_L1"), ("H1", "alias_L0")}


def reachable_triples():
    """every (slot, decision, pw) that can occur: nothing of the previous bin at pw == 0, the two dead decisions nowhere"""
    out = set()
    for s in SLOTS:
        for d in DECISIONS[s]:
            if (s, d) in UNREACHABLE:
                continue
            for pw in range(7):
                if pw == 0 and d.startswith("copy_"):
                    continue
                out.add((s, d, pw))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# roi_level: floor((4 + det_log2f(sqrt(area) / 224)) + 1e-6) clamped to 2..5, in float32
# ---------------------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """float32 fused multiply-add, exactly: the product of two float32 is exact in float64; the float64 sum is forced to round-to-odd
    (one ulp towards the discarded part when its last bit is even), after which the rounding to float32 is the single correct one"""
    p = float(a) * float(b)
    c = float(c)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    if e != 0.0 and math.isfinite(s):
        m, _ = math.frexp(s)
        if int(m * 9007199254740992.0) % 2 == 0:
            s = math.nextafter(s, math.inf if e > 0 else -math.inf)
    return F32(s)


def _bits(x):
    return int(np.array(x, F32).view(np.uint32))


def _from_bits(u):
    return np.array(u, np.uint32).view(F32)[()]


def det_logf(x):
    """common.h det_logf"""
    x = F32(x)
    if x != x:
        return x
    if x < 0:
        return F32(np.nan)
    if x == 0:
        return F32(-np.inf)
    if x == F32(np.inf):
        return x
    e = 0
    u = _bits(x)
    if u < 0x00800000:
        x = F32(x * F32(8388608.0)); u = _bits(x); e = -23
    e += (u >> 23) - 126
    m = _from_bits((u & 0x007fffff) | 0x3f000000)
    if m < F32(0.70710678):
        e -= 1; f = F32(F32(m + m) - F32(1.0))
    else:
        f = F32(m - F32(1.0))
    z = F32(f * f)
    p = F32(7.0376836292e-2)
    for k in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1,
              3.3333331174e-1):
        p = fmaf(p, f, F32(k))
    y = F32(F32(p * f) * z)
    fe = F32(e)
    y = fmaf(fe, F32(-2.12194440e-4), y)
    y = fmaf(z, F32(-0.5), y)
    r = F32(f + y)
    return fmaf(fe, F32(0.693359375), r)


def roi_level(box, wrong=()):
    """kernels.h roi_level: 0..3 for P2..P5.  A negative area gives NaN and so level 0, a zero one -inf and level 0."""
    b = [F32(v) for v in box]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        area = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
        s = np.sqrt(area, dtype=F32)
        k = F32(F32(4.0) + F32(det_logf(F32(s / F32(224.0))) * F32(1.44269504)))
        if "no_level_eps" not in wrong:
            k = F32(k + F32(1e-6))
        k = np.floor(k)
    if not k >= 2.0:
        k = 2.0
    if k > 5.0:
        k = 5.0
    return int(k) - 2


# ---------------------------------------------------------------------------------------------------------------------------
# samples
# ---------------------------------------------------------------------------------------------------------------------------
def roi_sample(start, bin_, p, i, size, wrong=()):
    """kernels.h roi_sample, operation by operation: (lo, hi, l, h, valid)"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = F32(F32(start + F32(F32(p) * bin_)) + F32(F32(F32(F32(i) + F32(0.5)) * bin_) / F32(2.0)))
    valid = not (t < F32(-1.0) or (t >= F32(size) if "valid_ge" in wrong else t > F32(size)))
    tt = F32(0.0) if t <= F32(0.0) else t
    lo = int(min(float(tt), 2147483647.0)) if tt == tt else 0            # the conversion saturates
    if lo >= size - 1:
        hi = lo = size - 1
        if "clamp_keeps_tt" not in wrong:
            tt = F32(lo)
    else:
        hi = lo + 1
    with np.errstate(over="ignore", invalid="ignore"):
        l = F32(tt - F32(lo)); h = F32(F32(1.0) - l)
    if "weights_swapped" in wrong:
        l, h = h, l
    if not valid:
        lo = hi = 0
    return lo, hi, l, h, valid


def axis_samples(start, extent, size, wrong=()):
    """the 14 samples of one axis of a RoI that starts at `start` and is `extent` long, both in pixels of its map"""
    start, extent = F32(start), F32(extent)
    if "no_min_size" not in wrong and not extent >= F32(1.0):
        extent = F32(1.0)
    b = F32(extent / F32(7.0))
    return [roi_sample(start, b, k >> 1, k & 1, size, wrong) for k in range(14)]


def roi_setup(box, level_hw, wrong=()):
    """level, the 14 row samples and the 14 column samples of one box (the first 28 threads of either kernel)"""
    box = [F32(v) for v in box]
    l = roi_level(box, wrong)
    scale = F32(F32(1.0) / F32(4 << l))
    x1, y1, x2, y2 = [F32(v * scale) for v in box]
    return l, axis_samples(y1, F32(y2 - y1), level_hw[l][0], wrong), axis_samples(x1, F32(x2 - x1), level_hw[l][1], wrong)


def weights(sy, sx):
    """[49][4 samples (iy, ix)][4 corners] float32: w1 = hy hx, w2 = hy lx, w3 = ly hx, w4 = ly lx; zero unless both samples are valid"""
    w = np.zeros((49, 4, 4), F32)
    for ph in range(7):
        for pw in range(7):
            for iy in range(2):
                for ix in range(2):
                    Y, X = sy[2 * ph + iy], sx[2 * pw + ix]
                    if Y[4] and X[4]:
                        w[ph * 7 + pw, iy * 2 + ix] = [F32(Y[3] * X[3]), F32(Y[3] * X[2]), F32(Y[2] * X[3]), F32(Y[2] * X[2])]
    return w


def gather_plan(sy, sx):
    """(rows, cols) [49][4][4]: the pixels roi_align_kernel and the oracle multiply -- (yl, xl), (yl, xh), (yh, xl), (yh, xh), all zero
    unless both samples are valid"""
    rows = np.zeros((49, 4, 4), np.int64); cols = np.zeros((49, 4, 4), np.int64)
    for ph in range(7):
        for pw in range(7):
            for iy in range(2):
                for ix in range(2):
                    Y, X = sy[2 * ph + iy], sx[2 * pw + ix]
                    if Y[4] and X[4]:
                        rows[ph * 7 + pw, iy * 2 + ix] = [Y[0], Y[0], Y[1], Y[1]]
                        cols[ph * 7 + pw, iy * 2 + ix] = [X[0], X[1], X[0], X[1]]
    return rows, cols


# ---------------------------------------------------------------------------------------------------------------------------
# the row walk on indices
# ---------------------------------------------------------------------------------------------------------------------------
def row_pattern(Y0, Y1, wrong=()):
    """roi_align_rows_kernel's choice for one bin row and the pixel rows of the two sample rows: (pattern, (lo, hi) of sample row 0,
    (lo, hi) of sample row 1) as roi_rows_walk<pattern> reads them from its row registers"""
    r0, r1, r2, r3 = Y0[0], Y0[1], Y1[0], Y1[1]
    if r2 == r0 and (r3 == r1 or "pat2_on_r0" in wrong):
        pat = 2
    elif r2 == r1:
        pat = 1
    else:
        pat = 0
    regs = (r0, r1, r2 if pat == 0 else r3, r3)          # p0 .. p3; only the first NR = 4 / 3 / 2 are loaded
    second = {0: (2, 3), 1: (0, 1) if "pat1_rows01" in wrong else (1, 2), 2: (0, 1)}[pat]
    return pat, (regs[0], regs[1]), (regs[second[0]], regs[second[1]])


def column_walk(sx, wrong=()):
    """roi_rows_walk's seven steps over the 14 column samples: per bin the decision taken for each slot and the column each slot holds
    when the bin's arithmetic runs.  -> (decisions [7] of 4-tuples in SLOTS order, held [7] of (L0, H0, L1, H1) columns)"""
    L0 = H0 = L1 = H1 = -1                       # the registers start as zeros
    plo = phi = -1
    decisions, held = [], []
    for pw in range(7):
        c0l, c0h = sx[2 * pw][0], sx[2 * pw][1]
        c1l, c1h = sx[2 * pw + 1][0], sx[2 * pw + 1][1]
        d = {}
        # 1. what the previous bin already holds
        h0_alias = c0h == c0l
        l0_prev = c0l == plo or c0l == phi
        h0_prev = not h0_alias and (c0h == phi or c0h == plo)
        if l0_prev:
            if c0l == plo:
                L0 = L1; d["L0"] = "copy_L1"
            else:
                L0 = L1 if "l0_ignores_phi" in wrong else H1; d["L0"] = "copy_H1"
        if h0_prev:
            if c0h == phi:
                H0 = H1; d["H0"] = "copy_H1"
            else:
                H0 = L1; d["H0"] = "copy_L1"
        # 2. every column that has to come from memory
        l1_alias = c1l == c0l or c1l == c0h
        h1_alias = c1h == c1l or c1h == c0h or c1h == c0l
        if not l0_prev:
            L0 = c0l; d["L0"] = "load"
        if not h0_prev and not h0_alias:
            H0 = c0h; d["H0"] = "load"
        if not l1_alias:
            L1 = c1l; d["L1"] = "load"
        if not h1_alias:
            H1 = c1h; d["H1"] = "load"
        # 3. columns shared inside the bin
        if h0_alias:
            H0 = L0; d["H0"] = "alias_L0"
        if l1_alias:
            if c1l == c0l or "l1_alias_l0" in wrong:
                L1 = L0
            else:
                L1 = H0
            d["L1"] = "alias_L0" if c1l == c0l else "alias_H0"
        if h1_alias:
            if c1h == c1l:
                H1 = L1; d["H1"] = "alias_L1"
            elif c1h == c0h:
                H1 = L1 if "h1_alias_l1" in wrong else H0; d["H1"] = "alias_H0"
            else:
                H1 = L0; d["H1"] = "alias_L0"
        plo, phi = c1l, c1h
        decisions.append(tuple(d[s] for s in SLOTS))
        held.append((L0, H0, L1, H1))
    return decisions, held


def walk_plan(sy, sx, wrong=()):
    """(rows, cols) [49][4][4] as gather_plan gives them, but read off the replayed walk: what roi_align_rows_kernel multiplies with the
    weights of weights(sy, sx).  An invalid sample keeps the indices the walk holds for it (its weights are zero)."""
    rows = np.zeros((49, 4, 4), np.int64); cols = np.zeros((49, 4, 4), np.int64)
    _, held = column_walk(sx, wrong)
    for ph in range(7):
        _, first, second = row_pattern(sy[2 * ph], sy[2 * ph + 1], wrong)
        for pw in range(7):
            L0, H0, L1, H1 = held[pw]
            for iy, (rl, rh) in enumerate((first, second)):
                for ix, (cl, ch) in enumerate(((L0, H0), (L1, H1))):
                    rows[ph * 7 + pw, iy * 2 + ix] = [rl, rl, rh, rh]
                    cols[ph * 7 + pw, iy * 2 + ix] = [cl, ch, cl, ch]
    return rows, cols


def census(rois, level_hw, wrong=()):
    """what the RoIs reach of the walk: patterns {(pattern, ph)}, triples {(slot, decision, pw)}, tuples {4 decisions of a bin} and
    crossed {(pattern, slot, decision, pw)} -- every column decision is separate machine code in each pattern's instantiation"""
    seen = dict(patterns=set(), triples=set(), tuples=set(), crossed=set(), levels=set())
    for box in rois:
        l, sy, sx = roi_setup(box, level_hw, wrong)
        seen["levels"].add(l)
        pats = {row_pattern(sy[2 * ph], sy[2 * ph + 1], wrong)[0] for ph in range(7)}
        seen["patterns"] |= {(row_pattern(sy[2 * ph], sy[2 * ph + 1], wrong)[0], ph) for ph in range(7)}
        for pw, d in enumerate(column_walk(sx, wrong)[0]):
            seen["tuples"].add(d)
            for s, dec in zip(SLOTS, d):
                seen["triples"].add((s, dec, pw))
                seen["crossed"] |= {(p, s, dec, pw) for p in pats}
    return seen


# ---------------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------------
def _pixels(f, rows, cols):
    """f [H][W][C] at (rows, cols); a column of -1 reads zeros"""
    H, W, C = f.shape
    flat = np.concatenate([f.reshape(H * W, C), np.zeros((1, C), f.dtype)])
    return flat[np.where(cols < 0, H * W, rows * W + cols)]


def evaluate(feats, rois, wrong=(), plan="gather"):
    """[R][49][C] float32: acc += ((w1 v1 + w2 v2) + w3 v3) + w4 v4 over the samples (0,0), (0,1), (1,0), (1,1), then / 4 -- the order of
    the oracle and of both kernels.  plan "walk" multiplies the pixels walk_plan names instead of the gather kernel's."""
    feats = [np.asarray(f, F32) for f in feats]
    level_hw = [f.shape[:2] for f in feats]
    out = np.empty((len(rois), 49, feats[0].shape[2]), F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for r, box in enumerate(rois):
            l, sy, sx = roi_setup(box, level_hw, wrong)
            rows, cols = walk_plan(sy, sx, wrong) if plan == "walk" else gather_plan(sy, sx)
            w = weights(sy, sx)[..., None]
            v = _pixels(feats[l], rows, cols)                    # [49][4][4][C]
            acc = np.zeros((49, v.shape[-1]), F32)
            for s in range(4):
                acc = acc + (((w[:, s, 0] * v[:, s, 0] + w[:, s, 1] * v[:, s, 1]) + w[:, s, 2] * v[:, s, 2]) + w[:, s, 3] * v[:, s, 3])
            out[r] = acc / F32(4.0)
    return out


def evaluate_f64(feats, rois):
    """the same sums in float64 from the SAME float32 sample positions and 1-D weights (lo, hi, l, h of roi_sample): (value, sum |w v| / 4),
    both [R][49][C] float64.  The weight products are exact in float64."""
    feats = [np.asarray(f, F32) for f in feats]
    level_hw = [f.shape[:2] for f in feats]
    val = np.empty((len(rois), 49, feats[0].shape[2]), F64); mag = np.empty_like(val)
    for r, box in enumerate(rois):
        l, sy, sx = roi_setup(box, level_hw)
        rows, cols = gather_plan(sy, sx)
        w = np.zeros((49, 4, 4), F64)
        for ph in range(7):
            for pw in range(7):
                for iy in range(2):
                    for ix in range(2):
                        Y, X = sy[2 * ph + iy], sx[2 * pw + ix]
                        if Y[4] and X[4]:
                            hy, ly, hx, lx = float(Y[3]), float(Y[2]), float(X[3]), float(X[2])
                            w[ph * 7 + pw, iy * 2 + ix] = [hy * hx, hy * lx, ly * hx, ly * lx]
        t = w[..., None] * _pixels(feats[l], rows, cols).astype(F64)
        val[r] = t.sum(axis=(1, 2)) / 4.0
        mag[r] = np.abs(t).sum(axis=(1, 2)) / 4.0
    return val, mag


# ---------------------------------------------------------------------------------------------------------------------------
# processing order
# ---------------------------------------------------------------------------------------------------------------------------
def _to_int(x):
    """the device's float -> int conversion: truncation, saturating, NaN -> 0"""
    x = float(x)
    return 0 if x != x else int(max(-2147483648.0, min(2147483647.0, x)))


def order_key(box):
    """roi_order_kernel's position word: level << 22 | 16-row band << 12 | column, of the box centre on its level's map"""
    b = [F32(v) for v in box]
    l = roi_level(b)
    scale = F32(F32(1.0) / F32(4 << l))
    cy = F32(F32(F32(b[1] + b[3]) * F32(0.5)) * scale); cx = F32(F32(F32(b[0] + b[2]) * F32(0.5)) * scale)
    yb = min(max(_to_int(F32(cy * F32(0.0625))), 0), 1023)
    xb = min(max(_to_int(cx), 0), 4095)
    return (l << 22) | (yb << 12) | xb


def roi_order(rois):
    """the first n = len(rois) entries of a view's order: ascending position word, ties by DESCENDING index (the sort is descending on
    (complemented position, index))"""
    keys = [order_key(b) for b in rois]
    return np.array(sorted(range(len(rois)), key=lambda i: (keys[i], -i)), np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# split form (h16.h)
# ---------------------------------------------------------------------------------------------------------------------------
def split_words(x, wrong=()):
    """x [...][C] float32 (C % 16 == 0) -> uint32 [...][C]: the bytes h16_store4 leaves -- per 16-channel chunk 16 fp16 hi, then 16 fp16
    lo, hi = fp16(16 x), lo = fp16(16 x - hi), round to nearest even with subnormals"""
    x = np.asarray(x, F32)
    C = x.shape[-1]
    assert C % 16 == 0
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s = x * F32(16.0)
        hi = s.astype(np.float16)
        lo = ((x if "split_lo_from_x" in wrong else s) - hi.astype(F32)).astype(np.float16)
    halves = np.stack([hi.view(np.uint16).reshape(x.shape[:-1] + (C // 16, 16)), lo.view(np.uint16).reshape(x.shape[:-1] + (C // 16, 16))], axis=-2)
    return np.ascontiguousarray(halves).view("<u4").reshape(x.shape)


def join(words):
    """h16_join of every element of a split-form array: (hi + lo) / 16 in float32"""
    words = np.ascontiguousarray(words, "<u4")
    C = words.shape[-1]
    halves = words.view(np.uint16).reshape(words.shape[:-1] + (C // 16, 2, 16)).view(np.float16)
    return ((halves[..., 0, :].astype(F32) + halves[..., 1, :].astype(F32)) * F32(0.0625)).reshape(words.shape)
