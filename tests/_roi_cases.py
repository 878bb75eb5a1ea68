"""Constructed inputs of the RoIAlign tests (test_roi_align.py on the CPU, test_gpu_roi_align.py on the GPU).

The 1-D profiles (start, extent), in pixels of the map they fall on, were picked by a greedy cover over the exhaustive family of
test_roi_align.py (FAMILY_*) so that together they reach every reachable (slot, decision, pw) of roi_rows_walk's column walk, every
decision 4-tuple and every (row pattern, ph); test_roi_align.py recomputes that census from the cases and asserts it, so a profile
list that stops covering something fails there.  Level 0 RoIs are the full cross of a map's column profiles with its row profiles:
every column decision meets every row pattern (each pattern is its own instantiation of the walk).  The named edges (a sample at
exactly t == size, one ulp beyond, t in [-1, 0), clamps, zero extents, invalid rows / columns, level boundaries) are added by hand
and asserted by test_named_edges_are_present.
"""
import functools

import numpy as np

F32 = np.float32
C_MAX = 260                     # features are made once at 260 channels; the C = 256 / C = 8 cases are their first channels
ROI_CAP = 1000

# ---- the exhaustive 1-D family (the census of the issue): map sizes, starts -6 .. size + 3 in steps of 1/8, fifteen extents ----
FAMILY_SIZES = (1, 2, 3, 5, 9, 16)
FAMILY_EXTENTS = (0, 0.5, 1, 1.75, 2.5, 3.5, 5, 7, 9.25, 12, 14, 17.5, 21, 28, 40)


def family(sizes=FAMILY_SIZES):
    for size in sizes:
        for k in range(-48, (size + 3) * 8 + 1):
            for ext in FAMILY_EXTENTS:
                yield size, k / 8.0, ext


# ---- pyramids: level 0 of 3 x 3 and 9 x 7 ([H][W]), smaller upper levels, one level of 1 x 1 ----
PYRAMIDS = {"a": [(3, 3), (2, 2), (1, 2), (1, 1)], "b": [(9, 7), (5, 4), (3, 2), (1, 1)]}



def ULP(x):
    return float(np.spacing(F32(x)))


# column profiles of a 3-pixel and a 7-pixel axis, row profiles of a 3-pixel and a 9-pixel axis: (start, extent)
COVER_X3 = [(-2.25, 7), (-0.25, 2.5), (0.0, 14), (-4.25, 17.5), (-3.375, 7), (-1.125, 2.5), (0.0, 21), (-2.875, 7), (-3.0, 17.5), (1.25, 7), (-6.0, 17.5),
            (0.0, 5), (-0.125, 5), (0.25, 0), (-0.375, 1.75), (0.5, 3.5), (-0.625, 1.75), (-1.25, 17.5), (-2.25, 17.5), (-4.125, 28)]
COVER_X7 = [(0.0, 9.25), (0.5, 5), (-6.0, 9.25), (-2.125, 28), (-5.875, 21), (-3.0, 17.5), (0.375, 7), (-0.125, 28), (0.5, 9.25), (0.25, 17.5),
            (-0.625, 9.25), (-4.125, 28)]
COVER_Y3 = [(0.0, 0), (-1.375, 7), (-2.375, 7), (-3.375, 7), (0.0, 9.25), (0.0, 14), (0.0, 21), (-0.25, 2.5), (-0.25, 7)]
COVER_Y9 = [(0.0, 0), (0.25, 7), (0.0, 21), (-2.25, 17.5), (0.0, 12), (0.125, 9.25)]
# by hand: extent 7 gives bins of exactly one pixel, samples at start + p + 1/4 and + 3/4
EDGE_X3 = [(0.75, 7),                          # t == 3 exactly at (p 2, i 0): valid; the next sample is outside
           (4.5, 1)]                           # every column outside on the right
EDGE_X7 = [(0.75, 7),                          # t == 7 exactly at (p 6, i 0)
           (0.75 + ULP(7.0), 7),               # the same sample one ulp beyond 7 (start + 6 and + 1/4 are exact): invalid
           (8.5, 1), (3.25, 0)]                # outside on the right; zero width
EDGE_Y3 = [(0.75, 7), (-6.0, 2.5)]             # t == 3; every row above -1
EDGE_Y9 = [(2.75, 7), (2.75 + ULP(9.0), 7),    # t == 9 exactly, and one ulp beyond
           (-6.0, 2.5), (10.5, 1)]             # every row outside, above and below
# upper levels: (level, (x start, extent)) -- the decision tuples that need a 2- or 4-pixel axis; the height puts sqrt(area) at 20 pixels
# of the level's own map, inside the level's range of [14, 28)
UPPER = {"a": [(1, (0.0, 21)), (1, (-2.25, 17.5)), (1, (-3.0, 17.5)), (1, (-4.125, 28)), (2, (0.0, 21)), (2, (-3.0, 17.5)), (3, (-9.5, 20)), (3, (0.0, 16))],
         "b": [(1, (-2.5, 40)), (1, (-4.125, 28)), (1, (0.25, 17.5)), (2, (0.0, 21)), (2, (-2.25, 17.5)), (2, (-3.0, 17.5)), (2, (-4.125, 28)),
               (3, (-9.5, 20)), (3, (0.0, 16))]}
BOUNDARIES = (112.0, 224.0, 448.0)             # sqrt(area) at which the level changes


def _features(seed, hw):
    """finite float32 [H][W][C_MAX]: sign * [1, 2) * 2^e with e in -28 .. 4 (16 x is an fp16 subnormal below 2^-18), distinct values"""
    rs = np.random.RandomState(seed)
    H, W = hw
    x = ((1.0 + rs.rand(H, W, C_MAX)) * 2.0 ** rs.randint(-28, 5, (H, W, C_MAX)) * rs.choice([-1.0, 1.0], (H, W, C_MAX))).astype(F32)
    assert np.isfinite(x).all() and (np.diff(np.sort(x.reshape(H * W, C_MAX), axis=0), axis=0) != 0).all()       # no two pixels agree in any channel
    return x


def _box(l, xs, ys):
    """image coordinates of the RoI whose profiles on level l are xs, ys = (start, extent): times 4 << l (exact)"""
    s = F32(4 << l)
    x1, y1 = F32(xs[0]), F32(ys[0])
    return [x1 * s, y1 * s, F32(x1 + F32(xs[1])) * s, F32(y1 + F32(ys[1])) * s]


def _boundary_boxes():
    out = []
    for b in BOUNDARIES:
        for k in (-1, 0, 1, 2, 3, 4, 5, 6):        # sides b (1 - k 2^-24): one ulp above, the boundary, one to six ulps below
            a = F32(b * (1.0 - k * 2.0 ** -24)) if k >= 0 else np.nextafter(F32(b), F32(np.inf))
            out.append([F32(0), F32(0), a, a])
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """one pyramid with its RoIs: dict(level_hw, feats (C_MAX channels), rois [R][4] float32, n_cross = how many of them are the level 0 cross)"""
    hw = PYRAMIDS[name]
    feats = [_features(100 * (1 + "ab".index(name)) + l, s) for l, s in enumerate(hw)]
    px, py = (COVER_X3 + EDGE_X3, COVER_Y3 + EDGE_Y3) if name == "a" else (COVER_X7 + EDGE_X7, COVER_Y9 + EDGE_Y9)
    rois = [_box(0, xs, ys) for xs in px for ys in py]
    n_cross = len(rois)
    for l, xs in UPPER[name]:
        h = 400.0 / xs[1]
        rois.append(_box(l, xs, (hw[l][0] / 2.0 - h / 2.0, h)))
    rois += _boundary_boxes()
    rois.append([F32(5), F32(9), F32(2), F32(11)])          # x2 < x1: negative area (level 0), rw raised to 1
    rois = np.array(rois, F32)
    assert np.isfinite(rois).all() and len(rois) <= ROI_CAP
    for f in feats:
        f.setflags(write=False)
    rois.setflags(write=False)
    return dict(name=name, level_hw=hw, feats=feats, rois=rois, n_cross=n_cross, px=px, py=py)


def feats_at(c, C):
    return [np.ascontiguousarray(f[:, :, :C]) for f in c["feats"]]


# ---- the views case: V = 9, so XCD column 0 holds views 0 and 8 ----
VIEW_COUNTS = (1000, 0, 1000, 7, 64, 1, 1000, 999, 1000)        # an empty view between full ones; view 6: every RoI ties on the order key
TIE_VIEW = 6
CLAMP_VIEW = 3
# the order key's clamps (level 0, centres in map pixels): column 5000 and 4250 -> 4095 (a tie), row band 1093 and 1031 -> 1023 (a tie),
# a negative centre -> (0, 0), and two ordinary boxes
CLAMP_ROIS = [[19992, 0, 20008, 16], [16992, 0, 17008, 16], [0, 69992, 16, 70008], [0, 65992, 16, 66008], [-500, -500, -480, -480], [1, 1, 9, 9],
              [2, 2, 10, 10]]


@functools.lru_cache(maxsize=None)
def views_case():
    """dict(V, counts, level_hw [V][4], feats [V][4] (256 channels), rois [V] of [n][4])"""
    V = len(VIEW_COUNTS)
    rs = np.random.RandomState(77)
    level_hw, feats, rois = [], [], []
    for v in range(V):
        H, W = 3 + v, 4 + (3 * v) % 7
        hw = [(H, W)]
        for _ in range(3):
            hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
        level_hw.append(hw)
        feats.append([np.ascontiguousarray(_features(1000 + 10 * v + l, s)[:, :, :256]) for l, s in enumerate(hw)])
        n = VIEW_COUNTS[v]
        if v == TIE_VIEW:           # level 0 boxes whose centre lies in pixel column 1 (rows: every map here has fewer than 16)
            cx, cy = 4 * (1.05 + 0.9 * rs.rand(n)), 4 * H * rs.rand(n)
            w, h = 2 + 30 * rs.rand(n), 2 + 30 * rs.rand(n)
        else:
            cx, cy = 4 * (-1 + (W + 2) * rs.rand(n)), 4 * (-1 + (H + 2) * rs.rand(n))
            w, h = 2.0 ** (1 + 9.3 * rs.rand(n)), 2.0 ** (1 + 9.3 * rs.rand(n))      # 2 .. 1260 pixels: every level
        b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1).astype(F32).reshape(n, 4)
        if v == CLAMP_VIEW:
            b = np.array(CLAMP_ROIS, F32)
        b.setflags(write=False)
        rois.append(b)
    return dict(V=V, counts=np.array(VIEW_COUNTS, np.int32), level_hw=level_hw, feats=feats, rois=rois)
