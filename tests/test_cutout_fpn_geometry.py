"""The cut_out reuse's dirty sets beyond layer3 (cald_op_cutout_geometry over all 16 blocks, cald_op_cutout_fpn_geometry; host only) against
the CPU oracle: a view and its cutout version run through the whole ResNet-50 body and the FPN, and every pixel of the layer4 block outputs,
of the laterals (inner P2..P5) and of the 3 x 3 output convs (P2..P5) that differs must lie inside the predicted dirty set; the output
conv's set is the lateral's set plus exactly one ring.  Then the entry point against a restatement on boolean masks, over random sizes."""
import numpy as np
import pytest

STRIDES = np.array([1, 1, 1, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 2, 1, 1], np.int32)     # conv2 strides of layer1..layer4 (ResNet-50)
NB = len(STRIDES)
ENDS = [2, 6, 12, 15]            # the blocks whose outputs are C2..C5
SET = 17


@pytest.fixture(scope="module")
def model(oracle):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    return oracle.prepare_frcnn(sd, 21, 50)


def _call(fn, n_sets, H, W, mn, mx, rects):
    from cald_amd import _ffi
    r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1))
    out = np.zeros(n_sets * SET, np.int32)
    _ffi.check(fn(H, W, mn, mx, len(rects), _ffi.ptr(r, _ffi.c_i) if len(rects) else None, NB, _ffi.ptr(STRIDES, _ffi.c_i),
                  _ffi.ptr(out, _ffi.c_i)))
    return out


def block_geometry(H, W, mn, mx, rects):
    from cald_amd import _ffi
    return _call(_ffi.lib().cald_op_cutout_geometry, (NB + 1) * 2, H, W, mn, mx, rects).reshape(NB + 1, 2, SET)


def fpn_geometry(H, W, mn, mx, rects):
    """[0]: inner P2..P5, [1]: output P2..P5"""
    from cald_amd import _ffi
    return _call(_ffi.lib().cald_op_cutout_fpn_geometry, 8, H, W, mn, mx, rects).reshape(2, 4, SET)


def mask(s, H, W):
    m = np.zeros((H, W), bool)
    for i in range(s[0]):
        x0, y0, x1, y1 = s[1 + 4 * i: 5 + 4 * i]
        assert 0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H, (x0, y0, x1, y1, H, W)
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def ring(m):
    """the 3 x 3 pad-1 map of a mask"""
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def up2(m):
    return np.repeat(np.repeat(m, 2, axis=0), 2, axis=1)


def tensors(orc, P, img, mn, mx, rects):
    """the 16 block outputs, the four laterals and the four output convs, as the oracle's frcnn_backbone computes them"""
    x, _ = orc.preprocess_view(img, mn, mx, rects=rects)
    wk, bn = P["conv1"]
    y = orc._conv(P, "backbone.body.conv1.weight", x, wk, 7, 7, 2, 3, bn=bn, relu=True)
    y = orc.maxpool3x3s2(y)
    blocks = []
    for blk in P["blocks"]:
        idn = y
        pre = blk["name"]
        if "down" in blk:
            idn = orc._conv(P, pre + ".downsample.0.weight", y, blk["down"][0], 1, 1, blk["stride"], 0, bn=blk["down"][1])
        o = orc._conv(P, pre + ".conv1.weight", y, blk["conv1"][0], 1, 1, 1, 0, bn=blk["conv1"][1], relu=True)
        o = orc._conv(P, pre + ".conv2.weight", o, blk["conv2"][0], 3, 3, blk["stride"], 1, bn=blk["conv2"][1], relu=True)
        y = orc._conv(P, pre + ".conv3.weight", o, blk["conv3"][0], 1, 1, 1, 0, bn=blk["conv3"][1], residual=idn, relu=True)
        blocks.append(y)
    assert len(blocks) == NB and [b for b, k in enumerate(P["blocks"]) if k["layer_end"]] == ENDS
    feats = [blocks[b] for b in ENDS]
    fi, fl = "backbone.fpn.inner_blocks.%d.weight", "backbone.fpn.layer_blocks.%d.weight"
    inner = [None] * 4
    inner[3] = orc._conv(P, fi % 3, feats[3], P["fpn_inner"][3][0], 1, 1, 1, 0, bias=P["fpn_inner"][3][1])
    for i in (2, 1, 0):
        inner[i] = orc._conv(P, fi % i, feats[i], P["fpn_inner"][i][0], 1, 1, 1, 0, bias=P["fpn_inner"][i][1], up=inner[i + 1])
    outs = [orc._conv(P, fl % i, inner[i], P["fpn_layer"][i][0], 3, 3, 1, 1, bias=P["fpn_layer"][i][1]) for i in range(4)]
    return blocks, inner, outs


# a 64 x 96 view (scale 1, no padding): the smallest whose P5 is 2 x 3 while every level is half the one below
# rects: (left, top, right, bottom), right / bottom exclusive
CASES = {
    "corner": [[0, 0, 14, 10]],                                     # touches two borders
    "two_meeting_at_p3": [[10, 8, 18, 14], [30, 20, 38, 27]],       # far apart in the image, their upsampled P5 sets overlap from P4 down
    "large": [[20, 14, 38, 26]],                                    # 19 % x 19 % of the view: C5 is all dirty
    "none": [],
}


def differs(a, b):
    return np.any(a.view(np.uint32) != b.view(np.uint32), axis=2)


@pytest.mark.parametrize("case", sorted(CASES))
def test_layer4_and_fpn_sets_cover_every_changed_pixel(oracle, model, case):
    from cald_amd import synth
    H, W, mn, mx = 64, 96, 64, 96
    rects = CASES[case]
    img = synth.synth_image(3, H, W)
    ref = tensors(oracle, model, img, mn, mx, None)
    cut = tensors(oracle, model, img, mn, mx, np.array(rects, np.int32) if rects else None)
    assert ref[0][-1].shape[:2] == (2, 3) and [t.shape[:2] for t in ref[2]] == [(16, 24), (8, 12), (4, 6), (2, 3)]
    g = block_geometry(H, W, mn, mx, rects)
    f = fpn_geometry(H, W, mn, mx, rects)
    for b in (13, 14, 15):                                          # the three layer4 blocks
        h, w = ref[0][b].shape[:2]
        d = differs(ref[0][b], cut[0][b])
        assert not np.any(d & ~mask(g[1 + b, 0], h, w)), (case, b)
        assert d.any() == bool(rects)
    c_dirty = [mask(g[1 + b, 0], *ref[0][b].shape[:2]) for b in ENDS]
    inner = [mask(f[0, i], *ref[1][i].shape[:2]) for i in range(4)]
    outp = [mask(f[1, i], *ref[2][i].shape[:2]) for i in range(4)]
    for i in range(4):
        di, do = differs(ref[1][i], cut[1][i]), differs(ref[2][i], cut[2][i])
        assert not np.any(di & ~inner[i]), (case, "inner", i, np.argwhere(di & ~inner[i])[:5])
        assert not np.any(do & ~outp[i]), (case, "output", i, np.argwhere(do & ~outp[i])[:5])
        assert di.any() == bool(rects) and do.any() == bool(rects)
        # the rule: C_l's dirty set joined with the upsampled set of the lateral above; the output conv adds one ring, not more
        want = c_dirty[i] | (up2(inner[i + 1]) if i < 3 else False)
        assert np.array_equal(inner[i], want), (case, i)
        assert np.array_equal(outp[i], ring(inner[i])), (case, i)
    if not rects:
        assert not any(m.any() for m in inner + outp) and f[:, :, 0].max() == 0
    if case == "large":
        assert c_dirty[3].all()
    if case == "two_meeting_at_p3":
        a, b = [np.zeros_like(inner[1]) for _ in range(2)]
        for q, m in enumerate((a, b)):
            x0, y0, x1, y1 = f[0, 1, 1 + 4 * q: 5 + 4 * q]
            m[y0:y1 + 1, x0:x1 + 1] = True
        assert f[0, 1, 0] == 2 and np.any(a & b)                    # the two rectangles' sets overlap at P3
    if case == "corner":
        assert not c_dirty[0].all() and inner[0].all()               # C2 keeps clean pixels; the top-down path of so small a view leaves none in P2


# ---- the entry points against a restatement on boolean row / column vectors (a rectangle's mask is their outer product) ----
def _win(vec, k, s, p, n_out):
    """outputs of a k-wide, stride-s, pad-p window that meet a dirty input"""
    out = np.zeros(n_out, bool)
    for o in range(n_out):
        lo, hi = o * s - p, o * s - p + k
        out[o] = vec[max(lo, 0):max(hi, 0)].any()
    return out


def _resize(a, b, n_src, nr, n_pad):
    """resized pixels whose bilinear taps (floor(max(sc (y + 0.5) - 0.5, 0)) and the next), widened by one source index, meet [a, b)"""
    out = np.zeros(n_pad, bool)
    sc = n_src / nr
    for y in range(nr):
        t0 = int(max(sc * (y + 0.5) - 0.5, 0.0))
        out[y] = t0 + 2 >= a and t0 - 1 <= b - 1
    return out


def restated(H, W, mn, mx, rects):
    from cald_amd import _ffi
    import ctypes as C
    sz = [C.c_int() for _ in range(4)]
    _ffi.check(_ffi.lib().cald_op_transform_size(H, W, mn, mx, *[C.byref(s) for s in sz]))
    Hr, Wr, Hp, Wp = [s.value for s in sz]
    blocks = [np.zeros((Hp >> l, Wp >> l), bool) for l in (2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 5, 5, 5)]
    inner = [np.zeros((Hp >> l, Wp >> l), bool) for l in (2, 3, 4, 5)]
    outp = [m.copy() for m in inner]
    for (l, t, r, b) in rects:
        if r <= l or b <= t:
            continue
        ys, xs = _resize(t, b, H, Hr, Hp), _resize(l, r, W, Wr, Wp)
        if not (ys.any() and xs.any()):
            continue
        ys, xs = _win(ys, 7, 2, 3, Hp >> 1), _win(xs, 7, 2, 3, Wp >> 1)
        ys, xs = _win(ys, 3, 2, 1, Hp >> 2), _win(xs, 3, 2, 1, Wp >> 2)
        cs = []
        for bi, s in enumerate(STRIDES):
            ys, xs = _win(ys, 3, s, 1, len(ys) // s), _win(xs, 3, s, 1, len(xs) // s)
            blocks[bi] |= np.outer(ys, xs)
            if bi in ENDS:
                cs.append((ys, xs))
        iy, ix = cs[3]
        for i in (3, 2, 1, 0):
            if i < 3:
                iy, ix = cs[i][0] | np.repeat(iy, 2), cs[i][1] | np.repeat(ix, 2)
            inner[i] |= np.outer(iy, ix)
            outp[i] |= np.outer(_win(iy, 3, 1, 1, len(iy)), _win(ix, 3, 1, 1, len(ix)))
    return blocks, inner, outp


def test_entry_points_match_the_restatement_on_random_views():
    rs = np.random.RandomState(11)
    n_dirty = 0
    for it in range(300):
        H, W = int(rs.randint(40, 420)), int(rs.randint(40, 420))
        mn = int(rs.choice([64, 160, 300, 600]))
        mx = int(mn * rs.choice([1.0, 1.4, 1.667]))
        rects = []
        for _ in range(rs.randint(0, 3)):
            sh, sw = rs.uniform(0.05 * H, 0.2 * H), rs.uniform(0.05 * W, 0.2 * W)
            left, top = rs.uniform(0, W - sw), rs.uniform(0, H - sh)
            rects.append([int(left), int(top), int(left + sw), int(top + sh)])
        blocks, inner, outp = restated(H, W, mn, mx, rects)
        g = block_geometry(H, W, mn, mx, rects)
        f = fpn_geometry(H, W, mn, mx, rects)
        for b in range(NB):
            assert np.array_equal(mask(g[1 + b, 0], *blocks[b].shape), blocks[b]), (it, H, W, mn, mx, rects, b)
        for i in range(4):
            assert np.array_equal(mask(f[0, i], *inner[i].shape), inner[i]), (it, H, W, mn, mx, rects, "inner", i)
            assert np.array_equal(mask(f[1, i], *outp[i].shape), outp[i]), (it, H, W, mn, mx, rects, "output", i)
        n_dirty += bool(outp[0].any()) and not outp[0].all()
    assert n_dirty > 40                                             # the larger views leave P2 partly clean


def test_fpn_geometry_rejects_bad_arguments():
    from cald_amd import _ffi
    L = _ffi.lib()
    out = np.zeros(8 * SET, np.int32)
    r = np.zeros(20, np.int32)
    three = np.array([1, 1, 1, 2, 1, 2, 1], np.int32)               # three stages, not four
    assert L.cald_op_cutout_fpn_geometry(64, 96, 64, 96, 5, _ffi.ptr(r, _ffi.c_i), NB, _ffi.ptr(STRIDES, _ffi.c_i), _ffi.ptr(out, _ffi.c_i)) != 0
    assert L.cald_op_cutout_fpn_geometry(64, 96, 64, 96, 0, None, NB, _ffi.ptr(STRIDES, _ffi.c_i), None) != 0
    assert L.cald_op_cutout_fpn_geometry(64, 96, 64, 96, 0, None, len(three), _ffi.ptr(three, _ffi.c_i), _ffi.ptr(out, _ffi.c_i)) != 0
