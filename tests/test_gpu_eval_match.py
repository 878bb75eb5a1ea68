"""GPU tests of the evaluation matching kernels (cald_amd/csrc/eval.hip: cald_op_coco_match, cald_op_voc_match) and of the
``matching="device"`` path through both evaluators.  The reference is this package's host code (COCOeval.evaluate_img, voc_eval.best_overlaps
/ mark_detections), every comparison is np.array_equal or ==.  All boxes have integer coordinates, so every IoU is an exact rational and
the edge cases below (IoU equal to a threshold, equal IoUs, areas on a range's border) are hit on purpose, not by luck."""
import ctypes as C
import os

import numpy as np
import pytest

import _eval_scenes as S
from cald_amd import coco_eval as ce, voc_eval as ve

pytestmark = pytest.mark.gpu

MAX_DT, MAX_GT = 128, 256          # CALD_EVAL_MAX_DT / CALD_EVAL_MAX_GT of include/cald_hip.h


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run with -m gpu on a GPU box); no CPU fallback exists for the product path")
    from cald_amd import _ffi, detector
    assert (_ffi.EVAL_MAX_DT, _ffi.EVAL_MAX_GT) == (MAX_DT, MAX_GT)
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


# ---- the COCO operator ------------------------------------------------------------------------------------------------------------
def coco_op(hip, inp, thrs=None, rng=None, fill=None):
    """cald_op_coco_match on coco_reference's inputs; returns (rc, dt_match, dt_ignore, gt_ignore).  `fill` pre-sets the outputs."""
    ffi, L = hip["ffi"], hip["L"]
    thrs = np.ascontiguousarray(ce.IOU_THRS if thrs is None else thrs, np.float64)
    rng = np.ascontiguousarray(ce.AREA_RNG if rng is None else rng, np.float64)
    A, T, D, G = len(rng), len(thrs), int(inp["dt_off"][-1]), int(inp["gt_off"][-1])
    m, di, gi = np.full((A, T, D), -7 if fill is None else fill, np.int32), np.full((A, T, D), 9, np.uint8), np.full((A, G), 9, np.uint8)
    rc = L.cald_op_coco_match(hip["ctx"], len(inp["dt_off"]) - 1, ffi.ptr(inp["dt_off"], ffi.c_i64), ffi.ptr(inp["gt_off"], ffi.c_i64),
                              ffi.ptr(inp["dt_box"], ffi.c_d), ffi.ptr(inp["dt_area"], ffi.c_d), ffi.ptr(inp["gt_box"], ffi.c_d),
                              ffi.ptr(inp["gt_area"], ffi.c_d), ffi.ptr(inp["crowd"], ffi.c_u8), ffi.ptr(inp["ign"], ffi.c_u8), T, ffi.ptr(thrs, ffi.c_d),
                              A, ffi.ptr(rng, ffi.c_d), ffi.ptr(m, C.POINTER(C.c_int32)), ffi.ptr(di, ffi.c_u8), ffi.ptr(gi, ffi.c_u8))
    return rc, m, di, gi


def seg(dt, gt, area=None, crowd=None, ign=None):
    """One segment from xywh lists; the annotation area defaults to w * h, the flags to 0."""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    n = len(gt)
    return (dt, gt, np.asarray(gt[:, 2] * gt[:, 3] if area is None else area, np.float64).reshape(n),
            np.asarray(np.zeros(n) if crowd is None else crowd, np.uint8).reshape(n), np.asarray(np.zeros(n) if ign is None else ign, np.uint8).reshape(n))


def check_coco(hip, segments):
    inp, (want_m, want_di, want_gi) = S.coco_reference(segments)
    rc, m, di, gi = coco_op(hip, inp)
    assert rc == 0, hip["L"].cald_last_error()
    assert np.array_equal(gi, want_gi)
    assert np.array_equal(m, want_m), np.argwhere(m != want_m)[:5]
    assert np.array_equal(di, want_di), np.argwhere(di != want_di)[:5]
    return want_m, want_di, want_gi


def row_of_gts(n):
    """n disjoint 40 x 40 ground truths (area 1600: medium) in rows of 16."""
    return [[48.0 * (k % 16), 48.0 * (k // 16), 40.0, 40.0] for k in range(n)]


def test_coco_op_constructed_cases(hip):
    G40 = [0, 0, 40, 40]
    thr_ladder = [[0, 0, 20, k] for k in range(19, 9, -1)]          # against a 20 x 20 box: IoU k / 20 = 0.95 ... 0.50, one per threshold
    cases = {
        "1a no detections": seg([], [G40, [100, 0, 8, 8]]),
        "1b no ground truths": seg([[0, 0, 40, 40], [0, 0, 8, 8], [0, 0, 100, 100]], []),
        "2 two detections on one crowd": seg([[0, 0, 40, 40], [8, 8, 16, 16]], [[0, 0, 80, 80]], crowd=[1], ign=[1]),
        "3 the regular ground truth wins over a better ignored one": seg([[0, 0, 40, 40]], [[0, 0, 40, 36], [0, 0, 40, 24]], ign=[1, 0]),
        "4 IoU exactly 0.5": seg([[0, 0, 40, 20]], [G40]),
        "5 the same overlap at each threshold": seg(thr_ladder, [[0, 0, 20, 20]] * 10),
        "6 equal IoU: the later ground truth": seg([[8, 0, 40, 40], [8, 0, 40, 40]], [[0, 0, 40, 40], [16, 0, 40, 40], [8, 0, 40, 40]]),
        "7 areas on the borders": seg([[0, 0, 32, 32], [100, 0, 96, 96], [300, 0, 40, 40]], [[0, 0, 32, 32], [100, 0, 96, 96], [300, 0, 40, 40]],
                                      area=[1024, 9216, 1024]),
        "8 unmatched detections in and out of range": seg([[0, 0, 16, 16], [200, 200, 50, 50], [400, 400, 100, 100], [600, 0, 32, 32]], [[0, 300, 8, 8]]),
        "crowd and regular, detection prefers the regular": seg([[0, 0, 40, 40], [0, 0, 40, 40]], [[0, 0, 80, 80], G40], crowd=[1, 0], ign=[1, 0]),
        "ignored non-crowd is matched once": seg([[0, 0, 40, 40], [0, 0, 40, 40]], [G40], ign=[1]),
    }
    want = {}
    for name, s in cases.items():
        want[name] = check_coco(hip, [s])
    want_all = check_coco(hip, list(cases.values()))          # and all of them in one call
    # what the cases are meant to show, read off the reference's side
    m, di, gi = want["2 two detections on one crowd"]
    assert (m[0] == 0).all() and (di[0] == 1).all()
    m, di, gi = want["3 the regular ground truth wins over a better ignored one"]
    assert m[0, 0, 0] == 1 and di[0, 0, 0] == 0 and m[0, 6, 0] == 0 and di[0, 6, 0] == 1      # at 0.8 only the ignored one (IoU 0.9) passes
    m, di, gi = want["4 IoU exactly 0.5"]
    assert m[0, 0, 0] == 0 and m[0, 1, 0] == -1
    m, di, gi = want["5 the same overlap at each threshold"]
    assert (m[0, 0] >= 0).all() and (m[0, 9] >= 0).sum() == 1
    m, di, gi = want["6 equal IoU: the later ground truth"]
    assert m[0, 0, 0] == 2 and m[0, 0, 1] == 1
    m, di, gi = want["7 areas on the borders"]
    assert list(gi[1]) == [0, 1, 0] and list(gi[2]) == [0, 0, 0] and list(gi[3]) == [1, 0, 1]
    m, di, gi = want["8 unmatched detections in and out of range"]
    assert (m == -1).all() and list(di[1, 0]) == [0, 1, 1, 0] and list(di[2, 0]) == [1, 0, 1, 0] and list(di[3, 0]) == [1, 1, 0, 1]
    assert want_all[0].shape[2] == sum(len(s[0]) for s in cases.values())


@pytest.mark.parametrize("n_dt", [100, MAX_DT])
def test_coco_op_many_detections(hip, n_dt):
    """Exactly 100 detections (COCO's maxDets) and the cap: 20 ground truths, every detection near one of them."""
    rs = np.random.RandomState(n_dt)
    gts = row_of_gts(20)
    dts = [[gts[k % 20][0] + 8 * rs.randint(0, 3), gts[k % 20][1] + 8 * rs.randint(0, 3), 40, 40] for k in range(n_dt)]
    m, di, gi = check_coco(hip, [seg(dts, gts, crowd=[k == 7 for k in range(20)], ign=[k == 7 for k in range(20)])])
    assert (m[0, 0] >= 0).sum() >= 15 and (m[0, 0] == 7).sum() > 1 and (m[0, 0] == -1).any()


@pytest.mark.parametrize("n_gt", [1, 31, 32, 33, 63, 64, 65, MAX_GT])
def test_coco_op_flag_word_boundaries(hip, n_gt):
    """Ground-truth counts around the 32-bit words of the matched flags: the last, the first and a middle ground truth are each claimed
    twice (the second claim must fail), the last one is a crowd in a second segment (both claims hold)."""
    gts = row_of_gts(n_gt)
    picks = [n_gt - 1, 0, n_gt // 2, n_gt - 1, 0, n_gt // 2, max(n_gt - 2, 0)]
    dts = [gts[k] for k in picks]
    crowd = [k == n_gt - 1 for k in range(n_gt)]
    m, di, gi = check_coco(hip, [seg(dts, gts), seg(dts, gts, crowd=crowd, ign=crowd)])
    if n_gt == 1:
        assert list(m[0, 0]) == [0] + [-1] * 6 + [0] * 7
    else:
        assert list(m[0, 0, :7]) == [n_gt - 1, 0, n_gt // 2, -1, -1, -1, n_gt - 2]
        assert list(m[0, 0, 7:]) == [n_gt - 1, 0, n_gt // 2, n_gt - 1, -1, -1, n_gt - 2]


def test_coco_op_over_a_cap_is_unsupported_and_writes_nothing(hip):
    for s in (seg(row_of_gts(MAX_DT + 1), row_of_gts(3)), seg(row_of_gts(3), row_of_gts(MAX_GT + 1))):
        inp, _ = S.coco_reference([seg([[0, 0, 8, 8]], [[0, 0, 8, 8]]), s])
        rc, m, di, gi = coco_op(hip, inp)
        assert rc == hip["ffi"].ERR_UNSUPPORTED and b"the kernel takes" in hip["L"].cald_last_error()
        assert (m == -7).all() and (di == 9).all() and (gi == 9).all()
        with pytest.raises(NotImplementedError):
            hip["ffi"].check(rc)
    inp, _ = S.coco_reference([seg([[0, 0, 8, 8]], [[0, 0, 8, 8]])])
    rc, m, di, gi = coco_op(hip, inp, thrs=np.linspace(0.1, 0.9, 17))       # 17 x 4 variants
    assert rc == hip["ffi"].ERR_UNSUPPORTED and (m == -7).all()


def random_segments(seed, n):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        D, G = rs.randint(0, 21), rs.randint(0, 13)
        gt = np.stack([8 * rs.randint(0, 12, G), 8 * rs.randint(0, 12, G), 8 * rs.randint(1, 14, G), 8 * rs.randint(1, 14, G)], 1).astype(np.float64)
        dt = np.stack([8 * rs.randint(0, 12, D), 8 * rs.randint(0, 12, D), 8 * rs.randint(1, 14, D), 8 * rs.randint(1, 14, D)], 1).astype(np.float64)
        for d in range(D):                                    # most detections sit on or next to a ground truth
            if G and rs.rand() < 0.7:
                dt[d] = gt[rs.randint(G)] + 8 * np.array([rs.randint(-1, 2), rs.randint(-1, 2), 0, 0])
                dt[d, 2:] = np.maximum(8, dt[d, 2:] + 8 * rs.randint(-1, 2, 2))
        crowd = rs.rand(G) < 0.1
        area = gt[:, 2] * gt[:, 3] * rs.choice([1.0, 1.0, 0.5, 0.25], G)
        out.append(seg(dt, gt, area=area, crowd=crowd, ign=crowd | (rs.rand(G) < 0.1)))
    return out


def test_coco_op_random_segments(hip):
    segments = random_segments(0, 300)
    m, di, gi = check_coco(hip, segments)
    assert (m >= 0).mean() > 0.1 and (m == -1).mean() > 0.1 and 0.05 < di.mean() < 0.95 and 0.05 < gi.mean() < 0.95


# ---- the COCO evaluator -----------------------------------------------------------------------------------------------------------
def test_coco_evaluator_device_equals_cocoeval(hip, golden):
    scenes = {"random": S.random_scene(0), "known answers": S.golden_scene(golden("coco_ap_known_answers")),
              "one segment over the cap": S.random_scene(0, big_gt=MAX_GT + 1)}
    for name, (images, anns, cats, dets) in scenes.items():
        want = S.run(ce.COCOeval(ce.CocoGT(images, anns, cats)), images, dets)
        got = S.run(ce.FlatCOCOeval(ce.CocoGT(images, anns, cats), matching="device"), images, dets)
        S.assert_same_eval(got, want)
        assert got.host_segments == (1 if "cap" in name else 0), name
        flat = S.run(ce.FlatCOCOeval(ce.CocoGT(images, anns, cats), matching="host"), images, dets)._chunks[0]
        dev = got._chunks[0]
        for key in ("dt_gid", "dt_ig", "gt_ig"):              # the flat match arrays themselves, not only what accumulate makes of them
            assert np.array_equal(getattr(dev, key), getattr(flat, key)), (name, key)
        if name == "known answers":
            np.testing.assert_allclose(got.stats, golden("coco_ap_known_answers")["stats"], rtol=0, atol=1e-12)


def test_coco_evaluator_device_in_batches(hip):
    images, anns, cats, dets = S.random_scene(2)
    want = S.run(ce.COCOeval(ce.CocoGT(images, anns, cats)), images, dets, batches=3)
    ev = ce.CocoEvaluator(ce.CocoGT(images, anns, cats), ["bbox"], matching="device")
    assert type(ev.coco_eval["bbox"]) is ce.FlatCOCOeval
    got = S.run(ev.coco_eval["bbox"], images, dets, batches=3)
    S.assert_same_eval(got, want)


# ---- the VOC operator -------------------------------------------------------------------------------------------------------------
def check_voc(hip, image_ids, BB, table):
    BB = np.asarray(BB, np.float64).reshape(-1, 4)
    ovmax, jmax = ve.best_overlaps(image_ids, BB, table)
    got_ov, got_j, tp, fp = ve.match_device(image_ids, BB, table, ve.IOU_THRESHOLDS)
    assert got_ov.dtype == np.float64 and got_j.dtype == np.int64
    assert np.array_equal(got_ov, ovmax) and np.array_equal(got_j, jmax)
    for i, t in enumerate(ve.IOU_THRESHOLDS):
        wtp, wfp = ve.mark_detections(image_ids, ovmax, jmax, table, t)
        assert np.array_equal(tp[i], wtp) and np.array_equal(fp[i], wfp), t
    return ovmax, jmax, tp, fp


def gt_entry(boxes, difficult=None):
    b = np.array(boxes).astype(float)
    return (b, np.array([0] * len(boxes) if difficult is None else difficult).astype(bool))


def test_voc_op_constructed_cases(hip):
    table = {
        "equal": gt_entry([[10, 0, 19, 9], [0, 0, 9, 9]]),                        # a detection in the middle overlaps both equally
        "ladder": gt_entry([[0, 0, 9, 9]]),                                       # 10 x 10 = 100 pixels
        "difficult": gt_entry([[0, 0, 9, 9], [20, 0, 29, 9]], [1, 0]),
        "none": gt_entry([]),
        "touch": gt_entry([[0, 0, 9, 9]]),
    }
    rows = [("equal", [5, 0, 14, 9]),
            ("ladder", [0, 0, 9, 4]), ("ladder", [0, 0, 9, 5]), ("ladder", [0, 0, 9, 6]), ("ladder", [0, 0, 9, 8]), ("ladder", [0, 0, 9, 9]),
            ("difficult", [0, 0, 9, 9]), ("difficult", [20, 0, 29, 9]), ("difficult", [20, 0, 29, 9]),
            ("none", [0, 0, 9, 9]),
            ("touch", [9, 9, 18, 18])]
    ids, BB = [r[0] for r in rows], [r[1] for r in rows]
    ov, j, tp, fp = check_voc(hip, ids, BB, table)
    assert j[0] == 0 and ov[0] == 50 / 150                                        # the first of two equal maxima
    assert ov[1] == 0.5 and tp[0, 1] == 0 and fp[0, 1] == 1                       # equal to the threshold: no match
    assert ov[2] == 0.6 and tp[2, 2] == 0 and fp[2, 2] == 1 and tp[1, 2] == 1     # 60 / 100 == the literal 0.6
    assert tp[0, 5] == 0 and fp[0, 5] == 1 and tp[9, 5] == 1                      # the box was claimed at 0.5 by row 2, still free at 0.95
    assert tp[:, 6].sum() == 0 and fp[:, 6].sum() == 0                            # difficult: neither
    assert tp[0, 7] == 1 and fp[0, 8] == 1                                        # the second detection on a claimed box
    assert ov[9] == -np.inf and j[9] == 0 and fp[:, 9].all()
    assert ov[10] == 1 / 199 and fp[:, 10].all()                                  # one shared pixel


def test_voc_op_tied_confidences_over_images(hip, tmp_path):
    """Three-decimal scores tie constantly: the order is read_detections' np.argsort(-confidence), and the device path must mark in it."""
    rs = np.random.RandomState(3)
    names = ["im%02d" % i for i in range(12)]
    table = {n: gt_entry([[8 * rs.randint(0, 5), 8 * rs.randint(0, 5), 8 * rs.randint(6, 12), 8 * rs.randint(6, 12)] for _ in range(rs.randint(1, 4))])
             for n in names}
    lines = []
    for k in range(90):
        n = names[rs.randint(12)]
        g = table[n][0][rs.randint(len(table[n][0]))]
        b = g + 8 * rs.randint(-1, 2, 4)
        lines.append("%s %.3f %.1f %.1f %.1f %.1f\n" % (n, rs.choice([0.9, 0.5, 0.25]), b[0], b[1], max(b[2], b[0] + 8), max(b[3], b[1] + 8)))
    fn = tmp_path / "det.txt"
    fn.write_text("".join(lines))
    image_ids, BB = ve.read_detections(str(fn))
    ov, j, tp, fp = check_voc(hip, image_ids, BB, table)
    assert tp[0].sum() >= 12 and fp[0].sum() >= 12 and tp[9].sum() < tp[0].sum()


def test_voc_op_random_segments(hip):
    rs = np.random.RandomState(1)
    names = ["s%03d" % i for i in range(200)]
    table, ids, BB = {}, [], []
    for n in names:
        G = rs.randint(0, 9)
        gt = np.stack([8 * rs.randint(0, 10, G), 8 * rs.randint(0, 10, G), 8 * rs.randint(0, 10, G), 8 * rs.randint(0, 10, G)], 1)
        gt[:, 2:] += gt[:, :2] + 7
        table[n] = gt_entry(gt.tolist(), (rs.rand(G) < 0.2).tolist())
        for _ in range(rs.randint(0, 12)):
            b = (gt[rs.randint(G)] + 8 * rs.randint(-1, 2, 4)) if G and rs.rand() < 0.8 else np.r_[8 * rs.randint(0, 10, 2), 8 * rs.randint(10, 20, 2)]
            ids.append(n); BB.append([b[0], b[1], max(b[2], b[0]), max(b[3], b[1])])
    perm = rs.permutation(len(ids))                           # the class's confidence order interleaves the images
    ov, j, tp, fp = check_voc(hip, [ids[i] for i in perm], np.array(BB, np.float64)[perm], table)
    assert len(ids) > 800 and tp[0].sum() > 100 and (ov == -np.inf).any() and (j > 0).any()


def test_voc_op_over_a_cap_is_unsupported_and_the_python_layer_goes_to_the_host(hip):
    ffi, L = hip["ffi"], hip["L"]
    for nd, G in ((MAX_DT + 1, 1), (1, MAX_GT + 1)):
        dt_off, gt_off = np.array([0, nd], np.int64), np.array([0, G], np.int64)
        gt_box, diff = np.tile(np.array([0., 0., 9., 9.]), (G, 1)), np.zeros(G, np.uint8)
        dt_box, idx = np.tile(np.array([0., 0., 9., 9.]), (nd, 1)), np.arange(nd, dtype=np.int64)
        thrs = np.array(ve.IOU_THRESHOLDS, np.float64)
        ov, jm, tp, fp = np.full(nd, 7.0), np.full(nd, 7, np.int64), np.full((10, nd), 9, np.uint8), np.full((10, nd), 9, np.uint8)
        rc = L.cald_op_voc_match(hip["ctx"], 1, ffi.ptr(dt_off, ffi.c_i64), ffi.ptr(gt_off, ffi.c_i64), ffi.ptr(gt_box, ffi.c_d), ffi.ptr(diff, ffi.c_u8),
                                 ffi.ptr(dt_box, ffi.c_d), ffi.ptr(idx, ffi.c_i64), 10, ffi.ptr(thrs, ffi.c_d), nd, ffi.ptr(ov, ffi.c_d),
                                 ffi.ptr(jm, ffi.c_i64), ffi.ptr(tp, ffi.c_u8), ffi.ptr(fp, ffi.c_u8))
        assert rc == ffi.ERR_UNSUPPORTED and (ov == 7).all() and (jm == 7).all() and (tp == 9).all() and (fp == 9).all()
        check_voc(hip, ["a"] * nd, dt_box, {"a": gt_entry(gt_box.tolist())})
    check_voc(hip, ["a"] * MAX_DT, np.tile(np.array([0., 0., 9., 9.]), (MAX_DT, 1)), {"a": gt_entry([[0, 0, 9, k % 10 + 5] for k in range(MAX_GT)])})
    check_voc(hip, [], np.zeros((0, 4)), {"a": gt_entry([[0, 0, 9, 9]])})


# ---- the VOC path -----------------------------------------------------------------------------------------------------------------
def test_voc_device_path_on_the_golden_tree(hip, golden, tmp_path, capsys):
    from types import SimpleNamespace
    from test_cpu_host import _materialise_voc_tree
    g = golden("voc_eval")
    root = str(tmp_path)
    classes, imagesetfile, annopath = _materialise_voc_tree(g, root)
    ann = ve.VocAnnotations(imagesetfile, annopath)
    with np.errstate(all="ignore"):
        for cls in classes[1:]:
            fn = os.path.join(root, "res", "det_test_%s.txt" % cls)
            for use07 in (False, True):
                multi = ve.voc_eval_thresholds(cls, fn, ann, [float(t) for t in g["ious"]], use_07_metric=use07, matching="device")
                assert len(multi) == len(g["ious"])
                for t, (rec, prec, ap) in zip(g["ious"], multi):
                    key = "%s_%d_%d" % (cls, int(round(float(t) * 100)), int(use07))
                    np.testing.assert_array_equal(rec, g["rec_" + key])
                    np.testing.assert_array_equal(prec, g["prec_" + key])
                    np.testing.assert_array_equal(np.float64(ap), g["ap_" + key])
        for key, ncls in (("python_eval_stdout", 5), ("python_eval_stdout_3cls", 4)):
            loader = SimpleNamespace(dataset=SimpleNamespace(root=root, image_set="test",
                                                             _transforms=SimpleNamespace(transforms=[SimpleNamespace(CLASSES=tuple(classes[:ncls]))])))
            want = ve.do_python_eval(loader, "2012", "res", root=root)
            capsys.readouterr()
            got = ve.do_python_eval(loader, "2012", "res", root=root, matching="device")
            assert capsys.readouterr().out == str(g[key])
            assert repr(got) == repr(want) and got["line"] == str(g[key]).splitlines()[1]        # repr(): an AP may be nan


# ---- the engine -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_model(hip):
    from cald_amd import synth
    model = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=300, max_size=500)
    model.to("cuda").load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0))
    model.eval()
    return model


def test_engine_voc_evaluate_device_equals_host(hip, tiny_model, tmp_path):
    from types import SimpleNamespace
    torch = hip["torch"]
    from cald_amd import synth, engine
    pool = synth.make_pool(3, "voc", 0, scale=0.5)
    names = ["2010_%06d" % (7 * i + 3) for i in range(len(pool))]
    classes = ('__background__',) + tuple("class%02d" % c for c in range(1, 21))
    root = str(tmp_path)
    base = os.path.join(root, "VOCdevkit", "VOC2012")
    os.makedirs(os.path.join(base, "ImageSets", "Main")); os.makedirs(os.path.join(base, "Annotations"))
    with open(os.path.join(base, "ImageSets", "Main", "test.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    ds = SimpleNamespace(root=root, image_set="test", _transforms=SimpleNamespace(transforms=[SimpleNamespace(CLASSES=classes)]))

    class Loader(list):
        dataset = ds
    loader = Loader(((torch.from_numpy(im).permute(2, 0, 1).float().div(255),), ({"name": torch.tensor([ord(ch) for ch in n])},))
                    for im, n in zip(pool, names))
    all_boxes, index = engine.voc_detections(tiny_model, loader, len(classes), 4)
    for i, n in enumerate(names):                             # ground truth: the image's three best detections, rounded; the third is difficult
        cand = sorted(((float(all_boxes[c][i][0][k, 4]), c, k) for c in range(1, 21) if all_boxes[c][i] != [] for k in range(all_boxes[c][i][0].shape[0])), reverse=True)[:3]
        xml = "<annotation>"
        for r, (_, c, k) in enumerate(cand):
            b = np.round(all_boxes[c][i][0][k, :4].numpy()).astype(int) + 1
            xml += ("<object><name>%s</name><difficult>%d</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                    % (classes[c], int(r == 2), b[0], b[1], max(b[2], b[0] + 1), max(b[3], b[1] + 1)))
        with open(os.path.join(base, "Annotations", n + ".xml"), "w") as f:
            f.write(xml + "</annotation>")
    with np.errstate(all="ignore"):
        want = engine.voc_evaluate(tiny_model, loader, "2012", path="host", root=root, batch_views=4)
        got = engine.voc_evaluate(tiny_model, loader, "2012", path="dev", root=root, batch_views=4, matching="device")
    for cls in classes[1:]:
        assert open(os.path.join(root, "host", "det_test_%s.txt" % cls)).read() == open(os.path.join(root, "dev", "det_test_%s.txt" % cls)).read()
    assert got["line"] == want["line"] and str(got) == str(want)              # str(): classes without ground truth have AP nan
    assert max(a for a in got["ap_per_class"] if a == a) > 0.5


def test_engine_coco_evaluate_device_equals_host(hip, tiny_model, capsys):
    torch = hip["torch"]
    from cald_amd import synth, engine
    pool = synth.make_pool(3, "voc", 5, scale=0.5)
    imgs = [torch.from_numpy(im).permute(2, 0, 1).float().div(255) for im in pool]
    plain = [((im,), ({"image_id": torch.tensor(40 + i)},)) for i, im in enumerate(imgs)]
    preds = engine.coco_predictions(tiny_model, plain, batch_views=4)

    class Dataset(list):
        pass
    ds = Dataset()
    for i, im in enumerate(imgs):                             # ground truth: the three best detections of each image, the third a crowd
        p = preds[40 + i]
        b = torch.round(p["boxes"][:3]).double() + torch.tensor([0., 0., 1., 1.])
        ds.append((im, {"image_id": torch.tensor(40 + i), "boxes": b, "labels": p["labels"][:3], "area": (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]),
                        "iscrowd": torch.tensor([0, 0, 1][:len(b)])}))

    class Loader(list):
        dataset = ds
    loader = Loader(((im,), (t,)) for im, t in ds)
    want = engine.coco_evaluate(tiny_model, loader, classwise=True, batch_views=4)
    out_host = capsys.readouterr().out
    got = engine.coco_evaluate(tiny_model, loader, classwise=True, batch_views=4, matching="device")
    assert capsys.readouterr().out == out_host and "Average Precision" in out_host
    assert type(got.coco_eval["bbox"]) is ce.FlatCOCOeval and got.coco_eval["bbox"].host_segments == 0
    S.assert_same_eval(got.coco_eval["bbox"], want.coco_eval["bbox"])
    assert got.img_ids == want.img_ids and want.coco_eval["bbox"].stats[1] > 0
