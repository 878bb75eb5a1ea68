"""Rounding noise of precision="f16x3" against the exact mode on a RetinaNet's detections: the row _ffi.MARGIN_NOISE_F16X3_RETINA.

    python tools/retina_f16x3_noise.py [--images 256] [--out profiles/retina_f16x3_noise.json]

The decision-margin audit flags an image when one of its decisions lies within a few times the fast mode's rounding noise of its flip
point, so the noise has to be known on each margin's scale -- and it must not come from the audit's own output.  This tool measures it on
plain forwards: the pseudo-trained RetinaNet (synth.pseudo_trained_retinanet(21, 50, seed=0)) on synth.make_pool(n, "voc", seed=1), every
image once with precision="fp32" and once with precision="f16x3".  Over the views whose two detection lists have the same length and the
same labels (no decision flipped, so rows correspond) it takes the 90th percentile of

    |delta score|                              -> the score margins: post_thr, post_order, post_cap, ref_subsample, zero_row (7, 9, 10, 11, 13)
    |delta box coordinate| on the resized image -> post_small (15)
    |delta IoU| of neighbouring same-class rows -> post_iou, argmax (8, 12)

Slot 14 (cutout) is host arithmetic on the rectangles and keeps the Faster R-CNN row's value; slots 0-6 (RPN, RoI) do not occur.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCORE_SLOTS, IOU_SLOTS, BOX_SLOTS = (7, 9, 10, 11, 13), (8, 12), (15,)


def iou_rows(a, b):
    a = a.astype(np.float64); b = b.astype(np.float64)
    w = np.maximum(0.0, np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]))
    h = np.maximum(0.0, np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]))
    inter = w * h
    union = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter
    return inter / np.maximum(union, 1e-30)


def two_digits(x):
    return float("%.1e" % x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--min-size", type=int, default=600)
    ap.add_argument("--max-size", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retina_f16x3_noise.json"))
    args = ap.parse_args()
    if args.images < 256:
        raise SystemExit("the row is calibrated on at least 256 images")
    import torch
    from cald_amd import _ffi, detector, synth
    sd = synth.pseudo_trained_retinanet(21, 50, seed=0)
    pool = synth.make_pool(args.images, "voc", seed=1)
    dev = [torch.from_numpy(im).cuda() for im in pool]
    res = {}
    for prec in ("fp32", "f16x3"):
        m = detector.retinanet_resnet50_fpn_cal(num_classes=21, min_size=args.min_size, max_size=args.max_size, precision=prec).to("cuda")
        m.load_state_dict(sd); m.eval()
        out = []
        for i in range(0, len(dev), args.chunk):
            for r in m(dev[i:i + args.chunk]):
                out.append({k: r[k].cpu().numpy() for k in ("boxes", "scores", "labels")})
        res[prec] = out
        del m
        torch.cuda.empty_cache()
    L = _ffi.lib()
    ds, db, di = [], [], []
    used = 0
    for im, e, h in zip(pool, res["fp32"], res["f16x3"]):
        if len(e["labels"]) != len(h["labels"]) or not np.array_equal(e["labels"], h["labels"]) or len(e["labels"]) == 0:
            continue
        used += 1
        Hr, Wr, Hp, Wp = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _ffi.check(L.cald_op_transform_size(im.shape[0], im.shape[1], args.min_size, args.max_size, C.byref(Hr), C.byref(Wr), C.byref(Hp), C.byref(Wp)))
        sc = np.array([Wr.value / im.shape[1], Hr.value / im.shape[0]] * 2, np.float64)
        be, bh = e["boxes"].astype(np.float64) * sc, h["boxes"].astype(np.float64) * sc
        ds.append(np.abs(e["scores"].astype(np.float64) - h["scores"].astype(np.float64)))
        db.append(np.abs(be - bh).reshape(-1))
        same = e["labels"][1:] == e["labels"][:-1]
        if same.any():
            di.append(np.abs(iou_rows(be[:-1][same], be[1:][same]) - iou_rows(bh[:-1][same], bh[1:][same])))
    if used == 0:
        raise SystemExit("no view kept its detection list between the two modes")
    ds, db, di = np.concatenate(ds), np.concatenate(db), np.concatenate(di)
    pct = {name: {str(p): float(np.percentile(v, p)) for p in (50, 90, 99)} for name, v in (("score", ds), ("box", db), ("iou", di))}
    row = [0.0] * _ffi.N_MARGINS
    for q in SCORE_SLOTS:
        row[q] = two_digits(pct["score"]["90"])
    for q in IOU_SLOTS:
        row[q] = two_digits(pct["iou"]["90"])
    for q in BOX_SLOTS:
        row[q] = two_digits(pct["box"]["90"])
    row[14] = _ffi.MARGIN_NOISE_F16X3[14]
    doc = dict(command="python tools/retina_f16x3_noise.py --images %d --min-size %d --max-size %d" % (args.images, args.min_size, args.max_size),
               model="synth.pseudo_trained_retinanet(21, 50, seed=0)", pool="synth.make_pool(%d, 'voc', seed=1)" % args.images,
               images=args.images, views_used=used, detections=int(ds.size), neighbour_pairs=int(di.size), percentiles=pct,
               row_rule="90th percentile, two significant digits: score -> %s, iou -> %s, box -> %s, slot 14 = the Faster R-CNN row's"
                        % (list(SCORE_SLOTS), list(IOU_SLOTS), list(BOX_SLOTS)),
               MARGIN_NOISE_F16X3_RETINA=row)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
