"""Scenes and reference packaging shared by tests/test_eval_flat.py (CPU) and tests/test_gpu_eval_match.py (GPU): seeded COCO scenes on an
integer grid, the scene of tests/golden/coco_ap_known_answers.npz, and evaluate_img's results laid out like cald_op_coco_match's outputs."""
import json

import numpy as np

from cald_amd import coco_eval as ce


def random_scene(seed=0, n_img=30, n_cat=5, big_gt=0):
    """(images, annotations, categories, detections): boxes on a grid of 8 (every IoU an exact rational), about 10 % crowds, annotation
    areas that differ from w * h, two-decimal scores (ties), image 3 with more than 100 detections of category 1, an image without
    detections, a category-image pair with detections only, and an annotation with id 0 (pycocotools' "unmatched" quirk).
    big_gt > 0 puts that many ground truths of category 2 into image 5."""
    rs = np.random.RandomState(seed)
    images = [{"id": 11 + 3 * i} for i in range(n_img)]
    cats = [{"id": 2 * c + 1} for c in range(n_cat)]
    anns, dets = [], []

    def box(lo=1, hi=20):
        w, h = 8 * rs.randint(lo, hi), 8 * rs.randint(lo, hi)
        return [float(8 * rs.randint(0, 30)), float(8 * rs.randint(0, 30)), float(w), float(h)]
    for i, im in enumerate(images):
        for _ in range(rs.randint(0, 7)):
            b = box()
            area = b[2] * b[3] * (1.0 if rs.rand() < 0.5 else rs.choice([0.25, 0.5, 0.75]))
            anns.append({"id": len(anns), "image_id": im["id"], "category_id": cats[rs.randint(n_cat)]["id"], "bbox": b, "area": area,
                         "iscrowd": int(rs.rand() < 0.1)})
        if i == 5:
            for k in range(big_gt):
                b = [float(8 * (k % 32)), float(8 * (k // 32)), 8.0, 8.0]
                anns.append({"id": len(anns), "image_id": im["id"], "category_id": cats[1]["id"], "bbox": b, "area": 64.0, "iscrowd": 0})
        if i == 7:
            continue                                          # ground truth only
        mine = [a for a in anns if a["image_id"] == im["id"]]
        n_det = 130 if i == 3 else rs.randint(0, 25)
        for _ in range(n_det):
            if mine and rs.rand() < 0.6:                      # near a ground truth: shifted / resized on the grid
                a = mine[rs.randint(len(mine))]
                b = [a["bbox"][0] + 8 * rs.randint(-1, 2), a["bbox"][1] + 8 * rs.randint(-1, 2),
                     max(8.0, a["bbox"][2] + 8 * rs.randint(-1, 2)), max(8.0, a["bbox"][3] + 8 * rs.randint(-1, 2))]
                cat = a["category_id"]
            else:
                b, cat = box(), cats[rs.randint(n_cat)]["id"]
            if i == 3:
                cat = cats[0]["id"]
            dets.append({"image_id": im["id"], "category_id": cat, "bbox": [float(v) for v in b], "score": float(np.round(rs.rand(), 2))})
    return images, anns, cats, dets


def golden_scene(g):
    return (json.loads(str(g["images"])), json.loads(str(g["annotations"])), json.loads(str(g["categories"])), json.loads(str(g["detections"])))


def run(ev, images, dets, batches=1):
    """add_results + evaluate in `batches` calls (the evaluator sees the images of a batch with that batch's detections), then
    accumulate and summarize."""
    ids = [im["id"] for im in images]
    for b in range(batches):
        part = ids[b::batches]
        ev.add_results([d for d in dets if d["image_id"] in part])
        ev.evaluate(part)
    ev.accumulate()
    ev.summarize(quiet=True)
    return ev


def assert_same_eval(got, want):
    for key in ("precision", "recall", "scores"):
        assert got.eval[key].shape == want.eval[key].shape and np.array_equal(got.eval[key], want.eval[key]), key
    assert np.array_equal(np.asarray(got.stats), np.asarray(want.stats))


def coco_reference(segments):
    """evaluate_img on hand-built segments, in the layout of cald_op_coco_match.  A segment is (dt_box [D, 4] in score order, gt_box
    [G, 4], gt_area [G], iscrowd [G], ignore [G]).  Returns the op's inputs and the expected (dt_match, dt_ignore, gt_ignore)."""
    A, T = len(ce.AREA_RNG), len(ce.IOU_THRS)
    images, anns, dets = [], [], []
    for s, (dt, gt, area, crowd, ign) in enumerate(segments):
        images.append({"id": s + 1})
        for k in range(len(gt)):
            anns.append({"id": len(anns) + 1, "image_id": s + 1, "category_id": 1, "bbox": [float(v) for v in gt[k]], "area": float(area[k]),
                         "iscrowd": int(crowd[k]), "_ignore": int(ign[k])})
        for k in range(len(dt)):
            dets.append({"image_id": s + 1, "category_id": 1, "bbox": [float(v) for v in dt[k]], "score": float(len(dt) - k)})
    gt_api = ce.CocoGT(images, anns, [{"id": 1}])
    for a in gt_api.anns:
        a["ignore"] = a.pop("_ignore")                        # evaluate_img reads the flag; CocoGT alone would set it to iscrowd
    ev = ce.COCOeval(gt_api)
    ev.add_results(dets)
    dn, gn = [len(s[0]) for s in segments], [len(s[1]) for s in segments]
    dt_off, gt_off = np.r_[0, np.cumsum(dn)].astype(np.int64), np.r_[0, np.cumsum(gn)].astype(np.int64)
    D, G = int(dt_off[-1]), int(gt_off[-1])
    want_m, want_di, want_gi = np.full((A, T, D), -1, np.int32), np.zeros((A, T, D), np.uint8), np.zeros((A, G), np.uint8)
    for s, (dt, gt, area, crowd, ign) in enumerate(segments):
        ids = [a["id"] for a in ev._gts.get((s + 1, 1), [])]
        for a, rng in enumerate(ce.AREA_RNG):
            e = ev.evaluate_img(s + 1, 1, rng, 10 ** 9)
            if e is None:
                continue
            flag = np.array([1 if (ign[k] or area[k] < rng[0] or area[k] > rng[1]) else 0 for k in range(len(gt))], np.uint8)
            assert np.array_equal(np.sort(flag), np.asarray(e["gtIgnore"]).reshape(-1))       # evaluate_img's own flags, sorted
            want_gi[a, gt_off[s]:gt_off[s + 1]] = flag
            m = np.asarray(e["dtMatches"]).reshape(T, -1)
            want_m[a, :, dt_off[s]:dt_off[s + 1]] = [[ids.index(int(v)) if v else -1 for v in row] for row in m]
            want_di[a, :, dt_off[s]:dt_off[s + 1]] = np.asarray(e["dtIgnore"]).reshape(T, -1)
    cat = lambda i, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(s[i], dt).reshape((-1,) + w) for s in segments]) if segments else np.zeros((0,) + w, dt))
    inputs = {"dt_off": dt_off, "gt_off": gt_off, "dt_box": cat(0, np.float64, (4,)), "gt_box": cat(1, np.float64, (4,)),
              "gt_area": cat(2, np.float64, ()), "crowd": cat(3, np.uint8, ()), "ign": cat(4, np.uint8, ())}
    inputs["dt_area"] = np.ascontiguousarray(inputs["dt_box"][:, 2] * inputs["dt_box"][:, 3])
    return inputs, (want_m, want_di, want_gi)
