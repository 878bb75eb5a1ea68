"""Host against device matching in the two AP evaluators (matching="host" / matching="device"), stage by stage, on one MI355X.

A COCO-shaped set (seeded: `--images` images x 80 categories, 100 detections an image, about 7 ground truths an image, some crowds) goes
through COCOeval (the host path: the code of the commit before the device path existed) and through FlatCOCOeval(matching="device"); a
VOC-shaped set (20 classes, `--voc-images` images, `--voc-dets` detections a class, three-decimal scores) goes through voc_eval's host
functions and through match_device.  Both start from what the engine hands an evaluator: prediction dicts / results files.

    stage           host                                              device
    segment table   prepare_for_coco_detection + add_results          add_predictions + segment_table
    matching        COCOeval.evaluate (evaluate_img per segment)      match (cald_op_coco_match: upload, kernel, download, ids)
    accumulate      COCOeval.accumulate                               FlatCOCOeval.accumulate (vectorised)
    VOC read        read_detections                                   read_detections (the same call)
    VOC matching    best_overlaps + 10 x mark_detections              match_device (grouping, cald_op_voc_match)
    VOC curves      _curve x 10                                       _curve x 10 (the same call)

The two paths are alternated `--rounds` times in one process after one warm-up of each; every stage is timed with the host clock between
device synchronisations; medians and the min / max over the rounds are written.  The results are compared for equality in every round.
`--flat-host` times FlatCOCOeval's host route in place of the device (needs no GPU, writes no file): a rehearsal of this script and a
measure of the vectorised accumulate alone, not a measurement of the device path.

    python tools/bench_eval.py [--images 500] [--voc-images 2000] [--voc-dets 10000] [--rounds 3] [--out profiles/eval_match_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cald_amd import coco_eval as ce, voc_eval as ve


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


class Stages(object):
    def __init__(self):
        self.t = {}

    def run(self, name, fn):
        sync(); t0 = time.perf_counter()
        out = fn()
        sync(); self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
        return out


def coco_set(n_img, seed):
    rs = np.random.RandomState(seed)
    images = [{"id": 1000 + i} for i in range(n_img)]
    cats = [{"id": c} for c in range(1, 81)]
    anns, preds = [], {}
    for im in images:
        G = rs.randint(1, 14)
        gxy, gwh = rs.randint(0, 500, (G, 2)).astype(np.float64), rs.randint(8, 220, (G, 2)).astype(np.float64)
        gcat = rs.randint(1, 81, G) if rs.rand() < 0.5 else rs.choice(rs.randint(1, 81, 3), G)        # images of a few categories, as in COCO
        for k in range(G):
            anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": int(gcat[k]), "bbox": [gxy[k, 0], gxy[k, 1], gwh[k, 0], gwh[k, 1]],
                         "area": float(gwh[k, 0] * gwh[k, 1] * rs.uniform(0.4, 1.0)), "iscrowd": int(rs.rand() < 0.03)})
        src = rs.randint(0, G, 100)
        near = rs.rand(100) < 0.7                             # 70 detections jitter a ground truth and carry its label, 30 are clutter
        xy = np.where(near[:, None], gxy[src] + rs.normal(0, 6, (100, 2)), rs.randint(0, 500, (100, 2)))
        wh = np.where(near[:, None], gwh[src] * rs.uniform(0.8, 1.25, (100, 2)), rs.randint(8, 220, (100, 2)))
        lab = np.where(near, gcat[src], rs.randint(1, 81, 100))
        b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        preds[im["id"]] = {"boxes": torch.from_numpy(b), "scores": torch.from_numpy(np.sort(rs.rand(100).astype(np.float32))[::-1].copy()),
                           "labels": torch.from_numpy(lab.astype(np.int64))}
    return images, anns, cats, preds


def coco_host(gt, preds, st):
    ev = ce.COCOeval(gt)
    st.run("segment table", lambda: ev.add_results(ce.CocoEvaluator.prepare_for_coco_detection(preds)))
    st.run("matching", lambda: ev.evaluate(list(preds)))
    st.run("accumulate", ev.accumulate)
    ev.summarize(quiet=True)
    return ev


def coco_flat(gt, preds, st, matching):
    ev = ce.FlatCOCOeval(gt, matching=matching)

    def table():
        ev.add_predictions(preds)
        return ev.segment_table(list(preds))
    tab = st.run("segment table", table)

    st.run("matching", lambda: ev.keep(ev.match(tab)))
    st.run("accumulate", ev.accumulate)
    ev.summarize(quiet=True)
    return ev, len(tab.seg_cat), len(tab.dsel)


def voc_set(n_img, n_det, n_cls, seed, out_dir):
    rs = np.random.RandomState(seed)
    names = ["%06d" % i for i in range(n_img)]
    ann = ve.VocAnnotations.__new__(ve.VocAnnotations)
    ann.imagenames, ann.recs, ann._per_class = names, {}, {}
    files = []
    for c in range(n_cls):
        table, npos = {}, 0
        has = rs.rand(n_img) < 0.25
        for i, n in enumerate(names):
            G = rs.randint(1, 5) if has[i] else 0
            xy = rs.randint(1, 300, (G, 2))
            table[n] = (np.concatenate([xy, xy + rs.randint(20, 200, (G, 2))], 1).astype(float).reshape(G, 4) if G else np.array([]).astype(float),
                        (rs.rand(G) < 0.15).astype(bool))
            npos += int(np.sum(~table[n][1]))
        ann._per_class["c%02d" % c] = (table, npos)
        with_gt = np.flatnonzero(has)
        lines = []
        for _ in range(n_det):
            if rs.rand() < 0.6:
                n = names[with_gt[rs.randint(len(with_gt))]]
                g = table[n][0][rs.randint(len(table[n][0]))]
                b = g + rs.normal(0, 8, 4)
            else:
                n = names[rs.randint(n_img)]
                xy = rs.randint(1, 300, 2)
                b = np.r_[xy, xy + rs.randint(20, 200, 2)]
            lines.append("%s %.3f %.1f %.1f %.1f %.1f\n" % (n, rs.rand(), b[0], b[1], max(b[2], b[0] + 1), max(b[3], b[1] + 1)))
        files.append(os.path.join(out_dir, "det_test_c%02d.txt" % c))
        with open(files[-1], "w") as f:
            f.write("".join(lines))
    return ann, files


def voc_run(ann, files, st, device):
    out = []
    for c, fn in enumerate(files):
        table, npos = ann.of_class("c%02d" % c)
        image_ids, BB = st.run("VOC read", lambda: ve.read_detections(fn))
        if device:
            _, _, tp, fp = st.run("VOC matching", lambda: ve.match_device(image_ids, BB, table, ve.IOU_THRESHOLDS))
            marks = [(tp[i], fp[i]) for i in range(len(tp))]
        else:
            def host():
                ovmax, jmax = ve.best_overlaps(image_ids, BB, table)
                return [ve.mark_detections(image_ids, ovmax, jmax, table, t) for t in ve.IOU_THRESHOLDS]
            marks = st.run("VOC matching", host)
        out.append(st.run("VOC curves", lambda: [ve._curve(tp, fp, npos, False) for tp, fp in marks]))
    return out


def same_voc(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and repr(x[2]) == repr(y[2]) for ca, cb in zip(a, b) for x, y in zip(ca, cb))


def summary(rounds_host, rounds_dev, names):
    out = {}
    for n in names + ["total"]:
        h = [sum(r[k] for k in names) if n == "total" else r[n] for r in rounds_host]
        d = [sum(r[k] for k in names) if n == "total" else r[n] for r in rounds_dev]
        out[n] = {"host_s": float(np.median(h)), "host_min_max_s": [min(h), max(h)], "device_s": float(np.median(d)), "device_min_max_s": [min(d), max(d)],
                  "host_over_device": float(np.median(h) / np.median(d))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500); ap.add_argument("--voc-images", type=int, default=2000)
    ap.add_argument("--voc-dets", type=int, default=10000); ap.add_argument("--voc-classes", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--flat-host", action="store_true", help="rehearsal without a GPU: FlatCOCOeval's host route, COCO only, no file written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_match_bench.json"))
    a = ap.parse_args()
    if not a.flat_host and not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on an MI355X; --flat-host rehearses the script without one")
    matching = "host" if a.flat_host else "device"
    images, anns, cats, preds = coco_set(a.images, a.seed)
    gt = ce.CocoGT(images, anns, cats)
    C = ["segment table", "matching", "accumulate"]
    host_rounds, dev_rounds, equal = [], [], True
    for r in range(a.rounds + 1):                             # round 0 warms both paths up and is not kept
        sh, sd = Stages(), Stages()
        want = coco_host(gt, preds, sh)
        got, n_seg, n_dt = coco_flat(gt, preds, sd, matching)
        equal &= all(np.array_equal(got.eval[k], want.eval[k]) for k in ("precision", "recall", "scores")) and np.array_equal(got.stats, want.stats)
        assert equal, "the two paths differ"
        if r:
            host_rounds.append(sh.t); dev_rounds.append(sd.t)
        print("coco round %d  host %s  |  %s %s" % (r, {k: round(v, 4) for k, v in sh.t.items()}, matching, {k: round(v, 4) for k, v in sd.t.items()}), flush=True)
    res = {"coco": {"images": a.images, "categories": 80, "detections": n_dt, "ground_truths": len(anns), "segments": n_seg,
                    "host_route_segments": got.host_segments, "AP": float(want.stats[0]), "stages": summary(host_rounds, dev_rounds, C)}}
    if a.flat_host:
        print(json.dumps(res, indent=1))
        return
    V = ["VOC read", "VOC matching", "VOC curves"]
    with tempfile.TemporaryDirectory() as tmp:
        ann, files = voc_set(a.voc_images, a.voc_dets, a.voc_classes, a.seed + 1, tmp)
        host_rounds, dev_rounds = [], []
        with np.errstate(all="ignore"):
            for r in range(a.rounds + 1):
                sh, sd = Stages(), Stages()
                want_v, got_v = voc_run(ann, files, sh, False), voc_run(ann, files, sd, True)
                equal &= same_voc(want_v, got_v)
                assert equal, "the two VOC paths differ"
                if r:
                    host_rounds.append(sh.t); dev_rounds.append(sd.t)
                print("voc round %d  host %s  |  device %s" % (r, {k: round(v, 4) for k, v in sh.t.items()}, {k: round(v, 4) for k, v in sd.t.items()}), flush=True)
    res["voc"] = {"classes": a.voc_classes, "images": a.voc_images, "detections_per_class": a.voc_dets,
                  "mAP50": float(np.nanmean([c[0][2] for c in want_v])), "stages": summary(host_rounds, dev_rounds, V)}
    res.update({"rounds": a.rounds, "results_equal": bool(equal), "device": torch.cuda.get_device_name(0), "clock": "time.perf_counter between device synchronisations",
                "note": "host = the host path (COCOeval / best_overlaps + mark_detections); medians over the rounds after one warm-up round of each path"})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
