"""COCO bounding-box AP / AR for the evaluation consumer (COCO side: detection/engine.py:178-256
``coco_evaluate`` -> detection/coco_eval.py ``CocoEvaluator`` -> pycocotools ``COCOeval``).

pycocotools is a third-party dependency of the reference that is absent from this image (no wheel, no network): **parity unpinned**.
What the reference vendors in-repo is followed where it exists -- ``CocoEvaluator.update / accumulate / summarize`` and
``prepare_for_coco_detection`` (coco_eval.py:19-98), ``loadRes`` (:242-297: result ids 1..n, area = w * h), the patched
``evaluate`` loop order (:304-348) -- and the rest restates the published algorithm of pycocotools 2.0 ``cocoeval.py``
(``computeIoU`` with crowd handling as in ``maskApi.c bbIou``, ``evaluateImg``, ``accumulate``, ``summarize``): greedy matching of
score-sorted detections per (image, category, area range) at IoU 0.50:0.05:0.95, crowd / out-of-range ground truth ignored, 101-point
interpolated precision, maxDets (1, 10, 100).  Pinned only by self-consistency and hand-computed cases (tests/test_cpu_host.py).
Only ``iou_type='bbox'`` (the detectors here produce no masks or keypoints).
"""
import numpy as np

from .voc_eval import check_matching      # the `matching` keyword is shared by the two evaluators

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]


class CocoGT(object):
    """The ground-truth side of pycocotools' COCO object as far as bbox evaluation reads it."""

    def __init__(self, images, annotations, categories):
        self.imgs = {im["id"]: im for im in images}
        self.cats = {c["id"]: c for c in categories}
        self.anns = [dict(a) for a in annotations]
        for a in self.anns:
            a["ignore"] = int(a.get("iscrowd", 0))            # COCOeval._prepare: ignore = iscrowd
            a["iscrowd"] = int(a.get("iscrowd", 0))

    def get_cat_ids(self):
        return sorted(self.cats)

    @classmethod
    def from_dataset(cls, dataset):
        """get_coco_api_from_dataset (coco_utils.py:199-208): a cald_amd.coco_utils dataset carries its annotation file; any other
        dataset is converted from its targets (convert_to_coco_api, :146-196: annotation ids from 1, xywh boxes)."""
        for _ in range(10):
            if hasattr(dataset, "anns") and hasattr(dataset, "imgs"):
                break
            if hasattr(dataset, "dataset"):
                dataset = dataset.dataset
        if hasattr(dataset, "anns") and hasattr(dataset, "imgs"):
            anns = [a for lst in dataset.anns.values() for a in lst]
            return cls(list(dataset.imgs.values()), anns, list(dataset.cats.values()) or [{"id": c} for c in sorted({a["category_id"] for a in anns})])
        images, anns, cats, ann_id = [], [], set(), 1
        for idx in range(len(dataset)):
            img, t = dataset[idx]
            image_id = int(t["image_id"].item() if hasattr(t["image_id"], "item") else t["image_id"])
            images.append({"id": image_id, "height": int(img.shape[-2]), "width": int(img.shape[-1])})
            boxes = np.asarray(t["boxes"], np.float64).reshape(-1, 4).copy()
            boxes[:, 2:] -= boxes[:, :2]
            for i in range(len(boxes)):
                lab = int(t["labels"][i])
                cats.add(lab)
                anns.append({"image_id": image_id, "bbox": boxes[i].tolist(), "category_id": lab, "area": float(t["area"][i]),
                             "iscrowd": int(t["iscrowd"][i]), "id": ann_id})
                ann_id += 1
        return cls(images, anns, [{"id": c} for c in sorted(cats)])


def bbox_iou(dts, gts, iscrowd):
    """maskApi.c bbIou on xywh boxes: [D, G] float64; against a crowd ground truth the union is the detection's own area."""
    d = np.asarray(dts, np.float64).reshape(-1, 4); g = np.asarray(gts, np.float64).reshape(-1, 4)
    if len(d) == 0 or len(g) == 0:
        return np.zeros((len(d), len(g)))
    w = np.minimum(d[:, None, 0] + d[:, None, 2], g[None, :, 0] + g[None, :, 2]) - np.maximum(d[:, None, 0], g[None, :, 0])
    h = np.minimum(d[:, None, 1] + d[:, None, 3], g[None, :, 1] + g[None, :, 3]) - np.maximum(d[:, None, 1], g[None, :, 1])
    inter = np.where((w > 0) & (h > 0), w * h, 0.0)
    da, ga = (d[:, 2] * d[:, 3])[:, None], (g[:, 2] * g[:, 3])[None, :]
    union = np.where(np.asarray(iscrowd, bool)[None, :], da + 0 * ga, da + ga - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter > 0, inter / union, 0.0)


class COCOeval(object):
    """bbox evaluation over the images seen so far; ``eval['precision']`` is [T, R, K, A, M], ``eval['recall']`` [T, K, A, M]."""

    def __init__(self, coco_gt):
        self.gt = coco_gt
        self.cat_ids = coco_gt.get_cat_ids()
        self._gts = {}
        for a in coco_gt.anns:
            self._gts.setdefault((a["image_id"], a["category_id"]), []).append(a)
        self._dts = {}
        self.img_ids = []
        self.eval, self.stats = {}, []

    def add_results(self, results):
        """loadRes (coco_eval.py:242-297): ids continue from 1, area = w * h."""
        n = sum(len(v) for v in self._dts.values())
        for k, r in enumerate(results):
            bb = r["bbox"]
            d = dict(r, area=bb[2] * bb[3], id=n + k + 1, iscrowd=0)
            self._dts.setdefault((d["image_id"], d["category_id"]), []).append(d)

    def evaluate_img(self, img_id, cat_id, a_rng, max_det):
        gt, dt = self._gts.get((img_id, cat_id), []), self._dts.get((img_id, cat_id), [])
        if len(gt) == 0 and len(dt) == 0:
            return None
        ign = np.array([1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt], dtype=np.int64)
        gtind = np.argsort(ign, kind="mergesort")
        gt = [gt[i] for i in gtind]
        gt_ig = ign[gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[:max_det]]
        iscrowd = [int(g["iscrowd"]) for g in gt]
        ious = bbox_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], iscrowd)
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm, dt_ig = np.zeros((T, G)), np.zeros((T, D)), np.zeros((T, D))
        if G and D:
            for ti, t in enumerate(IOU_THRS):
                for di, d in enumerate(dt):
                    iou, m = min(t, 1 - 1e-10), -1
                    for gi in range(G):
                        if gtm[ti, gi] > 0 and not iscrowd[gi]:
                            continue                          # already matched, and not a crowd
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gi] == 1:
                            break                             # a regular match exists; the ignored ground truth comes last
                        if ious[di, gi] < iou:
                            continue
                        iou, m = ious[di, gi], gi
                    if m == -1:
                        continue
                    dt_ig[ti, di] = gt_ig[m]; dtm[ti, di] = gt[m]["id"]; gtm[ti, m] = d["id"]
        out_rng = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape(1, D)
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(out_rng, T, 0)))
        return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}

    def evaluate(self, img_ids):
        """Per-image evaluation of `img_ids`, in the loop order of coco_eval.py:338-345; results are kept per image for accumulate()."""
        img_ids = list(np.unique(img_ids))
        max_det = MAX_DETS[-1]
        for img_id in img_ids:
            if img_id in self.img_ids:
                continue
            self.img_ids.append(img_id)
        self._eval_imgs = getattr(self, "_eval_imgs", {})
        for cat_id in self.cat_ids:
            for ai, a_rng in enumerate(AREA_RNG):
                for img_id in img_ids:
                    self._eval_imgs[(cat_id, ai, img_id)] = self.evaluate_img(img_id, cat_id, a_rng, max_det)

    def accumulate(self):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RNG), len(MAX_DETS)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        img_ids = sorted(self.img_ids)
        for k, cat_id in enumerate(self.cat_ids):
            for a in range(A):
                E = [self._eval_imgs.get((cat_id, a, i)) for i in img_ids]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                for m, max_det in enumerate(MAX_DETS):
                    dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    dt_sorted = dt_scores[inds]
                    dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q, ss = np.zeros((R,)), np.zeros((R,))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist(); q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        ri_inds = np.searchsorted(rc, REC_THRS, side="left")
                        try:
                            for ri, pi in enumerate(ri_inds):
                                q[ri] = pr[pi]; ss[ri] = dt_sorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q); scores[t, :, k, a, m] = np.array(ss)
        self.eval = {"precision": precision, "recall": recall, "scores": scores, "counts": [T, R, K, A, M]}

    def _summarize(self, ap=1, iou_thr=None, area="all", max_dets=100, quiet=False):
        aind, mind = AREA_LBL.index(area), MAX_DETS.index(max_dets)
        s = self.eval["precision"] if ap == 1 else self.eval["recall"]
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        if not quiet:
            title, typ = ("Average Precision", "(AP)") if ap == 1 else ("Average Recall", "(AR)")
            iou = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
            print(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(title, typ, iou, area, max_dets, mean_s))
        return mean_s

    def summarize(self, quiet=False):
        S = self._summarize
        self.stats = np.array([S(1, quiet=quiet), S(1, iou_thr=.5, quiet=quiet), S(1, iou_thr=.75, quiet=quiet),
                               S(1, area="small", quiet=quiet), S(1, area="medium", quiet=quiet), S(1, area="large", quiet=quiet),
                               S(0, max_dets=1, quiet=quiet), S(0, max_dets=10, quiet=quiet), S(0, max_dets=100, quiet=quiet),
                               S(0, area="small", quiet=quiet), S(0, area="medium", quiet=quiet), S(0, area="large", quiet=quiet)])
        return self.stats


def refuse_multi_rank_device_matching():
    """matching="device" evaluates on one rank only."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError('matching="device" is built for single-process evaluation; use matching="host" with world size > 1')


class _Flat(object):
    """Arrays of one evaluate() call (a segment table and, after match(), its results)."""
    pass


class FlatCOCOeval(COCOeval):
    """COCOeval with the per-(image, category) dicts replaced by flat arrays: a segment table built with numpy (one lexsort for the score
    order, the cut at maxDets), match results as [A, T, D] arrays, and a vectorised accumulate().  Same ``eval`` and ``stats``, bit for bit.

    ``matching="device"`` fills the match arrays through cald_op_coco_match (eval.hip); ``matching="host"`` fills them by calling
    COCOeval.evaluate_img per segment, which is also the route of any segment above the kernel's caps.  Image ids must be integers."""

    def __init__(self, coco_gt, matching="host"):
        check_matching(matching)
        if matching == "device":
            refuse_multi_rank_device_matching()
        COCOeval.__init__(self, coco_gt)
        self.matching = matching
        anns = [a for a in coco_gt.anns if a["category_id"] in coco_gt.cats]      # the others are never visited by evaluate()
        self._g_img = np.array([a["image_id"] for a in anns], np.int64)
        self._g_cat = np.array([a["category_id"] for a in anns], np.int64)
        self._g_box = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
        self._g_area = np.array([a["area"] for a in anns], np.float64)
        self._g_crowd = np.array([a["iscrowd"] for a in anns], np.uint8)
        self._g_ign = np.array([1 if a["ignore"] else 0 for a in anns], np.uint8)
        self._g_id = np.array([a["id"] for a in anns], np.int64)
        self._d_parts, self._d, self._n_dt = [], None, 0
        self._chunks = []
        self.host_segments = 0                                # segments matched by evaluate_img (all of them with matching="host")

    # ---- detections -------------------------------------------------------------------------------------------------------------
    def add_arrays(self, image_ids, category_ids, boxes_xywh, scores):
        """add_results on arrays: ids continue from 1, area = w * h."""
        box = np.asarray(boxes_xywh, np.float64).reshape(-1, 4)
        n = len(box)
        self._d_parts.append((np.asarray(image_ids, np.int64).reshape(n), np.asarray(category_ids, np.int64).reshape(n), box,
                              np.asarray(scores, np.float64).reshape(n), box[:, 2] * box[:, 3], self._n_dt + 1 + np.arange(n, dtype=np.int64)))
        self._n_dt += n
        self._d = None

    def add_results(self, results):
        self.add_arrays([r["image_id"] for r in results], [r["category_id"] for r in results], [r["bbox"] for r in results],
                        [r["score"] for r in results])

    def add_predictions(self, predictions):
        """CocoEvaluator.prepare_for_coco_detection + add_results without the list of dicts (same float64 values)."""
        img, cat, box, score = [], [], [], []
        for original_id, p in predictions.items():
            if len(p) == 0:
                continue
            b = convert_to_xywh(p["boxes"].cpu().numpy() if hasattr(p["boxes"], "cpu") else p["boxes"])
            box.append(b); img.append(np.full(len(b), original_id, np.int64))
            score.append(np.asarray(p["scores"].cpu().numpy() if hasattr(p["scores"], "cpu") else p["scores"], np.float64).reshape(len(b)))
            cat.append(np.asarray(p["labels"].cpu().numpy() if hasattr(p["labels"], "cpu") else p["labels"], np.int64).reshape(len(b)))
        if box:
            self.add_arrays(np.concatenate(img), np.concatenate(cat), np.concatenate(box), np.concatenate(score))

    def _dt_arrays(self):
        if self._d is None:
            parts = self._d_parts or [(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros(0), np.zeros(0), np.zeros(0, np.int64))]
            self._d = tuple(np.concatenate([p[i] for p in parts]) for i in range(6))
            self._d_parts = [self._d]
        return self._d

    # ---- evaluate = segment table + matching ------------------------------------------------------------------------------------
    def segment_table(self, img_ids):
        """The segments = (category, image) pairs of `img_ids` that hold a ground truth or a detection, in (category, image id) order;
        per segment its detections in evaluate_img's order (stable by descending score, cut at maxDets) and its ground truths in
        annotation order."""
        d_img, d_cat, d_box, d_score, d_area, d_id = self._dt_arrays()
        tab = _Flat()
        tab.img_ids = np.unique(np.asarray(img_ids, np.int64))
        cats, n_img = np.asarray(self.cat_ids, np.int64), len(tab.img_ids)
        dall = np.flatnonzero(np.isin(d_img, tab.img_ids) & np.isin(d_cat, cats))
        dkey = np.searchsorted(cats, d_cat[dall]) * n_img + np.searchsorted(tab.img_ids, d_img[dall])
        order = np.lexsort((-d_score[dall], dkey))            # stable: equal scores keep their insertion order
        dall, dkey = dall[order], dkey[order]
        first = np.flatnonzero(np.r_[True, dkey[1:] != dkey[:-1]]) if len(dkey) else np.zeros(0, np.int64)
        rank = np.arange(len(dkey)) - np.repeat(first, np.diff(np.r_[first, len(dkey)]))
        keep = rank < MAX_DETS[-1]
        gsel = np.flatnonzero(np.isin(self._g_img, tab.img_ids))
        gkey = np.searchsorted(cats, self._g_cat[gsel]) * n_img + np.searchsorted(tab.img_ids, self._g_img[gsel])
        order = np.argsort(gkey, kind="stable")
        gsel, gkey = gsel[order], gkey[order]
        seg = np.union1d(dkey, gkey)
        tab.seg_cat, tab.seg_img = seg // max(n_img, 1), tab.img_ids[seg % max(n_img, 1)] if n_img else np.zeros(0, np.int64)
        tab.dall, tab.all_off = dall, np.r_[np.searchsorted(dkey, seg), len(dkey)]                # before the cut (the host route's input)
        tab.dsel, tab.dt_rank = dall[keep], rank[keep]
        tab.dt_off = np.r_[np.searchsorted(dkey[keep], seg), len(tab.dsel)].astype(np.int64)
        tab.gsel, tab.gt_off = gsel, np.r_[np.searchsorted(gkey, seg), len(gsel)].astype(np.int64)
        tab.dt_score = d_score[tab.dsel]
        return tab

    def match(self, tab):
        """Fills tab.dt_gid [A, T, D] (id of the matched ground truth, 0 = none), tab.dt_ig [A, T, D] and tab.gt_ig [A, G]."""
        A, T, D, G, S = len(AREA_RNG), len(IOU_THRS), len(tab.dsel), len(tab.gsel), len(tab.seg_cat)
        rng = np.asarray(AREA_RNG, np.float64)
        g_area = self._g_area[tab.gsel]
        tab.gt_ig = (self._g_ign[tab.gsel][None, :] != 0) | (g_area[None, :] < rng[:, :1]) | (g_area[None, :] > rng[:, 1:])
        tab.dt_gid, tab.dt_ig = np.zeros((A, T, D), np.int64), np.zeros((A, T, D), bool)
        host = np.ones(S, bool)
        if self.matching == "device" and S:
            from . import _ffi
            host = (np.diff(tab.dt_off) > _ffi.EVAL_MAX_DT) | (np.diff(tab.gt_off) > _ffi.EVAL_MAX_GT)
            self._match_device(tab, ~host, rng)
        for s in np.flatnonzero(host):
            self._match_host(tab, int(s))
        self.host_segments += int(host.sum())
        return tab

    def _match_device(self, tab, dev, rng):
        import ctypes as C
        from . import _ffi, detector
        ctx = detector.get_ctx()                              # raises without a GPU: there is no silent host route
        A, T = len(AREA_RNG), len(IOU_THRS)
        d_img, d_cat, d_box, d_score, d_area, d_id = self._dt_arrays()
        dn, gn = np.diff(tab.dt_off), np.diff(tab.gt_off)
        drow, grow = np.repeat(dev, dn), np.repeat(dev, gn)   # the rows of the segments that go to the device
        dsel, gsel = tab.dsel[drow], tab.gsel[grow]
        dt_off = np.r_[0, np.cumsum(dn[dev])].astype(np.int64); gt_off = np.r_[0, np.cumsum(gn[dev])].astype(np.int64)
        D, G, S = len(dsel), len(gsel), int(dev.sum())
        dt_box, dt_area = np.ascontiguousarray(d_box[dsel]), np.ascontiguousarray(d_area[dsel])
        gt_box, gt_area = np.ascontiguousarray(self._g_box[gsel]), np.ascontiguousarray(self._g_area[gsel])
        crowd, ign = np.ascontiguousarray(self._g_crowd[gsel]), np.ascontiguousarray(self._g_ign[gsel])
        thrs, rng = np.ascontiguousarray(IOU_THRS, np.float64), np.ascontiguousarray(rng)
        pos, dt_ig, gt_ig = np.full((A, T, D), -1, np.int32), np.zeros((A, T, D), np.uint8), np.zeros((A, G), np.uint8)
        _ffi.check(_ffi.lib().cald_op_coco_match(ctx, S, _ffi.ptr(dt_off, _ffi.c_i64), _ffi.ptr(gt_off, _ffi.c_i64), _ffi.ptr(dt_box, _ffi.c_d),
                                                 _ffi.ptr(dt_area, _ffi.c_d), _ffi.ptr(gt_box, _ffi.c_d), _ffi.ptr(gt_area, _ffi.c_d),
                                                 _ffi.ptr(crowd, _ffi.c_u8), _ffi.ptr(ign, _ffi.c_u8), T, _ffi.ptr(thrs, _ffi.c_d), A, _ffi.ptr(rng, _ffi.c_d),
                                                 _ffi.ptr(pos, C.POINTER(C.c_int32)), _ffi.ptr(dt_ig, _ffi.c_u8), _ffi.ptr(gt_ig, _ffi.c_u8)))
        g_id = self._g_id[gsel]
        base = np.repeat(gt_off[:-1], dn[dev])                # first ground-truth row of each detection's segment
        hit = pos >= 0
        gid = np.where(hit, g_id[np.where(hit, base[None, None, :] + pos, 0)] if G else 0, 0)
        dt_ig = dt_ig != 0
        if G and (g_id == 0).any():                           # an annotation with id 0 reads as "unmatched" in evaluate_img's last line
            out_rng = (dt_area[None, :] < rng[:, :1]) | (dt_area[None, :] > rng[:, 1:])
            dt_ig |= hit & (gid == 0) & out_rng[:, None, :]
        tab.dt_gid[:, :, drow], tab.dt_ig[:, :, drow], tab.gt_ig[:, grow] = gid, dt_ig, gt_ig != 0

    def _match_host(self, tab, s):
        d_img, d_cat, d_box, d_score, d_area, d_id = self._dt_arrays()
        img, cat = int(tab.seg_img[s]), self.cat_ids[int(tab.seg_cat[s])]
        rows = np.sort(tab.dall[tab.all_off[s]:tab.all_off[s + 1]])               # insertion order, before the cut
        self._dts[(img, cat)] = [{"image_id": img, "category_id": cat, "bbox": d_box[i].tolist(), "score": float(d_score[i]),
                                  "area": float(d_area[i]), "id": int(d_id[i]), "iscrowd": 0} for i in rows]
        d0, d1 = int(tab.dt_off[s]), int(tab.dt_off[s + 1])
        for a, a_rng in enumerate(AREA_RNG):
            e = self.evaluate_img(img, cat, a_rng, MAX_DETS[-1])
            tab.dt_gid[a, :, d0:d1], tab.dt_ig[a, :, d0:d1] = e["dtMatches"], e["dtIgnore"]

    def evaluate(self, img_ids):
        self.keep(self.match(self.segment_table(img_ids)))

    def keep(self, tab):
        """Files a matched table for accumulate()."""
        for img_id in tab.img_ids.tolist():
            if img_id not in self.img_ids:
                self.img_ids.append(img_id)
        for old in self._chunks:                              # an image evaluated again replaces its earlier result
            old.alive &= ~np.isin(old.seg_img, tab.img_ids)
        tab.alive = np.ones(len(tab.seg_cat), bool)
        self._chunks.append(tab)

    # ---- accumulate -------------------------------------------------------------------------------------------------------------
    def accumulate(self):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RNG), len(MAX_DETS)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        # all live segments, their detections in (category, image id, score order): the order COCOeval.accumulate concatenates them in
        dcat, dimg, drank, dscore, dgid, dig, gcat, gig, scat = [], [], [], [], [], [], [], [], []
        for c in self._chunks:
            dn, gn = np.diff(c.dt_off), np.diff(c.gt_off)
            drow, grow = np.repeat(c.alive, dn), np.repeat(c.alive, gn)
            dcat.append(np.repeat(c.seg_cat, dn)[drow]); dimg.append(np.repeat(c.seg_img, dn)[drow]); drank.append(c.dt_rank[drow])
            dscore.append(c.dt_score[drow]); dgid.append(c.dt_gid[:, :, drow] != 0); dig.append(c.dt_ig[:, :, drow])
            gcat.append(np.repeat(c.seg_cat, gn)[grow]); gig.append(c.gt_ig[:, grow]); scat.append(c.seg_cat[c.alive])
        if self._chunks:
            dcat, dimg, drank, dscore, gcat, scat = [np.concatenate(x) for x in (dcat, dimg, drank, dscore, gcat, scat)]
            dgid, dig, gig = np.concatenate(dgid, axis=2), np.concatenate(dig, axis=2), np.concatenate(gig, axis=1)
            order = np.lexsort((drank, dimg, dcat))
            dcat, drank, dscore, dgid, dig = dcat[order], drank[order], dscore[order], dgid[:, :, order], dig[:, :, order]
            order = np.argsort(gcat, kind="stable")
            gcat, gig = gcat[order], gig[:, order]
            d_lo, d_hi = np.searchsorted(dcat, np.arange(K)), np.searchsorted(dcat, np.arange(K), side="right")
            g_lo, g_hi = np.searchsorted(gcat, np.arange(K)), np.searchsorted(gcat, np.arange(K), side="right")
            n_seg = np.bincount(scat, minlength=K)
        for k in range(K if self._chunks else 0):
            if n_seg[k] == 0:
                continue
            npig_a = np.count_nonzero(~gig[:, g_lo[k]:g_hi[k]], axis=1)
            va = np.flatnonzero(npig_a)                       # an area range without a regular ground truth keeps its -1
            if len(va) == 0:
                continue
            npig = npig_a[va].astype(dtype=float)[:, None, None]
            # searchsorted(rc, REC_THRS, 'left') without a call per row.  rc = tp / npig is monotone in the integer count tp, so the first
            # rc >= thr is the first tp >= c(thr), the least count whose quotient -- the same division -- reaches thr.
            c_thr = np.stack([np.searchsorted(np.arange(n + 1).astype(dtype=float) / n, REC_THRS, side="left") for n in npig_a[va]])
            rows = len(va) * T                                # one row per (area range, threshold)
            lo, hi = d_lo[k], d_hi[k]
            k_score, k_gid, k_ig = dscore[lo:hi], dgid[:, :, lo:hi][va], dig[:, :, lo:hi][va]
            for m, max_det in enumerate(MAX_DETS):
                sel = np.flatnonzero(drank[lo:hi] < max_det)
                sel = sel[np.argsort(-k_score[sel], kind="mergesort")]
                dt_sorted, nd = k_score[sel], len(sel)
                if nd == 0:
                    recall[:, k, va, m], precision[:, :, k, va, m], scores[:, :, k, va, m] = 0, 0, 0
                    continue
                dtm, ig = k_gid[:, :, sel], k_ig[:, :, sel]
                tp_int = np.cumsum(dtm & ~ig, axis=2)
                tp_sum, fp_sum = tp_int.astype(dtype=float), np.cumsum(~dtm & ~ig, axis=2).astype(dtype=float)
                rc = tp_sum / npig
                pr = tp_sum / (fp_sum + tp_sum + np.spacing(1))
                recall[:, k, va, m] = rc[:, :, -1].T
                pr = np.maximum.accumulate(pr[:, :, ::-1], axis=2)[:, :, ::-1]       # the precision envelope: running max from the right (exact)
                # shifting row r by r * (nd + 1) keeps the rows' count ranges apart, so one search over the flattened counts serves every
                # row; a count no detection reaches lands on the next row's start, i.e. on nd
                shift = np.arange(rows)[:, None] * (nd + 1)
                want = np.repeat(np.minimum(c_thr, nd + 1), T, axis=0)
                ri = np.searchsorted((tp_int.reshape(rows, nd) + shift).ravel(), (want + shift).ravel(), side="left").reshape(rows, R)
                ri -= np.arange(rows)[:, None] * nd
                ok = ri < nd                                  # past the last detection the host loop stops and leaves zeros
                ri = np.minimum(ri, nd - 1)
                p = np.where(ok, np.take_along_axis(pr.reshape(rows, nd), ri, axis=1), 0.0).reshape(len(va), T, R)
                precision[:, :, k, va, m] = p.transpose(1, 2, 0)
                scores[:, :, k, va, m] = np.where(ok, dt_sorted[ri], 0.0).reshape(len(va), T, R).transpose(1, 2, 0)
        self.eval = {"precision": precision, "recall": recall, "scores": scores, "counts": [T, R, K, A, M]}


def convert_to_xywh(boxes):
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)


class CocoEvaluator(object):
    """detection/coco_eval.py:19-64 for iou_types == ['bbox'].  ``matching="device"`` evaluates through FlatCOCOeval and the HIP matching
    kernel (same numbers, bit for bit); the default ``"host"`` is COCOeval."""

    def __init__(self, coco_gt, iou_types=("bbox",), matching="host"):
        assert list(iou_types) == ["bbox"], "only bounding-box evaluation is built"
        check_matching(matching)
        self.coco_gt, self.iou_types, self.matching = coco_gt, list(iou_types), matching
        self.coco_eval = {"bbox": FlatCOCOeval(coco_gt, matching="device") if matching == "device" else COCOeval(coco_gt)}
        self.img_ids = []

    @staticmethod
    def prepare_for_coco_detection(predictions):
        """coco_eval.py:76-98."""
        out = []
        for original_id, p in predictions.items():
            if len(p) == 0:
                continue
            boxes = convert_to_xywh(p["boxes"].cpu().numpy() if hasattr(p["boxes"], "cpu") else p["boxes"]).tolist()
            scores = [float(s) for s in p["scores"]]; labels = [int(l) for l in p["labels"]]
            out.extend({"image_id": original_id, "category_id": labels[k], "bbox": box, "score": scores[k]} for k, box in enumerate(boxes))
        return out

    def update(self, predictions):
        img_ids = list(np.unique(list(predictions.keys())))
        self.img_ids.extend(img_ids)
        ev = self.coco_eval["bbox"]
        if self.matching == "device":
            ev.add_predictions(predictions)
        else:
            ev.add_results(self.prepare_for_coco_detection(predictions))
        ev.evaluate(img_ids)

    def synchronize_between_processes(self):
        pass                                                  # single process (cald_train.py evaluates on one rank)

    def accumulate(self):
        self.coco_eval["bbox"].accumulate()

    def summarize(self):
        print("IoU metric: bbox")
        return self.coco_eval["bbox"].summarize()
