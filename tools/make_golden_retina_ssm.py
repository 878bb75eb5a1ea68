"""tests/golden/retina_ssm.npz: the reference's RetinaNet SSM tail, executed as it is (build container only).

Imports ``detection.retina_ssm`` of the reference tree on the CPU under oracle/ref_harness.py's stubs, binds the torchvision primitives the
tail calls to the restatements of oracle/make_golden_postprocess.py (both imported, neither edited), makes ``Tensor.cuda`` the identity for
the length of the call (the tail calls ``.cuda()`` on its empty accumulators) and executes ``RetinaNet.ssm_postprocess_detections`` on
  few      a few anchors, score_thresh 0.5 and one logit of exactly 0 (a score of exactly the threshold: `>` against `>=`),
  voc      a VOC-sized K = 21 head on a small pyramid,
  al1      every logit at the -4.6 prior: al = 1, no rows, no random number drawn,
  many     K = 3, one class with more than 500 candidates, some of them clipped to no width (they use up picks),
  class0   scores of 0.5 and above in class 0 only: al = 0 and every label -1.
``random`` is seeded per case; the inputs, the seed, the per-class counts, the picks the reference's shuffles produced and the rows are
recorded, beside torch's sigmoid and the decoded boxes the tail worked on (tests/_retina_ssm_restatement.py then reproduces the rows
bit for bit).  A case's seed is advanced until no score lies within 1e-5 of its threshold or of 0.5 -- scores EQUAL to one of them, which
the cases above hold by design, aside -- and no IoU the NMS met within 1e-4 of 0.5; the margins are recorded.  Arrays only; no reference
code is copied.

    python tools/make_golden_retina_ssm.py            (from the repository root)
"""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden_postprocess as mgp  # noqa: E402  (it puts the repository root first on sys.path)
ref_harness = mgp.ref_harness
import _retina_ssm_restatement as R  # noqa: E402

MIN_IOU_MARGIN, MIN_P_MARGIN = 1e-4, 1e-5
#        name      K  Hp   Wp   Hr   Wr  score_thr per_class
SPECS = [("few", 3, 32, 32, 32, 32, 0.5, 50), ("voc", 21, 64, 96, 60, 90, 0.05, 50), ("al1", 21, 64, 96, 60, 90, 0.05, 50),
         ("many", 3, 128, 128, 100, 90, 0.05, 50), ("class0", 4, 64, 64, 64, 64, 0.05, 50)]


def level_shapes(Hp, Wp):
    out, h, w = [], Hp // 8, Wp // 8
    for _ in range(5):
        out.append((max(h, 1), max(w, 1))); h, w = (h + 1) // 2, (w + 1) // 2
    return out


def inputs(name, seed, K, shapes):
    """(logits [N][K], deltas [N][4]) in anchor order."""
    rs = np.random.RandomState(seed)
    N = sum(h * w for h, w in shapes) * 9
    deltas = (rs.randn(N, 4) * 0.5).astype(np.float32)
    if name == "few":
        logits = np.full((N, K), -6.0, np.float32)
        hot = rs.choice(N, 12, replace=False)
        logits[hot[:8], 1] = (0.5 + rs.rand(8) * 3).astype(np.float32)
        logits[hot[4:], 2] = (0.5 + rs.rand(8) * 3).astype(np.float32)
        logits[hot[0], 0] = 0.0                              # exactly 0.5 = score_thresh: not a candidate
        logits[hot[11], 1] = 0.0
    elif name == "voc":
        logits = (rs.randn(N, K) * 2.0 - 4.5).astype(np.float32)
    elif name == "al1":
        logits = np.full((N, K), -4.6, np.float32)
    elif name == "many":
        logits = (rs.randn(N, K) * 2.0 + np.array([-3.0, 0.0, -5.0])).astype(np.float32)
    else:
        logits = (-2.5 + 2.0 * rs.rand(N, K)).astype(np.float32)       # scores 0.076 .. 0.38: candidates below 0.5
        logits[:, 0] = (rs.randn(N) * 2.0).astype(np.float32)
    return logits, deltas


def main():
    ref_harness.install_stubs()
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    import importlib
    import torch
    from oracle import oracle as orc
    rs_mod = importlib.import_module("detection.retina_ssm")
    mgp.bind(rs_mod.box_ops)
    met = {"iou": np.inf}
    plain_nms = rs_mod.box_ops.nms

    def recording_nms(boxes, scores, thr):         # the same greedy pass once more in numpy, to measure the margins
        _, m = R.nms_margins(boxes.numpy(), scores.numpy(), thr, 1 << 30)
        met["iou"] = min(met["iou"], m)
        return plain_nms(boxes, scores, thr)
    rs_mod.box_ops.nms = recording_nms
    drawn = {"counts": [], "picks": []}

    def recording_shuffle(x):                      # random.shuffle itself, on the global generator; what it left is written down
        drawn["counts"].append(len(x))
        random.shuffle(x)
        drawn["picks"].append(list(x[:R.TAKE]))
    rs_mod.random = types.SimpleNamespace(shuffle=recording_shuffle)

    base = np.stack([orc.base_anchors(list(s), [0.5, 1.0, 2.0]) for s in orc.retina_anchor_sizes()]).astype(np.float32)   # [5][9][4]
    blob = {"n": np.array(len(SPECS), np.int64), "base": base, "names": np.array([s[0] for s in SPECS])}
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for c, (name, K, Hp, Wp, Hr, Wr, thr, per) in enumerate(SPECS):
            rn = rs_mod.RetinaNet.__new__(rs_mod.RetinaNet)
            torch.nn.Module.__init__(rn)
            rn.box_coder = mgp.BoxCoder((1., 1., 1., 1.)); rn.score_thresh = thr; rn.nms_thresh = 0.5; rn.detections_per_img = per
            shapes = level_shapes(Hp, Wp)
            anchors = R.grid_anchors(base, shapes, Hp, Wp)
            seed = 5100 + 10 * c
            while True:
                logits, deltas = inputs(name, seed, K, shapes)
                scores = torch.sigmoid(torch.from_numpy(logits)).numpy()
                m_thr, m_half = R._away(scores, thr), R._away(scores, 0.5)
                met["iou"] = np.inf; drawn["counts"], drawn["picks"] = [], []
                random.seed(seed)
                head = {"cls_logits": torch.from_numpy(logits)[None], "bbox_regression": torch.from_numpy(deltas)[None]}
                det = rn.ssm_postprocess_detections(head, [torch.from_numpy(anchors)], [(Hr, Wr)])[0]
                if met["iou"] > MIN_IOU_MARGIN and m_thr > MIN_P_MARGIN and m_half > MIN_P_MARGIN:
                    break
                seed += 1
            al = int(det["al"])
            assert len(drawn["counts"]) == (0 if al else K)
            counts = np.array(drawn["counts"] if not al else [0] * K, np.int64)
            picks, n_picks = R.pack_picks(drawn["picks"] if not al else [[]] * K, K)
            n = det["boxes"].shape[0]
            dec = mgp.clip_boxes_to_image(rn.box_coder.decode_single(torch.from_numpy(deltas), torch.from_numpy(anchors)), (Hr, Wr)).numpy()
            off = 0
            for l, (h, w) in enumerate(shapes):
                blob["c%d_cls%d" % (c, l)] = np.ascontiguousarray(logits[off:off + h * w * 9].reshape(h, w, 9 * K))
                blob["c%d_reg%d" % (c, l)] = np.ascontiguousarray(deltas[off:off + h * w * 9].reshape(h, w, 36))
                off += h * w * 9
            blob.update({"c%d_K" % c: np.array(K, np.int64), "c%d_sizes" % c: np.array([Hp, Wp, Hr, Wr], np.int64),
                         "c%d_level_hw" % c: np.array(shapes, np.int64), "c%d_thr" % c: np.array(thr, np.float64), "c%d_per" % c: np.array(per, np.int64),
                         "c%d_seed" % c: np.array(seed, np.int64), "c%d_ref_scores" % c: scores.astype(np.float32), "c%d_ref_boxes" % c: dec.astype(np.float32),
                         "c%d_counts" % c: counts, "c%d_picks" % c: picks, "c%d_n_picks" % c: n_picks, "c%d_al" % c: np.array(al, np.int64),
                         "c%d_boxes" % c: det["boxes"].numpy().reshape(n, 4).astype(np.float32), "c%d_scores" % c: det["scores"].numpy().reshape(n).astype(np.float32),
                         "c%d_labels" % c: np.array(det["labels"], np.int8).reshape(n, K - 1),
                         "c%d_margins" % c: np.array([met["iou"], m_thr, m_half], np.float64)})
            print("case", name, "seed", seed, "al", al, "rows", n, "counts", counts.tolist(), "margins", met["iou"], m_thr, m_half)
    finally:
        torch.Tensor.cuda = real_cuda
    path = os.path.join(ROOT, "tests", "golden", "retina_ssm.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
