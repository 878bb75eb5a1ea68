"""tests/golden/ssm.npz: the reference's SSM tail and stage-2 host functions, executed as they are (build container only).

Imports ``detection.frcnn_ssm`` and ``ssm.ssm_helper`` of the reference tree on the CPU under oracle/ref_harness.py's stubs, binds the
torchvision primitives the tail calls to the restatements of oracle/make_golden_postprocess.py (imported, not edited), and executes
  * ``RoIHeads.ssm_postprocess_detections`` on random heads (R <= 300),
  * ``judge_y`` on 0, 1 and the 2 000 floats on each side of 0.5,
  * ``judge_uv`` and ``calcu_iou`` on a handful of inputs,
  * ``image_cross_validation`` on the scripted scenes of tests/_ssm_restatement.py.
Only arrays are written; no reference code is copied.  For every tail case the smallest |IoU - 0.3| the NMS met and the smallest
|p - 0.05| and |p - 0.5| are recorded, and the case's seed is advanced until they exceed 1e-4 / 1e-5 / 1e-5: no decision of the fixture
hangs on the last bit of a softmax.

    python tools/make_golden_ssm.py            (from the repository root)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden_postprocess as mgp  # noqa: E402  (it puts the repository root first on sys.path)
ref_harness = mgp.ref_harness
import _ssm_restatement as R  # noqa: E402

# (R, C, H, W, logit gain): few rows, a VOC-sized head, zero gain (every probability 1 / 21: al = 1), few classes
TAIL_SPECS = [(5, 21, 100, 100, 3.0), (120, 21, 240, 320, 3.0), (60, 21, 150, 200, 0.0), (200, 5, 300, 500, 4.0)]
MIN_IOU_MARGIN, MIN_P_MARGIN = 1e-4, 1e-5


def tail_inputs(seed, Rn, C, H, W, gain):
    rs = np.random.RandomState(seed)
    x0 = rs.rand(Rn) * W * 0.8; y0 = rs.rand(Rn) * H * 0.8
    props = np.stack([x0, y0, np.minimum(x0 + 8 + rs.rand(Rn) * W * 0.5, W), np.minimum(y0 + 8 + rs.rand(Rn) * H * 0.5, H)], 1).astype(np.float32)
    logits = (rs.randn(Rn, C) * gain).astype(np.float32)
    deltas = (rs.randn(Rn, 4 * C) * np.array([1.5, 1.5, 0.8, 0.8] * C)).astype(np.float32)
    deltas[::17, 2::4] = 30.0                      # exercises the log(1000 / 16) clamp
    return logits, deltas, props


def main():
    ref_harness.install_stubs()
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    import torch
    import importlib
    fs = importlib.import_module("detection.frcnn_ssm")
    helper = importlib.import_module("ssm.ssm_helper")
    mgp.bind(fs.box_ops)
    met = {"iou": np.inf}
    plain_nms = fs.box_ops.nms

    def recording_nms(boxes, scores, thr):         # the same greedy pass, run once more in numpy to measure the margins (boxes carry the offset)
        _, m = R.nms_margins(boxes.numpy(), scores.numpy(), 0, thr, 1 << 30)
        met["iou"] = min(met["iou"], m)
        return plain_nms(boxes, scores, thr)
    fs.box_ops.nms = recording_nms
    fs.box_ops.batched_nms = lambda b, s, i, t: (torch.empty((0,), dtype=torch.int64) if b.numel() == 0 else
                                                 fs.box_ops.nms(b + (i.to(b) * (b.max() + torch.tensor(1).to(b)))[:, None], s, t))

    rh = fs.RoIHeads()
    rh.box_coder = mgp.BoxCoder((10., 10., 5., 5.)); rh.score_thresh = 0.05; rh.nms_thresh = 0.5; rh.detections_per_img = 100
    blob = {"t_n": np.array(len(TAIL_SPECS), np.int64)}
    for k, (Rn, C, H, W, gain) in enumerate(TAIL_SPECS):
        seed = 4100 + 10 * k
        while True:
            logits, deltas, props = tail_inputs(seed, Rn, C, H, W, gain)
            p = torch.softmax(torch.from_numpy(logits), -1).numpy()[:, 1:].astype(np.float64)
            m_thr, m_half = np.abs(p - 0.05).min(), np.abs(p - 0.5).min()
            met["iou"] = np.inf
            boxes, scores, labels, al = rh.ssm_postprocess_detections(torch.from_numpy(logits), torch.from_numpy(deltas), [torch.from_numpy(props)], [(H, W)])
            if met["iou"] > MIN_IOU_MARGIN and m_thr > MIN_P_MARGIN and m_half > MIN_P_MARGIN:
                break
            seed += 1
        n = boxes[0].shape[0]
        blob.update({"t%d_logits" % k: logits, "t%d_deltas" % k: deltas, "t%d_props" % k: props, "t%d_hw" % k: np.array([H, W], np.int64),
                     "t%d_seed" % k: np.array(seed, np.int64), "t%d_al" % k: np.array(al, np.int64),
                     "t%d_boxes" % k: boxes[0].numpy().reshape(n, 4).astype(np.float32),
                     "t%d_scores" % k: scores[0].numpy().reshape(n, C - 1).astype(np.float32),
                     "t%d_labels" % k: np.array(labels[0], np.int8).reshape(n, C - 1),
                     "t%d_margins" % k: np.array([met["iou"], m_thr, m_half], np.float64)})
        print("tail case", k, "seed", seed, "al", al, "rows", n, "margins", met["iou"], m_thr, m_half)

    # judge_y: 0, 1, and the 2 000 float32 values on each side of 0.5
    half = np.float32(0.5).view(np.uint32)
    jy_in = np.concatenate([np.array([0.0, 1.0], np.float32), np.arange(int(half) - 2000, int(half) + 2001, dtype=np.uint32).view(np.float32)])
    blob["jy_in"] = jy_in
    blob["jy_out"] = np.array(fs.judge_y(torch.from_numpy(jy_in)), np.int8)

    # judge_uv: below gamma (with one loss above its lambda), above, exactly gamma, NaN
    uv = [([0.1, 0.3, 0.05], 1.0, [0.2, 0.2, 0.2]), ([0.6, 0.7, 0.1], 1.0, [0.5, 0.5, 0.5]), ([0.25, 0.25, 0.5], 1.0, [0.5, 0.5, 0.5]),
          ([np.nan, 0.1, 0.1], 1.0, [0.5, 0.5, 0.5]), ([0.0, 0.0, 0.0], 0.2, [0.1, 0.1, 0.1])]
    blob["uv_loss"] = np.array([u[0] for u in uv], np.float64); blob["uv_gamma"] = np.array([u[1] for u in uv], np.float64)
    blob["uv_lambda"] = np.array([u[2] for u in uv], np.float64)
    res = [helper.judge_uv(np.array(l, np.float64), g, np.array(c, np.float64)) for l, g, c in uv]
    blob["uv_flag"] = np.array([r[0] for r in res], np.int8); blob["uv_v"] = np.array([r[1] for r in res], np.float64)

    # calcu_iou: overlapping, identical, touching (the +1 makes them overlap), disjoint, swapped roles (the areas are not symmetric)
    pairs = [([0, 0, 10, 10], [5, 5, 15, 15]), ([2, 3, 9, 11], [2, 3, 9, 11]), ([0, 0, 10, 10], [10, 10, 20, 20]), ([0, 0, 4, 4], [20, 20, 30, 30]),
             ([5, 5, 15, 25], [0, 0, 10, 10]), ([0, 0, 10, 10], [11, 0, 20, 10]), ([1.5, 2.5, 7.25, 9.0], [3.0, 1.0, 8.5, 6.5])]
    blob["iou_a"] = np.array([p[0] for p in pairs], np.float64); blob["iou_b"] = np.array([p[1] for p in pairs], np.float64)
    blob["iou_out"] = np.array([float(helper.calcu_iou(list(a), list(b))) for a, b in pairs], np.float64)

    # image_cross_validation on the scripted scenes
    for s, scene in enumerate(R.SCENES):
        flag, score, model, state = R.run_scene(helper.image_cross_validation, scene, torch, as_float=True)
        assert all(len(c) == 1 for c in model.calls)
        blob.update({"x%d_flag" % s: np.array(flag, np.int8), "x%d_score" % s: np.array(score, np.float64), "x%d_state" % s: state,
                     "x%d_visited" % s: np.array([c[0] for c in model.calls], np.int64),
                     "x%d_pastes" % s: np.array([r for _, r in model.pastes], np.int64).reshape(-1, 4)})
        print("scene", scene["name"], flag, score, "visited", [c[0] for c in model.calls])
    blob["x_n"] = np.array(len(R.SCENES), np.int64)

    path = os.path.join(ROOT, "tests", "golden", "ssm.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
