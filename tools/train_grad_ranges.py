"""The range of every data gradient's input over a soak of the training step: what the gradient exponents of backward_precision="f16x3"
(one G per layer and pyramid level, fixed between refreshes) have to cover.  tools/soak_train.py's configuration (batches of 1..6 VOC-sized
images, 1..11 boxes, lr 2e-5, momentum 0.9); every step is made a calibration step, so its data gradients are the exact ones and the
largest |g| of each data gradient's input is read back after it.

    python tools/train_grad_ranges.py [--steps 300] [--out profiles/train_f16x3_backward_ranges.json]

Per launch (layer, level): max |g| at step 0 -- what a refresh at that step would derive G from -- and the smallest / largest later maximum
relative to it.  A G derived at step 0 overflows fp16 when a later maximum exceeds 32 x that of step 0, and loses bits of the tensor's
largest entry below 2^-13 x.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cald_amd import synth, train
from cald_amd import train_ops as ops


def run(model, steps, seed=1):
    sd = synth.pseudo_trained_retinanet(21, 50, seed=0) if model == "retinanet" else synth.pseudo_trained_frcnn(21, 50, seed=0)
    kw = dict(min_size=600, max_size=1000, backward_precision="f16x3")
    net = (train.RetinaNetTrainer(sd, 21, **kw) if model == "retinanet"
           else train.FasterRCNNTrainer(sd, 21, generator=torch.Generator().manual_seed(seed), **kw))
    mdl = train.TrainableDetector(net)
    opt = train.SGD([p for p in mdl.parameters() if p.requires_grad], lr=2e-5, momentum=0.9, weight_decay=1e-4, net=net)
    rs = np.random.RandomState(seed)
    pool = synth.make_pool(24, "voc", seed)
    series, losses = {}, []
    for it in range(steps):
        bs = int(rs.choice([1, 2, 4, 4, 4, 6]))
        idx = rs.choice(len(pool), bs, replace=False)
        ims, tgs = [], []
        for i in idx:
            im = pool[i]; H, W = im.shape[:2]
            k = int(rs.randint(1, 12))
            x0 = rs.rand(k) * W * 0.7; y0 = rs.rand(k) * H * 0.7
            boxes = np.stack([x0, y0, np.minimum(x0 + W * (0.05 + 0.4 * rs.rand(k)), W - 1), np.minimum(y0 + H * (0.05 + 0.4 * rs.rand(k)), H - 1)], axis=1).astype(np.float32)
            ims.append(torch.from_numpy(im).cuda()); tgs.append({"boxes": torch.from_numpy(boxes), "labels": torch.from_numpy(rs.randint(1, 21, k).astype(np.int64))})
        net._calib = []                                   # this backward: exact data gradients, the maxima collected
        loss = sum(mdl(ims, tgs).values())
        opt.zero_grad(); loss.backward(); opt.step()
        losses.append(float(loss.detach()))
        for key, m in net._grad_max.items():
            series.setdefault(key, []).append(float(m))
    rows = {}
    for (ci, lvl), v in sorted(series.items()):
        v = np.asarray(v, np.float64)
        first = v[0]
        pos = v[v > 0]
        rows["%s level %d" % (net.convs[ci].name, lvl)] = {
            "max_abs_step0": first, "G_step0": ops.f16x3_grad_scale(first)[0], "steps_seen": int(len(v)),
            "min_over_steps": float(pos.min()) if len(pos) else 0.0, "max_over_steps": float(v.max()),
            "growth_vs_step0": float(v.max() / first) if first > 0 else None,
            "shrink_vs_step0": float(pos.min() / first) if first > 0 and len(pos) else None,
            "all_zero_steps": int((v == 0).sum())}
    gr = [r["growth_vs_step0"] for r in rows.values() if r["growth_vs_step0"] is not None]
    sh = [r["shrink_vs_step0"] for r in rows.values() if r["shrink_vs_step0"] is not None]
    return {"steps": steps, "launches": len(rows), "loss_first": losses[0], "loss_last": losses[-1], "finite": bool(np.all(np.isfinite(losses))),
            "worst_growth_vs_step0": max(gr), "worst_shrink_vs_step0": min(sh),
            "growth_beyond_x32_headroom": bool(max(gr) > 32.0), "shrink_beyond_2^-13": bool(min(sh) < 2.0 ** -13),
            "per_launch": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"what": "per data-gradient launch (layer, pyramid level) the largest |g| of the launch's input over %d steps of tools/soak_train.py's "
                   "configuration (R50, min_size 600 / max_size 1000, batches of 1..6 images, lr 2e-5), every step run as a calibration step; "
                   "growth / shrink are relative to step 0, where a refresh would have fixed G (target max |g| 2^(4+G) in [2^10, 2^11): "
                   "x 32 of growth before fp16 overflows, x 2^13 of shrink before the largest entry loses a bit)" % a.steps,
           "detectors": {m: run(m, a.steps) for m in ("frcnn", "retinanet")}}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({m: {k: v for k, v in r.items() if k != "per_launch"} for m, r in out["detectors"].items()}))


if __name__ == "__main__":
    main()
