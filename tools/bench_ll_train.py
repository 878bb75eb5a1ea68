"""What training LossNet beside the detector costs per step on one MI355X (ll_train.py:73-141): milliseconds per step of forward + backward
+ SGD at the reference's training configuration (batch 4, VOC-sized images at min_size 600 / max_size 1000, 2 000 proposals, 512 RoIs
per image) for

    plain      FasterRCNNTrainer as cald_train.py uses it: four scalar losses (--model retinanet: RetinaNetTrainer, two)
    detached   loss_mode="ll" (--model retinanet: RetinaNetLLTrainer), features detached (the reference's default, task_epochs = 0): per-image losses, cald_train_gap, LossNet forward /
               backward, LossPredLoss, a second fused SGD launch
    live       loss_mode="ll", LossNet's gradient enters the pyramid through the broadcast join (task_epochs > epoch)

alternated ``--rounds`` times in ONE process (so that clock and thermal drift hit the three alike); each block is timed with HIP events
between two synchronisations.  Writes the per-block times, their means and spreads and the differences to ``--out``.

    python tools/bench_ll_train.py [--model faster_rcnn|retinanet] [--steps 10] [--warmup 3] [--rounds 3] [--out profiles/ll_train_bench.json]

--model retinanet writes profiles/ll_train_bench_retinanet.json unless --out says otherwise.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cald_amd import ll_train, synth, train


def batches_of(batch):
    from torch.utils.data.sampler import SequentialSampler
    from cald_amd.group_by_aspect_ratio import GroupedBatchSampler, _quantize
    sizes = synth.pool_sizes(16 * batch, "voc", 0)
    groups = _quantize([float(w) / float(h) for h, w in sizes], (2 ** np.linspace(-1, 1, 7)).tolist())
    picked = [b for _, b in zip(range(2), GroupedBatchSampler(SequentialSampler(sizes), groups, batch))]
    imgs = [synth.synth_image(i, sizes[i][0], sizes[i][1]) for b in picked for i in b]
    rs = np.random.RandomState(0)
    out = []
    for b in range(2):
        ims, tgs = [], []
        for im in imgs[b * batch:(b + 1) * batch]:
            H, W = im.shape[:2]
            x0 = rs.rand(3) * W * 0.6; y0 = rs.rand(3) * H * 0.6
            boxes = np.stack([x0, y0, x0 + W * 0.3, y0 + H * 0.3], axis=1).astype(np.float32)
            ims.append(torch.from_numpy(im).cuda())
            tgs.append({"boxes": torch.from_numpy(boxes), "labels": torch.from_numpy(rs.randint(1, 21, 3).astype(np.int64))})
        out.append((ims, tgs))
    return out


class Mode(object):
    def __init__(self, name, batch, model="faster_rcnn"):
        self.name, self.retina = name, model == "retinanet"
        if self.retina:
            sd = synth.pseudo_trained_retinanet(21, 50, seed=0)
            self.net = (train.RetinaNetTrainer if name == "plain" else train.RetinaNetLLTrainer)(sd, 21, min_size=600, max_size=1000)
        else:
            sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
            self.net = train.FasterRCNNTrainer(sd, 21, min_size=600, max_size=1000, generator=torch.Generator().manual_seed(0),
                                               loss_mode=None if name == "plain" else "ll")
        self.model = train.TrainableDetector(self.net)
        self.opt = train.SGD(self.model.parameters(), lr=1e-5, momentum=0.9, weight_decay=1e-4, net=self.net)
        if name != "plain":
            torch.manual_seed(0)
            self.ll = ll_train.LossNet()
            self.ll_opt = train.SGD(self.ll.parameters(), lr=1e-5, momentum=0.9, weight_decay=1e-4, net=self.ll)

    def step(self, ims, tgs):
        if self.name == "plain":
            losses = sum(self.model(ims, tgs).values())
            self.opt.zero_grad(); losses.backward(); self.opt.step()
            return
        features, d = self.model(ims, tgs)                  # the loop body of ll_train.train_one_epoch without its host read of the loss
        if self.retina:                                     # ll_train.py:98-119
            target = sum(torch.stack(v[1]) for v in d.values())
            task = sum(v[0] for v in d.values())
            features = {str(k): features[k] for k in range(4)}
        else:
            target = sum(d.values())
            task = sum(torch.mean(v) for v in d.values())
        if self.name == "detached":
            features = {k: v.detach() for k, v in features.items()}
        pred = self.ll(features)
        losses = task + ll_train.LossPredLoss(pred.view(pred.size(0)), target, margin=1.0)
        self.opt.zero_grad(); self.ll_opt.zero_grad(); losses.backward(); self.opt.step(); self.ll_opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4); ap.add_argument("--steps", type=int, default=10); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--out", default=None)
    ap.add_argument("--model", choices=("faster_rcnn", "retinanet"), default="faster_rcnn")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join("profiles", "ll_train_bench.json" if a.model == "faster_rcnn" else "ll_train_bench_retinanet.json")
    batches = batches_of(a.batch)
    modes = [Mode(n, a.batch, a.model) for n in ("plain", "detached", "live")]
    # Every trainer opens two streams of its own beside the main one.  With those, the second trainer built here measured ~4 ms per step
    # slower than the other two whatever its mode's work (consistent with a process's four hardware queues: its streams come to share a
    # queue with the main stream, and its backward loses its overlap) -- a cost of holding three trainers in one process, not of the mode.
    # The modes run one after the other, so all three use the first trainer's streams.
    for m in modes[1:]:
        m.net.side, m.net.aux = modes[0].net.side, modes[0].net.aux
    for m in modes:
        for i in range(a.warmup):
            m.step(*batches[i % 2])
    blocks = {m.name: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for i in range(a.steps):
                m.step(*batches[i % 2])
            e1.record(); torch.cuda.synchronize()
            blocks[m.name].append(e0.elapsed_time(e1) / a.steps)
    mean = {k: float(np.mean(v)) for k, v in blocks.items()}
    res = {"metric": "training step, ms per step (forward + backward + SGD), batch %d at 600/1000" % a.batch, "unit": "ms", "model": a.model,
           "steps_per_block": a.steps, "warmup_steps": a.warmup, "rounds": a.rounds, "timer": "HIP events between two synchronisations",
           "blocks_ms": {k: [round(x, 3) for x in v] for k, v in blocks.items()},
           "mean_ms": {k: round(v, 3) for k, v in mean.items()},
           "spread_ms": {k: round(float(np.max(v) - np.min(v)), 3) for k, v in blocks.items()},
           "detached_minus_plain_ms": round(mean["detached"] - mean["plain"], 3), "live_minus_detached_ms": round(mean["live"] - mean["detached"], 3),
           "per_round_detached_minus_plain_ms": [round(d - p, 3) for d, p in zip(blocks["detached"], blocks["plain"])],
           "per_round_live_minus_detached_ms": [round(l - d, 3) for l, d in zip(blocks["live"], blocks["detached"])],
           "padded_batch_hw": list(modes[0].net.last_padded_hw), "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
