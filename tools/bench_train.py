"""Throughput of the training step on one MI355X: images / s of forward + backward + SGD at the reference's
training configuration (cald_train.py: batch size 4 per GPU, VOC images at min_size 600 / max_size 1000, 2 000 proposals,
512 sampled RoIs per image).  Synthetic VOC-sized images and boxes, pseudo-trained weights.

    python tools/bench_train.py [--batch 4] [--steps 10] [--warmup 3] [--forward-precision fp32|f16x3] [--backward-precision fp32|f16x3]
    python tools/bench_train.py --alternate 3 [--out profiles/train_f16x3_backward.json]

--alternate N: the four forward x backward precision combinations in ONE process: per detector one trainer of each combination on the same
weights and batches, N rounds of one block per combination; per combination the rounds' ms_per_step and forward_ms and their medians and
spreads, the forward layers and the data-gradient launches with the kernel each landed on, and the per-tensor gradient error of
tools/train_grad_check.py.  (The first backward of a backward_precision="f16x3" trainer is its calibration step: it falls into the warm-up.)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cald_amd import synth, train


def _trainer(arch, depth, forward_precision="fp32", backward_precision="fp32"):
    """(trainer, TrainableDetector, SGD) at the reference's training configuration; a keyword is passed only when it is not the default."""
    kw = {} if forward_precision == "fp32" else {"forward_precision": forward_precision}
    if backward_precision != "fp32":
        kw["backward_precision"] = backward_precision
    if arch == "retinanet":
        sd = synth.pseudo_trained_retinanet(21, depth, seed=0)
        net = train.RetinaNetTrainer(sd, 21, depth=depth, min_size=600, max_size=1000, **kw)
    else:
        sd = synth.pseudo_trained_frcnn(21, depth, seed=0)
        net = train.FasterRCNNTrainer(sd, 21, depth=depth, min_size=600, max_size=1000, generator=torch.Generator().manual_seed(0), **kw)
    model = train.TrainableDetector(net)
    opt = train.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-5, momentum=0.9, weight_decay=1e-4, net=net)
    return net, model, opt


def _batches(batch, mixed=False):
    """Two batches of synthetic VOC-sized images with three boxes each."""
    from types import SimpleNamespace
    a = SimpleNamespace(batch=batch)
    if mixed:                       # whatever order the pool comes in: landscape and portrait images share batches (pads to 800 x 800)
        imgs = synth.make_pool(a.batch * 2, "voc", 0)
    else:                           # cald_train.py's default sampler (:326-330, --aspect-ratio-group-factor 3): one aspect-ratio group per batch
        from torch.utils.data.sampler import SequentialSampler
        from cald_amd.group_by_aspect_ratio import GroupedBatchSampler, _quantize
        sizes = synth.pool_sizes(16 * a.batch, "voc", 0)
        groups = _quantize([float(w) / float(h) for h, w in sizes], (2 ** np.linspace(-1, 1, 7)).tolist())
        picked = [b for _, b in zip(range(2), GroupedBatchSampler(SequentialSampler(sizes), groups, a.batch))]
        imgs = [synth.synth_image(i, sizes[i][0], sizes[i][1]) for b in picked for i in b]
    rs = np.random.RandomState(0)
    batches = []
    for b in range(2):
        ims, tgs = [], []
        for im in imgs[b * a.batch:(b + 1) * a.batch]:
            H, W = im.shape[:2]
            k = 3
            x0 = rs.rand(k) * W * 0.6; y0 = rs.rand(k) * H * 0.6
            boxes = np.stack([x0, y0, x0 + W * 0.3, y0 + H * 0.3], axis=1).astype(np.float32)
            ims.append(torch.from_numpy(im).cuda()); tgs.append({"boxes": torch.from_numpy(boxes), "labels": torch.from_numpy(rs.randint(1, 21, k).astype(np.int64))})
        batches.append((ims, tgs))
    return batches


def measure(batch=4, steps=10, warmup=3, depth=50, verbose=False, model="frcnn", mixed=False, forward_precision="fp32", backward_precision="fp32"):
    from types import SimpleNamespace
    a = SimpleNamespace(batch=batch, steps=steps, warmup=warmup, depth=depth)
    arch = model
    net, model, opt = _trainer(arch, a.depth, forward_precision, backward_precision)
    batches = _batches(a.batch, mixed)

    def step(i, parts=None):
        ims, tgs = batches[i % 2]
        t0 = time.time()
        loss_dict = model(ims, tgs); losses = sum(loss_dict.values())
        if parts is not None:
            torch.cuda.synchronize(); t1 = time.time()
        opt.zero_grad(); losses.backward()
        if parts is not None:
            torch.cuda.synchronize(); t2 = time.time()
        opt.step()
        if parts is not None:
            torch.cuda.synchronize(); parts.append((t1 - t0, t2 - t1, time.time() - t2))
        return losses
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize(); t = time.time()
    per = []
    for i in range(a.steps):
        ts = time.time()
        last = step(i)
        per.append(round((time.time() - ts) * 1e3, 1))
    torch.cuda.synchronize(); dt = (time.time() - t) / a.steps
    if verbose:
        print("host time per step (ms, not synchronized):", per, file=sys.stderr)
    parts = []
    for i in range(4):
        step(i, parts)
    p = np.mean(parts, axis=0)
    ims, tgs = batches[0]
    net.forward(ims, tgs); torch.cuda.synchronize()
    t0 = time.time(); net.backward(); t_enq = time.time() - t0; torch.cuda.synchronize(); t_all = time.time() - t0
    if verbose:
        print("backward: host enqueue %.1f ms, until the GPU is done %.1f ms" % (t_enq * 1e3, t_all * 1e3), file=sys.stderr)
    net.flops = 0.0
    step(0)
    flops, net.flops = net.flops, None
    net.timing = []
    step(0)
    sections = {b[0]: round((b[1] - a_[1]) * 1e3, 2) for a_, b in zip(net.timing[:-1], net.timing[1:])}
    net.timing = None
    if verbose:
        print("forward sections (ms, synchronized):", sections, file=sys.stderr)
    return {"metric": "training step throughput (forward + backward + SGD)", "value": a.batch / dt, "unit": "images/s", "ms_per_step": dt * 1e3,
            "batch": a.batch, "model": arch, "depth": a.depth, "forward_ms": p[0] * 1e3, "backward_ms": p[1] * 1e3, "sgd_ms": p[2] * 1e3,
            "backward_gpu_ms": t_all * 1e3,
            "gemm": {"algorithmic_gflop_per_step": flops / 1e9, "achieved_tflops_over_whole_step": flops / dt / 1e12, "peak_tflops": 157.3,
                     "frac_of_fp32_mfma_peak": flops / dt / 1e12 / 157.3, "note": "forward + data-gradient + weight-gradient GEMM FLOPs (true channels, no padding, strided data gradients at their algorithmic cost) / wall-clock of the whole step incl. host work"}, "loss": float(last.detach()), "dtype": "f32", "forward_precision": forward_precision, "backward_precision": backward_precision,
            "batch_composition": "mixed orientations" if mixed else "one aspect-ratio group per batch (GroupedBatchSampler, k = 3)",
            "padded_batch_hw": [list(net.last_padded_hw)] if getattr(net, "last_padded_hw", None) else None,
            "config": "cald_train.py defaults: batch 4, VOC-sized synthetic images, min_size 600 / max_size 1000, SGD momentum 0.9"
                      + (", 2000 proposals, 512 RoIs / image" if arch == "frcnn" else ", 9 anchors / location on P3-P7")}


MODES = (("fp32", "fp32"), ("f16x3", "fp32"), ("fp32", "f16x3"), ("f16x3", "f16x3"))      # (forward_precision, backward_precision)


def alternate(rounds=3, steps=10, warmup=3, batch=4, depth=50, grad_check=True):
    """The four precision combinations alternated in one process on one trainer each per detector.  Keys: "<forward>/<backward>"."""
    from cald_amd import train_ops as ops
    out = {"what": "training step in the four combinations of forward_precision x backward_precision ('f16x3': forward convs / linears on "
                   "conv_h3 / conv_h4; data gradients on conv_h3 with per-tensor gradient exponents; weight gradients and SGD always exact "
                   "fp32): %d rounds of one block of %d steps per combination in one process, one trainer of each combination per detector on "
                   "the same weights and batches; batch %d, min_size 600 / max_size 1000, R%d" % (rounds, steps, batch, depth),
           "rounds": rounds, "steps_per_block": steps, "batch": batch, "detectors": {}}
    batches = _batches(batch)
    name = lambda m: "%s/%s" % m
    for arch in ("frcnn", "retinanet"):
        pair = {name(m): _trainer(arch, depth, *m) for m in MODES}

        def step(fp, i, parts=None):
            net, model, opt = pair[fp]
            ims, tgs = batches[i % 2]
            t0 = time.time()
            losses = sum(model(ims, tgs).values())
            if parts is not None:
                torch.cuda.synchronize(); parts.append(time.time() - t0)
            opt.zero_grad(); losses.backward(); opt.step()
            return losses
        res = {fp: {"ms_per_step_rounds": [], "forward_ms_rounds": []} for fp in pair}
        for r in range(rounds):
            for fp in pair:
                for i in range(warmup):
                    step(fp, i)
                torch.cuda.synchronize(); t = time.time()
                for i in range(steps):
                    last = step(fp, i)
                torch.cuda.synchronize()
                res[fp]["ms_per_step_rounds"].append(round((time.time() - t) / steps * 1e3, 3))
                parts = []
                for i in range(4):
                    step(fp, i, parts)
                torch.cuda.synchronize()
                res[fp]["forward_ms_rounds"].append(round(float(np.mean(parts)) * 1e3, 3))
                res[fp]["last_loss"] = float(last.detach())
        for fp in pair:
            for k in ("ms_per_step", "forward_ms"):
                v = res[fp][k + "_rounds"]
                res[fp][k] = float(np.median(v)); res[fp][k + "_spread"] = round(max(v) - min(v), 3)
            with ops.record_kernels() as log:
                pair[fp][0].forward(*batches[0])
            with ops.record_dgrad_kernels() as dlog:
                pair[fp][0].backward()
            torch.cuda.synchronize()
            res[fp]["forward_layers"] = [{"layer": l, "kernel": k} for l, k in log]
            res[fp]["dgrad_launches"] = [{"layer": l, "kernel": k} for l, k in dlog]
            for key, lg in (("launches_by_kernel_family", log), ("dgrad_launches_by_kernel_family", dlog)):
                fam = {}
                for _, k in lg:
                    fam[k.split("<")[0]] = fam.get(k.split("<")[0], 0) + 1
                res[fp][key] = fam
            if pair[fp][0].backward_precision == "f16x3":
                res[fp]["gradient_exponents_G"] = sorted(set(pair[fp][0]._grad_G.values()))
        base = res["fp32/fp32"]["ms_per_step"]
        spread = max(res[fp]["ms_per_step_spread"] for fp in pair)
        res["round_to_round_spread_ms"] = spread
        res["gain_ms_per_step_over_fp32/fp32"] = {fp: round(base - res[fp]["ms_per_step"], 3) for fp in pair if fp != "fp32/fp32"}
        res["backward_gain_ms_per_step"] = {"forward fp32": round(base - res["fp32/f16x3"]["ms_per_step"], 3),
                                            "forward f16x3": round(res["f16x3/fp32"]["ms_per_step"] - res["f16x3/f16x3"]["ms_per_step"], 3)}
        res["backward_f16x3_is_faster_by_more_than_the_spread"] = {k: bool(v > spread) for k, v in res["backward_gain_ms_per_step"].items()}
        out["detectors"][arch] = res
        del pair
        torch.cuda.empty_cache()
    if grad_check:
        import train_grad_check
        out["gradient_error_vs_float64_autograd"] = {
            "what": "tools/train_grad_check.py: the step after the calibration step at min_size 160 / max_size 256, worst per-tensor max |grad - ref| / max |ref|; the tests' bound is 1e-4",
            **{arch: {name(m): train_grad_check.check(arch, *m)["worst_tensor_error"] for m in MODES} for arch in ("frcnn", "retinanet")}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4); ap.add_argument("--steps", type=int, default=10); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=50); ap.add_argument("--model", default="frcnn", choices=["frcnn", "retinanet"])
    ap.add_argument("--mixed", action="store_true", help="landscape and portrait images in one batch instead of the reference's aspect-ratio-grouped batches")
    ap.add_argument("--forward-precision", default="fp32", choices=["fp32", "f16x3"], help="the trainers' forward_precision")
    ap.add_argument("--backward-precision", default="fp32", choices=["fp32", "f16x3"], help="the trainers' backward_precision")
    ap.add_argument("--alternate", type=int, default=0, metavar="ROUNDS", help="the four forward x backward precision combinations alternated in one process, both detectors")
    ap.add_argument("--out", default=None, help="with --alternate: write the result here as JSON")
    ap.add_argument("--no-grad-check", action="store_true", help="with --alternate: leave out the float64 gradient check")
    a = ap.parse_args()
    if a.alternate:
        res = alternate(a.alternate, a.steps, a.warmup, a.batch, a.depth, grad_check=not a.no_grad_check)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        slim = {k: ({d: {fp: {q: w for q, w in r.items() if q not in ("forward_layers", "dgrad_launches")} if isinstance(r, dict) else r for fp, r in dv.items()}
                     for d, dv in v.items()} if k == "detectors" else v) for k, v in res.items()}
        print(json.dumps(slim))
        return
    print(json.dumps(measure(a.batch, a.steps, a.warmup, a.depth, verbose=True, model=a.model, mixed=a.mixed, forward_precision=a.forward_precision,
                             backward_precision=a.backward_precision)))


if __name__ == "__main__":
    main()
