"""Per-tensor gradient error of one HIP training step against the float64 torch-CPU autograd oracle (debug aid).

    python tools/train_grad_check.py [out.json] [--model frcnn|retinanet] [--forward-precision fp32|f16x3] [--backward-precision fp32|f16x3]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cald_amd import synth, train
from oracle import torch_train as tt


def check(model="frcnn", forward_precision="fp32", backward_precision="fp32", verbose=False):
    """One step at min_size 160 / max_size 256 on two images; the reference gets the HIP run's proposals, sampler draws and ReLU decisions.
    backward_precision "f16x3": the checked step is the one after the calibration step (whose data gradients are the exact ones)."""
    from tests.test_gpu_train import _train_case
    kw = {} if forward_precision == "fp32" else {"forward_precision": forward_precision}
    if backward_precision != "fp32":
        kw["backward_precision"] = backward_precision
    if model == "retinanet":
        _, images, targets = _train_case(torch, seed=6)
        sd = synth.pseudo_trained_retinanet(21, 50, seed=2)
        net = train.RetinaNetTrainer(sd, 21, min_size=160, max_size=256, **kw)
    else:
        sd, images, targets = _train_case(torch)
        net = train.FasterRCNNTrainer(sd, 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(7), **kw)
    if backward_precision == "f16x3":
        net.forward(images, targets); net.backward()
    losses = net.forward(images, targets)
    grads = {k: v.clone() for k, v in net.backward().items()}
    if model == "retinanet":
        ref = tt.TorchTrainRetinaNet(sd, 21, min_size=160, max_size=256)
        ref.masks = net.relu_decisions()
        want, rec = ref.losses(images, targets)
    else:
        props = [p.cpu() for p in net.last["proposals"]]
        ref = tt.TorchTrainFRCNN(sd, 21, min_size=160, max_size=256)
        ref.masks = net.relu_decisions()
        want, rec = ref.losses(images, targets, props, None, cfg=dict(box_batch=64), samples=net.last["samples"])
    sum(want.values()).backward()
    tr = ref.trainable()
    rows = {}
    for k in net.names:
        w = tr[k].grad; g = grads[k].double().cpu(); d = (g - w).abs()
        rows[k] = {"max_abs_ref": float(w.abs().max()), "max_err_over_max_ref": float(d.max() / w.abs().max())}
        if verbose:
            print("%-55s max|ref| %.3e  err/max %.3e  rms err/rms ref %.3e" % (k, float(w.abs().max()), float(d.max() / w.abs().max()), float(d.pow(2).mean().sqrt() / w.pow(2).mean().sqrt())))
    return {"what": "one %s R50-FPN training step (2 images, min_size 160 / max_size 256%s), forward_precision %s, backward_precision %s: HIP vs the float64 "
                    "torch-CPU autograd restatement (oracle/torch_train.py) given the HIP run's %sReLU decisions"
                    % ("RetinaNet" if model == "retinanet" else "Faster R-CNN", "" if model == "retinanet" else ", 64 RoIs / image", forward_precision, backward_precision,
                       "" if model == "retinanet" else "proposals, sampler draws and "),
            "losses_hip": {k: float(v) for k, v in losses.items()}, "losses_ref": {k: float(v) for k, v in want.items()},
            "tensors": len(rows), "worst_tensor_error": max(r["max_err_over_max_ref"] for r in rows.values()),
            "tolerance_in_tests": 1e-4, "per_tensor": rows}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None, help="artifact: losses and the per-tensor errors as JSON")
    ap.add_argument("--model", default="frcnn", choices=["frcnn", "retinanet"])
    ap.add_argument("--forward-precision", default="fp32", choices=["fp32", "f16x3"])
    ap.add_argument("--backward-precision", default="fp32", choices=["fp32", "f16x3"])
    a = ap.parse_args()
    out = check(a.model, a.forward_precision, a.backward_precision, verbose=True)
    if a.out:
        import json
        json.dump(out, open(a.out, "w"), indent=1)
    print("worst", out["worst_tensor_error"])
