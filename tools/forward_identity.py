"""Launch-for-launch identity of two builds of the detector forward (a host-side refactor of forward.hip must not show here).

    python tools/forward_identity.py --root CHECKOUT --out A.json      # once per checkout (each with its own built library)
    python tools/forward_identity.py --compare A.json B.json --out profiles/NAME.json

For the checkout at --root (default: this one) every run below is made with cald_profile_enable on; the JSON holds, per run, the
`launch,desc,gflop` columns of cald_profile_dump (ms and tflops are timings and are left out) and a SHA-1 over the run's output bytes.  The
models are the small ones of the test fixtures (pseudo-trained ResNet-50, 300 / 500) on a fixed synth.make_pool.  --compare writes the first
file's runs plus the verdict; it exits 1 when the two differ.
"""
import argparse
import csv
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUGS = ["flip", "cut_out", "smaller_resize"]


def collect(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from cald_amd import _ffi, baselines, detector, synth, sweep
    assert os.path.abspath(os.path.dirname(os.path.dirname(_ffi.__file__))) == os.path.abspath(root), "cald_amd was not imported from --root"
    L, ctx = _ffi.lib(), detector.get_ctx(0)
    pool = synth.make_pool(4, "voc", 0, scale=0.5)
    dev = [torch.from_numpy(im).cuda() for im in pool]
    g = np.load(os.path.join(root, "tests", "golden", "lossnet.npz"))
    ll_sd = {k[3:]: g[k] for k in g.files if k.startswith("sd_")}

    def frcnn(**kw):
        m = detector.fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=300, max_size=500, **kw)
        m.to("cuda").load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0))
        return m.eval()

    def retina(**kw):
        m = detector.retinanet_resnet50_fpn_cal(num_classes=21, min_size=300, max_size=500, **kw)
        m.to("cuda").load_state_dict(synth.pseudo_trained_retinanet(21, 50, seed=0))
        return m.eval()

    def forward(m):
        rects = np.array([[20, 30, 60, 70], [100, 10, 130, 50]], np.int32)
        out = m.forward_views([(dev[1], False, None), (dev[2], True, None), (dev[0], False, rects)])
        return [v.cpu().numpy() for d in out for _, v in sorted(d.items())]

    def captured(m):
        m.set_rpn_prune_capture(True)
        try:
            return forward(m) + [m.debug_tensor("rpn_look0", 0), m.debug_tensor("rpn_pnorm1", 1)]
        finally:
            m.set_rpn_prune_capture(False)

    def swept(m, **kw):
        return list(sweep.sweep_device_images(m, dev, list(range(len(dev))), AUGS, bp=1.3, base_seed=3, batch_images=2, **kw))

    def ll(m):
        return list(baselines.ll_sweep_device_images(m, ll_sd, dev, [0, 0, 1, 1], return_pooled=True))

    runs = {}

    def run(name, fn, m):
        _ffi.check(L.cald_profile_enable(ctx, 1))
        arrays = fn(m)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "profile.csv")
            _ffi.check(L.cald_profile_dump(ctx, path.encode()))
            rows = ["%s,%s,%s" % (r["launch"], r["desc"], r["gflop"]) for r in csv.DictReader(open(path))]
        _ffi.check(L.cald_profile_enable(ctx, 0))
        h = hashlib.sha1()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        runs[name] = dict(sha1=h.hexdigest(), launches=rows)
        print("%-28s %4d launches  %s" % (name, len(rows), h.hexdigest()), flush=True)

    m = frcnn()
    m.set_rpn_prune(True)
    run("frcnn_forward", forward, m)
    run("frcnn_forward_capture", captured, m)
    run("frcnn_sweep", swept, m)
    run("frcnn_sweep_audit", lambda mm: swept(mm, margins=True), m)
    run("frcnn_ll_sweep", ll, m)
    del m
    m = retina()
    run("retina_forward", forward, m)
    run("retina_sweep", swept, m)
    run("retina_ll_sweep", ll, m)
    del m
    run("frcnn_forward_f16x3", forward, frcnn(precision="f16x3"))
    run("retina_forward_f16x3", forward, retina(precision="f16x3"))
    return runs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.compare:
        A, B = [json.load(open(p))["runs"] for p in a.compare]
        diff = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
        res = dict(compared=[os.path.basename(p) for p in a.compare], identical=not diff, differing_runs=diff,
                   launches={k: len(v["launches"]) for k, v in A.items()}, runs=A)
    else:
        res = dict(runs=collect(os.path.abspath(a.root)))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    if a.compare:
        print("identical" if res["identical"] else "DIFFERENT: %s" % ", ".join(res["differing_runs"]))
        sys.exit(0 if res["identical"] else 1)


if __name__ == "__main__":
    main()
