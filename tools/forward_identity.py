"""Launch-for-launch identity of two builds of the detector forward and of the sweeps on it (a host-side refactor of forward.hip, sweep.hip,
cutout_reuse.hip or lossnet.hip must not show here).

    python tools/forward_identity.py --root CHECKOUT --out A.json      # once per checkout (each with its own built library)
    python tools/forward_identity.py --compare A.json B.json --out profiles/NAME.json

For the checkout at --root (default: this one) every run below is made with cald_profile_enable on; the JSON holds, per run, the
`launch,desc,gflop` columns of cald_profile_dump (ms and tflops are timings and are left out) and a SHA-1 over the run's output bytes.  The
models are the small ones of the test fixtures (pseudo-trained ResNet-50, 300 / 500) on a fixed synth.make_pool.  The cut_out sweeps also hash
the counters of cald_profile_cutout / cald_profile_cutout_stages as they stand after the run.  --compare writes the first file's runs plus
the verdict; it exits 1 when the two differ.
"""
import argparse
import ctypes as C
import csv
import hashlib
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUGS = ["flip", "cut_out", "smaller_resize"]


def collect(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from cald_amd import _ffi, baselines, detector, ssm, synth, sweep, vaal
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

    def cut_counters():
        rows, dense, nb, nf = np.zeros(3), np.zeros(3), C.c_int64(), C.c_int64()
        _ffi.check(L.cald_profile_cutout(ctx, _ffi.ptr(rows, _ffi.c_d), _ffi.ptr(dense, _ffi.c_d), C.byref(nb), C.byref(nf)))
        st, kept = [np.zeros(6) for _ in range(4)], np.zeros(3, np.int64)
        _ffi.check(L.cald_profile_cutout_stages(ctx, *[_ffi.ptr(x, _ffi.c_d) for x in st], _ffi.ptr(kept, _ffi.c_i64)))
        return [rows, dense, np.array([nb.value, nf.value], np.int64)] + st + [kept]

    def swept_counted(m, reuse=None, cap=None):
        """the sweep under a cut_out reuse mode / a retention cap (None: the model's own), then the cut_out counters"""
        was_r, was_c = C.c_int(), C.c_int64()
        if reuse is not None:
            _ffi.check(L.cald_model_set_cutout_reuse(m.handle(), reuse, C.byref(was_r)))
        if cap is not None:
            _ffi.check(L.cald_model_set_cutout_retention_cap(m.handle(), cap, C.byref(was_c)))
        try:
            return swept(m) + cut_counters()
        finally:
            if reuse is not None:
                _ffi.check(L.cald_model_set_cutout_reuse(m.handle(), was_r.value, C.byref(was_r)))
            if cap is not None:
                _ffi.check(L.cald_model_set_cutout_retention_cap(m.handle(), was_c.value, C.byref(was_c)))

    def cutout_forward(m, prune):
        rects = np.array([[20, 30, 60, 70], [100, 10, 130, 50]], np.int32)
        out = m.debug_cutout_forward([(dev[1], False, rects[:1]), (dev[2], False, None), (dev[0], False, rects)], prune=prune)
        return [v.cpu().numpy() for d in out for _, v in sorted(d.items())] + [m.debug_tensor("C3", 0), m.debug_tensor("P2", 2)]

    def ssm_swept(m):
        return list(ssm.ssm_sweep_device_images(m, dev, batch_images=2))

    def retina_ssm_swept(m, pick=None):
        was = os.environ.pop("CALD_SSM_PICK", None)
        if pick:
            os.environ["CALD_SSM_PICK"] = pick
        try:
            random.seed(5)
            return ssm_swept(m)
        finally:
            os.environ.pop("CALD_SSM_PICK", None)
            if was is not None:
                os.environ["CALD_SSM_PICK"] = was

    loader = [((im,), (None,)) for im in dev]

    def ltc(m):
        return [np.array(baselines.lt_c_get_uncertainty(m, loader, batch_images=3))]

    def lsc(m):
        return [np.array(baselines.ls_c_get_uncertainty(m, loader, base_seed=3, batch_images=3))]

    def vaal_swept(_):
        sys.path.insert(0, os.path.join(root, "tests"))
        import _vaal_restatement as R
        g = np.load(os.path.join(root, "tests", "golden", "vaal.npz"))
        w = R.make_weights(int(g["seed"]))
        vm = vaal.VaalModel(w, w)
        try:
            imgs = [torch.from_numpy(np.ascontiguousarray(g["image%d" % i])).cuda() for i in range(int(g["n_images"]))]
            return [a for running in (False, True) for a in vaal.vaal_sweep_device_images(vm, None, imgs, batch_images=3, return_mu=True, bn_running=running)]
        finally:
            vm.close()

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
    run("frcnn_sweep", swept_counted, m)
    run("frcnn_sweep_reuse2", lambda mm: swept_counted(mm, reuse=2), m)
    run("frcnn_sweep_reuse0", lambda mm: swept_counted(mm, reuse=0), m)
    run("frcnn_sweep_stages_only", lambda mm: swept_counted(mm, cap=1), m)
    run("frcnn_cutout_forward", lambda mm: cutout_forward(mm, False), m)
    run("frcnn_cutout_forward_pruned", lambda mm: cutout_forward(mm, True), m)
    run("frcnn_sweep_audit", lambda mm: swept(mm, margins=True), m)
    run("frcnn_ll_sweep", ll, m)
    run("frcnn_ssm_sweep", ssm_swept, m)
    run("frcnn_ltc", ltc, m)
    run("frcnn_lsc", lsc, m)
    del m
    m = retina()
    run("retina_forward", forward, m)
    run("retina_sweep", swept, m)
    run("retina_ll_sweep", ll, m)
    run("retina_ssm_sweep", retina_ssm_swept, m)
    run("retina_ssm_sweep_python_pick", lambda mm: retina_ssm_swept(mm, "python"), m)
    run("retina_lsc", lsc, m)
    del m
    if os.path.exists(os.path.join(root, "tests", "golden", "vaal.npz")):
        run("vaal_sweep", vaal_swept, None)
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
