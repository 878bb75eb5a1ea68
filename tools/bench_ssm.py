"""Throughput of the SSM sweep (cald_sweep_ssm) on one MI355X, beside the lt_c baseline sweep on the same HBM-resident pool: synthetic
VOC-shaped images, Faster R-CNN ResNet-50 at min_size 600 / max_size 1000, exact fp32.  The two sweeps run the same forward up to the box
predictor and differ in their tails (per-class NMS over all proposals against one class-batched NMS over the candidates above 0.05) and
in what comes back to the host (rows of C - 1 scores and labels against one float an image).

Each sweep is warmed up, then the two are alternated `--rounds` times in one process; a round is timed with HIP events on the launch
stream between two device synchronisations (the whole call, host work included).  The tail alone is timed through its hook
(cald_op_ssm_postprocess) on the predictor rows and proposals of real forwards, one view a call: that time INCLUDES the hook's
allocation and its copies to and from the host, so `tail_hook_ms_per_batch` (the per-view median times the batch size) is an upper bound
of what the tail's four launches cost inside a sweep, where the views of a batch share them.

    python tools/bench_ssm.py [--images 640] [--rounds 3] [--out profiles/ssm_sweep_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cald_amd import _ffi, baselines, detector, ssm, synth, train_ops
from cald_amd.pool import DevicePool
from bench_ll import csrc_sha1, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=640); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="images per forward, both sweeps")
    ap.add_argument("--tail-views", type=int, default=8, help="views whose tail is timed alone through the hook")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssm_sweep_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssm.py measures on an MI355X; there is no CPU path")
    model = ssm.fasterrcnn_resnet50_fpn_ssm(num_classes=21, min_size=600, max_size=1000).to("cuda:0")
    model.load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0))
    model.eval()
    pool = DevicePool.from_arrays(synth.make_pool(a.images, "voc", 0))
    images = [pool[i] for i in range(len(pool))]
    ptrs, Hs, Ws = baselines._arrays(images)
    L = _ffi.lib()

    def run_ssm(n=len(images)):
        return ssm.ssm_sweep_device_images(model, images[:n], batch_images=a.batch)

    def run_ltc(n=len(images)):
        out = np.zeros(n, np.float64)
        _ffi.check(L.cald_sweep_ltc(model.handle(), n, ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i), a.batch, _ffi.ptr(out, _ffi.c_d)))
        return out

    warm = min(len(images), 2 * a.batch)
    run_ssm(warm); run_ltc(warm)
    ssm_ms, ltc_ms, first = [], [], None
    for _ in range(a.rounds):
        s, t = timed(run_ssm); ssm_ms.append(t)
        assert first is None or all(x.tobytes() == y.tobytes() for x, y in zip(s, first)), "the SSM sweep is not reproducible"
        first = s
        _, t = timed(run_ltc); ltc_ms.append(t)
    al, counts = first[0], first[1]

    # the tail alone: the hook on the predictor rows and proposals of a real forward (all 1 000 rows: the synthetic weights fill the cap)
    nv = min(a.tail_views, len(images), a.batch)
    run_ssm(nv)
    ctx = detector.get_ctx(0)
    hook_ms, agree = [], True
    for v in range(nv):
        H, W = images[v].shape[:2]
        Hr, Wr, _, _ = train_ops.transform_size(H, W, 600, 1000)
        pred = model.debug_tensor("pred", v).reshape(1000, 105)
        props = model.debug_tensor("proposals", v).reshape(-1, 4)
        logits = np.ascontiguousarray(pred[:, :21]); deltas = np.ascontiguousarray(pred[:, 21:]); props = np.ascontiguousarray(props)
        boxes = np.empty((2000, 4), np.float32); scores = np.empty((2000, 20), np.float32); labels = np.empty((2000, 20), np.int8)
        alv, n = C.c_int(), C.c_int()
        best = None
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _ffi.check(L.cald_op_ssm_postprocess(ctx, 1000, 21, _ffi.ptr(logits), _ffi.ptr(deltas), _ffi.ptr(props), Hr, Wr, H, W, 0.05, 100,
                                                 C.byref(alv), C.byref(n), _ffi.ptr(boxes), _ffi.ptr(scores), _ffi.ptr(labels, _ffi.c_i8)))
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        agree = agree and n.value == counts[v] and alv.value == al[v]      # false if a view has fewer than 1 000 proposals: its last rows are stale
        hook_ms.append(best)

    n_img = len(images)
    ssm_ips = [n_img / (t / 1e3) for t in ssm_ms]; ltc_ips = [n_img / (t / 1e3) for t in ltc_ms]
    batch_ms = float(np.median(ssm_ms)) / (n_img / a.batch)
    tail_ms = float(np.median(hook_ms)) * a.batch
    res = {
        "metric": "SSM sweep throughput (Faster R-CNN forward + per-class NMS tail + rows to the host)", "unit": "images/s",
        "value": float(np.median(ssm_ips)), "ssm_images_per_s": ssm_ips, "lt_c_images_per_s": ltc_ips,
        "lt_c_median_images_per_s": float(np.median(ltc_ips)), "ssm_over_lt_c": float(np.median(ssm_ips) / np.median(ltc_ips)),
        "ssm_ms_per_batch": batch_ms, "lt_c_ms_per_batch": float(np.median(ltc_ms)) / (n_img / a.batch),
        "tail_hook_ms_per_view": hook_ms, "tail_hook_ms_per_batch": tail_ms, "tail_hook_share_of_batch_upper_bound": tail_ms / batch_ms,
        "tail_hook_rows_equal_the_sweeps": bool(agree),
        "images": n_img, "rounds": a.rounds, "batch_images": a.batch, "rows": int(counts.sum()), "al_images": int(al.sum()),
        "timing": "sweeps: HIP events on the launch stream between two device synchronisations, whole call, alternated; tail: wall clock of "
                  "the one-view hook (best of 5), allocation and host copies included -- an upper bound of the tail inside a sweep",
        "config": "Faster R-CNN ResNet-50 FPN, fp32, min_size 600 / max_size 1000, 21 classes, synthetic VOC-shaped pool resident in HBM",
        "device": torch.cuda.get_device_name(0), "csrc_sha1": csrc_sha1(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
