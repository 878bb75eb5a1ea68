"""Throughput of the RetinaNet SSM sweep (cald_sweep_ssm_retina) on one MI355X, beside the stock RetinaNet forward over the same
HBM-resident pool: synthetic VOC-shaped images, RetinaNet ResNet-50 at min_size 600 / max_size 1000, 21 classes, 50 detections a class,
exact fp32.  The two run the same network up to the heads and differ in their tails: the SSM tail lists every class's candidates in
anchor order, stops on the host for the per-class picks (retina_ssm.py:540-542) and runs NMS on at most 500 picks a class; the stock tail
sorts and suppresses all candidates of a class.  The synthetic weights score low, so the classification bias is raised by `--bias` (as in
tests/test_gpu_retina_ssm.py) until images have al = 0 and classes pass 500 candidates; the counts the run met are written beside the rates.

Three timings, all in one process:
  * the sweep with the C pick (cald_ssm_pick_mt19937), the sweep with the Python pick (random.shuffle in a ctypes callback) and the stock
    forward (forward_views, `--batch` images a call), warmed up and then alternated `--rounds` times; a round is timed with HIP events on
    the launch stream between two device synchronisations (the whole call, host work included);
  * the tail alone through its hook (cald_op_retina_ssm_postprocess) on the head tensors of real forwards, one view a call, wall clock,
    best of 5: that time INCLUDES the hook's allocation and its copies to and from the host, so it is an upper bound of the tail inside
    a sweep.

    python tools/bench_retina_ssm.py [--images 256] [--rounds 3] [--out profiles/retina_ssm_sweep_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cald_amd import _ffi, detector, ssm, synth, train_ops
from cald_amd.pool import DevicePool
from bench_ll import csrc_sha1, timed
from oracle import oracle as orc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="images per forward, sweep and stock forward alike")
    ap.add_argument("--bias", type=float, default=2.0, help="added to the classification head's bias")
    ap.add_argument("--tail-views", type=int, default=8, help="views whose tail is timed alone through the hook")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retina_ssm_sweep_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retina_ssm.py measures on an MI355X; there is no CPU path")
    sd = dict(synth.pseudo_trained_retinanet(21, 50, seed=0))
    sd["head.classification_head.cls_logits.bias"] = np.asarray(sd["head.classification_head.cls_logits.bias"], np.float32) + np.float32(a.bias)
    model = ssm.retinanet_resnet50_fpn_ssm(num_classes=21, min_size=600, max_size=1000).to("cuda:0")
    model.load_state_dict(sd)
    model.eval()
    pool = DevicePool.from_arrays(synth.make_pool(a.images, "voc", 0))
    images = [pool[i] for i in range(len(pool))]
    n_img = len(images)
    L = _ffi.lib()

    def run_ssm(mode, n=n_img):
        if mode == "python":
            os.environ["CALD_SSM_PICK"] = "python"
        else:
            os.environ.pop("CALD_SSM_PICK", None)
        random.seed(0)
        return ssm.ssm_sweep_device_images(model, images[:n], batch_images=a.batch)

    def run_stock(n=n_img):
        rows = 0
        for i0 in range(0, n, a.batch):
            rows += sum(len(r["scores"]) for r in model.forward_views([(im, False, None) for im in images[i0:min(n, i0 + a.batch)]]))
        return rows

    assert ssm._c_pick_checked(), "cald_ssm_pick_mt19937 failed its self-check"
    warm = min(n_img, 2 * a.batch)
    run_ssm("c", warm); run_ssm("python", warm); run_stock(warm)
    c_ms, py_ms, stock_ms, first, stock_rows = [], [], [], None, 0
    for _ in range(a.rounds):
        s, t = timed(lambda: run_ssm("c")); c_ms.append(t)
        assert first is None or all(x.tobytes() == y.tobytes() for x, y in zip(s, first)), "the SSM sweep is not reproducible"
        first = s
        p, t = timed(lambda: run_ssm("python")); py_ms.append(t)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(p, first)), "the Python pick and the C pick disagree"
        stock_rows, t = timed(run_stock); stock_ms.append(t)
    os.environ.pop("CALD_SSM_PICK", None)
    al, counts = first[0], first[1]

    # candidates per image: one more (untimed) sweep whose callback writes the counts down and hands on to the C pick
    state = np.array(random.Random(0).getstate()[1], np.uint32)
    cand = {}

    @_ffi.PICK_FN
    def counting(user, image, K, cn, picks, n_picks):
        cand[image] = [cn[k] for k in range(K)]
        return L.cald_ssm_pick_mt19937(state.ctypes.data, image, K, cn, picks, n_picks)
    from cald_amd.baselines import _arrays
    ptrs, Hs, Ws = _arrays(images)
    cap = n_img * 21 * 50
    o_al = np.zeros(n_img, np.int32); o_cnt = np.zeros(n_img, np.int32); o_b = np.empty((cap, 4), np.float32); o_s = np.empty(cap, np.float32)
    o_l = np.empty((cap, 20), np.int8); need = C.c_int64(0)
    _ffi.check(L.cald_sweep_ssm_retina(model.handle(), n_img, ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i), a.batch, C.cast(counting, C.c_void_p), None,
                                       cap, _ffi.ptr(o_al, _ffi.c_i), _ffi.ptr(o_cnt, _ffi.c_i), _ffi.ptr(o_b), _ffi.ptr(o_s), _ffi.ptr(o_l, _ffi.c_i8), C.byref(need)))
    per_image = np.array([sum(v) for v in cand.values()], np.int64) if cand else np.zeros(1, np.int64)
    per_class = np.array([max(v) for v in cand.values()], np.int64) if cand else np.zeros(1, np.int64)

    # the tail alone: the hook on the head tensors of a real forward
    nv = min(a.tail_views, n_img, a.batch)
    run_ssm("c", nv)
    ctx = detector.get_ctx(0)
    base = np.ascontiguousarray(np.stack([orc.base_anchors(list(s), [0.5, 1.0, 2.0]) for s in orc.retina_anchor_sizes()]), np.float32)
    hook_ms, hook_cands = [], []
    pick_c = C.cast(L.cald_ssm_pick_mt19937, C.c_void_p)
    for v in range(nv):
        H, W = images[v].shape[:2]
        Hr, Wr, Hp, Wp = train_ops.transform_size(H, W, 600, 1000)
        cls = [np.ascontiguousarray(model.debug_tensor("cls%d" % l, v)) for l in range(5)]; reg = [np.ascontiguousarray(model.debug_tensor("reg%d" % l, v)) for l in range(5)]
        hw = np.array([x for c in cls for x in c.shape[:2]], np.int32)
        cp = (_ffi.c_f * 5)(*[_ffi.ptr(c) for c in cls]); rp = (_ffi.c_f * 5)(*[_ffi.ptr(r) for r in reg])
        boxes = np.empty((21 * 50, 4), np.float32); scores = np.empty(21 * 50, np.float32); labels = np.empty((21 * 50, 20), np.int8)
        cn = np.zeros(21, np.int32); alv, n = C.c_int(), C.c_int()
        best = None
        for _ in range(5):
            st = np.array(random.Random(v).getstate()[1], np.uint32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _ffi.check(L.cald_op_retina_ssm_postprocess(ctx, cp, rp, _ffi.ptr(hw, _ffi.c_i), 9, 21, _ffi.ptr(base), Hp, Wp, Hr, Wr, H, W, 0.05, 0.5, 50, pick_c,
                                                        C.c_void_p(st.ctypes.data), C.byref(alv), C.byref(n), _ffi.ptr(cn, _ffi.c_i), _ffi.ptr(boxes),
                                                        _ffi.ptr(scores), _ffi.ptr(labels, _ffi.c_i8)))
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        hook_ms.append(best); hook_cands.append(int(cn.sum()))

    ips = lambda ms: [n_img / (t / 1e3) for t in ms]
    c_ips, py_ips, stock_ips = ips(c_ms), ips(py_ms), ips(stock_ms)
    res = {
        "metric": "RetinaNet SSM sweep throughput (forward + candidate lists + host picks + per-class NMS + rows to the host)", "unit": "images/s",
        "value": float(np.median(c_ips)), "ssm_c_pick_images_per_s": c_ips, "ssm_python_pick_images_per_s": py_ips, "stock_forward_images_per_s": stock_ips,
        "stock_forward_median_images_per_s": float(np.median(stock_ips)), "ssm_over_stock_forward": float(np.median(c_ips) / np.median(stock_ips)),
        "python_pick_over_c_pick_time": float(np.median(py_ms) / np.median(c_ms)),
        "ssm_ms_per_image_c_pick": float(np.median(c_ms)) / n_img, "ssm_ms_per_image_python_pick": float(np.median(py_ms)) / n_img,
        "stock_forward_ms_per_image": float(np.median(stock_ms)) / n_img,
        "tail_hook_ms_per_view": hook_ms, "tail_hook_candidates_per_view": hook_cands,
        "candidates_per_image": {"images_with_al_0": int(len(cand)), "min": int(per_image.min()), "median": float(np.median(per_image)), "max": int(per_image.max()),
                                 "largest_class_median": float(np.median(per_class)), "largest_class_max": int(per_class.max())},
        "images": n_img, "rounds": a.rounds, "batch_images": a.batch, "rows": int(counts.sum()), "stock_rows": int(stock_rows), "al_images": int(al.sum()),
        "cls_bias_added": a.bias,
        "timing": "sweeps and stock forward: HIP events on the launch stream between two device synchronisations, whole call, alternated; tail: wall "
                  "clock of the one-view hook (best of 5), allocation and host copies included -- an upper bound of the tail inside a sweep",
        "config": "RetinaNet ResNet-50 FPN, fp32, min_size 600 / max_size 1000, 21 classes, 50 detections a class, synthetic VOC-shaped pool resident in HBM",
        "device": torch.cuda.get_device_name(0), "csrc_sha1": csrc_sha1(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
