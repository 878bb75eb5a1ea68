"""Throughput of the learning-loss sweep (cald_sweep_ll) on one MI355X, beside the lt_c baseline sweep (the full one-view forward) on the
same HBM-resident pool: synthetic VOC-shaped images, loader batches of 4, Faster R-CNN ResNet-50 at min_size 600 / max_size 1000, exact fp32.

Each sweep is warmed up, then the two are alternated `--rounds` times; a round is timed with HIP events on the launch stream between two
device synchronisations.  A last, separate ll pass runs under the library's event profile and gives the per-kernel times: the pooling
kernels' bytes / time stands next to the 6.29 TB/s float4-copy rate of the chip (8.0 TB/s HBM3E peak).

    python tools/bench_ll.py [--images 1280] [--rounds 3] [--out profiles/ll_sweep_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cald_amd import _ffi, baselines, detector, synth
from cald_amd.pool import DevicePool

COPY_RATE_TBPS = 6.29      # measured float4 copy rate of an MI355X


def csrc_sha1():
    import hashlib
    h = hashlib.sha1()
    d = os.path.join(ROOT, "cald_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")) or f == "Makefile":
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def lossnet_weights(seed=0, D=128):
    rs = np.random.RandomState(seed)
    sd = {}
    for j in range(1, 5):
        sd["FC%d.weight" % j] = (rs.randn(D, 256) / 16).astype(np.float32)
        sd["FC%d.bias" % j] = (rs.randn(D) * 0.1).astype(np.float32)
    sd["linear.weight"] = (rs.randn(1, 4 * D) / np.sqrt(4 * D)).astype(np.float32)
    sd["linear.bias"] = np.array([0.1], np.float32)
    return sd


def timed(fn):
    """(result, milliseconds between two events on the current stream), synchronised on both sides"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1280); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--group", type=int, default=4, help="loader batch size (ll_train.py --batch_size)")
    ap.add_argument("--batch-views", type=int, default=32); ap.add_argument("--ltc-batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ll_sweep_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ll.py measures on an MI355X; there is no CPU path")
    model = detector.fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=600, max_size=1000).to("cuda:0")
    model.load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0))
    model.eval()
    ll_sd = lossnet_weights()
    pool = DevicePool.from_arrays(synth.make_pool(a.images, "voc", 0))
    images = [pool[i] for i in range(len(pool))]
    groups = [i // a.group for i in range(len(images))]
    ptrs, Hs, Ws = baselines._arrays(images)
    L = _ffi.lib()

    def run_ll(n=len(images)):
        return baselines.ll_sweep_device_images(model, ll_sd, images[:n], groups[:n], batch_views=a.batch_views)

    def run_ltc(n=len(images)):
        out = np.zeros(n, np.float64)
        _ffi.check(L.cald_sweep_ltc(model.handle(), n, ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i), a.ltc_batch, _ffi.ptr(out, _ffi.c_d)))
        return out

    warm = min(len(images), 2 * max(a.batch_views, a.ltc_batch))
    run_ll(warm); run_ltc(warm)
    ll_ms, ltc_ms, ll_first = [], [], None
    for _ in range(a.rounds):
        s, t = timed(run_ll); ll_ms.append(t)
        assert ll_first is None or np.array_equal(s, ll_first), "the ll sweep is not reproducible"
        ll_first = s
        _, t = timed(run_ltc); ltc_ms.append(t)
    # the same images as loader batches of one: no image is padded beyond its own size (what the group padding costs)
    solo = list(range(len(images)))
    baselines.ll_sweep_device_images(model, ll_sd, images[:warm], solo[:warm], batch_views=a.batch_views)
    _, solo_ms = timed(lambda: baselines.ll_sweep_device_images(model, ll_sd, images, solo, batch_views=a.batch_views))
    sizes = [tuple(im.shape[:2]) for im in images]
    area = lambda pads: float(sum(h * w for h, w in pads))
    pad_ratio = area(baselines.ll_group_padding(sizes, groups, 600, 1000)) / area(baselines.ll_group_padding(sizes, solo, 600, 1000))
    # ---- per-kernel times of one ll pass, in a run of its own (the profile's events serialise nothing but are not free) ----
    ctx = detector.get_ctx(0)
    _ffi.check(L.cald_profile_enable(ctx, 1))
    run_ll()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ll.csv")
        _ffi.check(L.cald_profile_dump(ctx, path.encode()))
        import csv
        rows = list(csv.reader(open(path)))[1:]          # launch, "desc", gflop, ms, tflops
    _ffi.check(L.cald_profile_enable(ctx, 0))
    gap_ms = gap_bytes = finish_ms = conv_ms = 0.0
    for r in rows:
        ms = float(r[3])
        if r[1].startswith("gap_partial"):
            gap_ms += ms; gap_bytes += float(r[1].split("bytes=")[1])
        elif r[1].startswith("gap_finish"):
            finish_ms += ms
        else:
            conv_ms += ms
    n = len(images)
    ll_ips = [n / (t / 1e3) for t in ll_ms]; ltc_ips = [n / (t / 1e3) for t in ltc_ms]
    res = {
        "metric": "learning-loss sweep throughput (features-only forward + pooling + LossNet)", "unit": "images/s",
        "value": float(np.median(ll_ips)), "ll_images_per_s": ll_ips, "lt_c_images_per_s": ltc_ips,
        "lt_c_median_images_per_s": float(np.median(ltc_ips)), "ll_over_lt_c": float(np.median(ll_ips) / np.median(ltc_ips)),
        "ll_loader_batch_1_images_per_s": n / (solo_ms / 1e3), "padded_pixels_over_own_pixels": pad_ratio,
        "images": n, "rounds": a.rounds, "loader_batch": a.group, "batch_views": a.batch_views, "lt_c_batch_images": a.ltc_batch,
        "timing": "HIP events on the launch stream between two device synchronisations, whole call (host work included); ll and lt_c alternated",
        "profiled_ll_pass": {
            "conv_ms": conv_ms, "gap_partial_ms": gap_ms, "gap_finish_ms": finish_ms, "gap_partial_bytes": gap_bytes,
            "gap_partial_tbps": (gap_bytes / (gap_ms / 1e3) / 1e12) if gap_ms > 0 else None, "float4_copy_tbps": COPY_RATE_TBPS,
            "gap_partial_share_of_copy_rate": (gap_bytes / (gap_ms / 1e3) / 1e12 / COPY_RATE_TBPS) if gap_ms > 0 else None,
            "note": "event times of the launches of one ll pass (profile on, a run of its own); bytes = the pooled levels read once"},
        "config": "Faster R-CNN ResNet-50 FPN, fp32, min_size 600 / max_size 1000, synthetic VOC-shaped pool resident in HBM",
        "device": torch.cuda.get_device_name(0), "csrc_sha1": csrc_sha1(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
