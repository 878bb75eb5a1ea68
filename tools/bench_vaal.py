"""Throughput of the VAAL sweep (cald_sweep_vaal) on one MI355X over an HBM-resident pool, beside the torch-ROCm execution of this
package's own VAE / Discriminator modules the way the reference's sampler runs them: loader batch 1, the VAE in train() mode, the full
forward including the unused decoder and its host-side randn (vaal_helper.py:186-216).

Both are warmed up, then alternated `--rounds` times in one process; a round is timed with HIP events on the launch stream between two
device synchronisations, whole call (host work included).  The torch side gets its images already converted to float CHW in HBM (the
reference's loader does that on the CPU), so only what the sampler itself runs is timed.  The two sides' predictions are compared.

FLOPs and bytes are counted from the shapes: FLOPs = 2 x the multiply-adds of the five convolutions, fc_mu and the head; bytes = what the
launch sequence as built moves per image (resize write + read, per layer the conv output written, read three times by the statistics and
the normalisation, written once and read by the next layer) plus the packed weights once per launch sequence.  Both rates are whole-call
figures over the event time, not a kernel's share of peak.

    python tools/bench_vaal.py [--images 1024] [--torch-images 256] [--rounds 3] [--repeats 8] [--out profiles/vaal_sweep_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from cald_amd import synth, vaal
from cald_amd.pool import DevicePool

PEAK_FP32_TFLOPS = 157.3   # MI355X vector / matrix fp32 peak
COPY_RATE_TBPS = 6.29      # measured float4 copy rate of an MI355X (8.0 TB/s HBM3E peak)
WIDTHS = (3, 64, 128, 256, 512, 1024)


def csrc_sha1():
    import hashlib
    h = hashlib.sha1()
    d = os.path.join(ROOT, "cald_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")) or f == "Makefile":
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def counts(batch):
    """(FLOPs per image, bytes per image at `batch` images per launch sequence) from the shapes."""
    macs, act, wbytes = 0, 2 * 65536 * 4 * 4, 0
    for l in range(5):
        pix = (128 >> l) ** 2
        macs += pix * WIDTHS[l + 1] * 16 * WIDTHS[l]
        act += 6 * pix * WIDTHS[l + 1] * 4
        wbytes += 16 * max(WIDTHS[l], 4) * WIDTHS[l + 1] * 4
    macs += 65536 * 256 + 256 * 512 + 512 * 512 + 512
    act += 2 * 256 * 256 * 4                                  # fc_mu's segment sums, written and read
    wbytes += (65536 * 256 + 256 * 512 + 512 * 512 + 512) * 4
    return 2.0 * macs, act + wbytes / float(batch)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024); ap.add_argument("--torch-images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--batch-images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=8, help="sweeps of the pool per timed window (one sweep of 1 024 images is 60 ms)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vaal_sweep_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vaal.py measures on an MI355X; there is no CPU path")
    torch.manual_seed(0)
    vae, disc = vaal.VAE(), vaal.Discriminator()
    with torch.no_grad():                                     # non-trivial biases and affine terms; train mode ignores the running statistics
        for m in vae.encoder:
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0.0, 0.1)
    vae.train()
    model = vaal.VaalModel(vae, disc)
    vae, disc = vae.cuda(), disc.cuda()
    pool = DevicePool.from_arrays(synth.make_pool(a.images, "voc", 0))
    images = [pool[i] for i in range(len(pool))]
    nt = min(a.torch_images, len(images))
    chw = [im.permute(2, 0, 1).float().div(255).contiguous() for im in images[:nt]]

    def run_hip(n=len(images)):
        return vaal.vaal_sweep_device_images(model, None, images[:n], batch_images=a.batch_images)

    def run_torch(n=nt):
        preds = []
        with torch.no_grad():
            for img in chw[:n]:
                x = F.interpolate(img.unsqueeze(0), (256, 256))
                _, _, mu, _ = vae(x)
                preds.extend(disc(mu))
        return torch.stack(preds).view(-1).cpu().numpy()

    run_hip(min(len(images), 2 * a.batch_images)); run_torch(min(nt, 16))
    hip_ms, torch_ms, first = [], [], None
    for _ in range(a.rounds):
        ps, t = timed(lambda: [run_hip() for _ in range(a.repeats)]); hip_ms.append(t / a.repeats)
        assert all(np.array_equal(p, ps[0]) for p in ps) and (first is None or np.array_equal(ps[0], first)), "the VAAL sweep is not reproducible"
        first = ps[0]
        pt, t = timed(run_torch); torch_ms.append(t)
    diff = float(np.abs(first[:nt].astype(np.float64) - pt.astype(np.float64)).max())
    assert diff < 1e-3, "the sweep and torch disagree: %g" % diff
    n = len(images)
    hip_ips = [n / (t / 1e3) for t in hip_ms]; torch_ips = [nt / (t / 1e3) for t in torch_ms]
    flops, nbytes = counts(min(a.batch_images if a.batch_images > 0 else 64, n))
    ips = float(np.median(hip_ips))
    res = {
        "metric": "VAAL sweep throughput (resize + VAE encoder with batch statistics + fc_mu + discriminator)", "unit": "images/s",
        "value": ips, "vaal_images_per_s": hip_ips, "torch_images_per_s": torch_ips, "torch_median_images_per_s": float(np.median(torch_ips)),
        "vaal_over_torch": ips / float(np.median(torch_ips)),
        "gflop_per_image": flops / 1e9, "achieved_tflops": ips * flops / 1e12, "share_of_fp32_peak": ips * flops / 1e12 / PEAK_FP32_TFLOPS,
        "mbytes_per_image": nbytes / 1e6, "achieved_hbm_tbps": ips * nbytes / 1e12, "share_of_copy_rate": ips * nbytes / 1e12 / COPY_RATE_TBPS,
        "bound": "compute: %.3g us per image at the fp32 peak against %.3g us at the copy rate" % (flops / PEAK_FP32_TFLOPS / 1e6, nbytes / COPY_RATE_TBPS / 1e6),
        "max_abs_pred_difference_to_torch": diff,
        "images": n, "torch_images": nt, "rounds": a.rounds, "sweeps_per_window": a.repeats, "batch_images": a.batch_images,
        "torch_side": "this package's VAE / Discriminator on torch-ROCm: batch 1, train() mode, full forward with decoder and host randn, float CHW images resident in HBM",
        "timing": "HIP events on the launch stream between two device synchronisations, whole call (host work included); the two sides alternated; "
                  "rates are whole-call figures over shape-counted FLOPs and bytes, not kernel shares of peak",
        "config": "exact fp32, synthetic VOC-shaped pool resident in HBM, peaks %.1f TFLOPS fp32 / %.2f TB/s float4 copy" % (PEAK_FP32_TFLOPS, COPY_RATE_TBPS),
        "device": torch.cuda.get_device_name(0), "csrc_sha1": csrc_sha1(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
