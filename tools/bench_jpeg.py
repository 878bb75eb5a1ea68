#!/usr/bin/env python
"""Informational: GPU JPEG decode throughput vs Pillow on this host.
Encodes N VOC-shaped synthetic images with Pillow (quality 90, 4:2:0; --progressive: all of them progressive;
--mixed FRACTION: that fraction of them, evenly spread), then times
  * DevicePool.from_jpeg_bytes (files already in host memory, GPU decode),
  * the host fallback route on the same files: Pillow decode in this one process + DevicePool.from_arrays, and
  * PIL.Image.open(...).convert('RGB') alone on one core.
Prints one JSON line."""
import argparse
import io
import json
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from cald_amd import pool, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=512)
ap.add_argument("--progressive", action="store_true", help="encode every file with progressive=True")
ap.add_argument("--mixed", type=float, default=None, metavar="FRACTION", help="encode this fraction of the files progressive")
args = ap.parse_args()
n = args.n
frac = 1.0 if args.progressive else (args.mixed or 0.0)
imgs = synth.make_pool(min(n, 64), "voc", 0)
blobs = []
for i in range(n):
    bio = io.BytesIO()
    progressive = int((i + 1) * frac) > int(i * frac)
    Image.fromarray(imgs[i % len(imgs)]).save(bio, "JPEG", quality=90, subsampling=2, progressive=progressive)
    blobs.append(bio.getvalue())
pool.DevicePool.from_jpeg_bytes(blobs[:8])            # warm up (module load, first launches)
pool.DevicePool.from_jpeg_bytes(blobs[-8:])
torch.cuda.synchronize()
res = {}
for chunk in (64, 512):
    t0 = time.time()
    dp = pool.DevicePool.from_jpeg_bytes(blobs, chunk=chunk)
    torch.cuda.synchronize()
    res["gpu_images_per_s_chunk%d" % chunk] = n / (time.time() - t0)
m = min(n, 200)
t0 = time.time()
arrays = [np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in blobs[:m]]
t_pil = time.time() - t0
pool.DevicePool.from_arrays(arrays)
torch.cuda.synchronize()
res["pillow_images_per_s_1core"] = m / t_pil
res["fallback_images_per_s"] = m / (time.time() - t0)  # what every file would cost on the host route
ok = all(np.array_equal(dp[i].cpu().numpy(), np.asarray(Image.open(io.BytesIO(blobs[i])).convert("RGB"))) for i in range(0, n, max(1, n // 16)))
res.update(n=n, progressive_fraction=frac, decode_counts=dp.decode_counts, file_MB=sum(len(b) for b in blobs) / 1e6,
           decoded_MB=dp.nbytes / 1e6, bit_identical_to_pillow=bool(ok))
print(json.dumps(res))
