#!/usr/bin/env python
"""Writes tests/golden/jpeg_progressive_cases.npz: progressive JPEG files (colour 4:4:4 / 4:2:2 / 4:2:0, gray, with and
without restart intervals) and one RGB-coded file, each with the RGB image Pillow decodes from it.  Same key layout as
jpeg_cases.npz (n, file_i, rgb_i).  The fixture pins the decoder to one recorded Pillow / libjpeg-turbo output,
whatever Pillow the test machine has."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cald_amd import synth  # noqa: E402

# (H, W), quality, subsampling (None = gray), restart_marker_blocks (0 = none)
CASES = [((1, 1), 75, 2, 0), ((2, 3), 90, 0, 0), ((8, 8), 35, 1, 0), ((17, 23), 75, 2, 3), ((33, 31), 97, 1, 0),
         ((5, 40), 90, None, 0), ((3, 200), 75, 0, 2), ((200, 3), 35, 2, 0), ((64, 48), 90, None, 5), ((100, 75), 97, 0, 0),
         ((120, 160), 75, 1, 7), ((100, 140), 90, 2, 0)]


def image(k, H, W):
    a = np.ascontiguousarray(synth.synth_image(7000 + k, max(H, 33), max(W, 33))[:H, :W])
    if k % 2 == 0:
        rng = np.random.default_rng(k)
        a = (a.astype(np.int32) + rng.integers(-20, 21, a.shape)).clip(0, 255).astype(np.uint8)
    return a


def main():
    out = {}
    blobs = []
    for k, ((H, W), quality, sub, rst) in enumerate(CASES):
        im = Image.fromarray(image(k, H, W))
        kw = dict(quality=quality, progressive=True)
        if sub is None:
            im = im.convert("L")
        else:
            kw["subsampling"] = sub
        if rst:
            kw["restart_marker_blocks"] = rst
        bio = io.BytesIO()
        im.save(bio, "JPEG", **kw)
        blobs.append(bio.getvalue())
    bio = io.BytesIO()
    Image.fromarray(image(99, 40, 56)).save(bio, "JPEG", quality=85, keep_rgb=True)
    blobs.append(bio.getvalue())
    for i, b in enumerate(blobs):
        out["file_%d" % i] = np.frombuffer(b, np.uint8)
        out["rgb_%d" % i] = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    out["n"] = np.int64(len(blobs))
    path = os.path.join(ROOT, "tests", "golden", "jpeg_progressive_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(blobs), "cases")


if __name__ == "__main__":
    main()
