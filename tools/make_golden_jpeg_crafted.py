#!/usr/bin/env python
"""Writes tests/golden/jpeg_crafted.npz: the 12 over-range files of tests/test_jpeg_crafted.py (gray 8 x 32, q = 1,
DC = +-1000, the first 1, 3 or 6 AC coefficients at +-300 / 600 / 900 / 1023), each with the RGB image Pillow decodes
from it, and the versions of Pillow and libjpeg-turbo that decoded.  Their inverse DCT leaves the 10-bit range-limit
table of libjpeg's C code, which wraps there; libjpeg-turbo's SIMD code saturates.  The fixture records the saturating
output, whatever Pillow the test machine has.  Keys: n, name_i, file_i, rgb_i, pillow_version, libjpeg_turbo_version."""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_writer as jw  # noqa: E402


def main():
    out = {}
    blobs = jw.overrange_blobs()
    for i, (name, b) in enumerate(blobs):
        out["name_%d" % i] = np.array(name)
        out["file_%d" % i] = np.frombuffer(b, np.uint8)
        out["rgb_%d" % i] = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    out["n"] = np.int64(len(blobs))
    out["pillow_version"] = np.array(PIL.__version__)
    out["libjpeg_turbo_version"] = np.array(str(features.version("libjpeg_turbo")))
    path = os.path.join(ROOT, "tests", "golden", "jpeg_crafted.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(blobs), "cases, Pillow", PIL.__version__, "libjpeg-turbo", features.version("libjpeg_turbo"))


if __name__ == "__main__":
    main()
