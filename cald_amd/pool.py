"""Input side of the sweep: the unlabeled pool kept resident in HBM.

The reference re-reads and re-decodes every pool image on the CPU in every active-learning cycle
(``DataLoader(dataset_aug, batch_size=1, sampler=SubsetSequentialSampler(subset), num_workers=...)``,
cald_train.py:434; ``Image.open(path).convert('RGB')`` in torchvision's VOCDetection.__getitem__ reached from
detection/voc_utils.py:47-58; ``ToTensor`` in detection/train.py:54-59).  A MI355X has 288 GB of HBM: all of
VOC07+12 trainval as uint8 RGB is 9 GB, COCO train2017 about 90 GB.  ``DevicePool`` therefore decodes each JPEG
ONCE, on the GPU (``cald_jpeg_decode_batch_any``: bit-identical to Pillow, except for files whose dequantised
coefficients do not fit int16, which no encoder makes from 8-bit samples), keeps the uint8 HWC images in one HBM arena,
and hands the sweep device pointers; later cycles only change the subset of positions.

Which file goes where (``jpeg_probe``): baseline and progressive 8-bit Huffman JPEGs (gray, YCbCr or RGB-coded; 4:4:4,
4:2:2, 4:2:0) are decoded on the GPU.  Every other file -- CMYK, arithmetic-coded, 12-bit, multi-scan sequential,
progressive with an incomplete or rule-breaking scan script, truncated, or not a JPEG at all -- is decoded per file by
Pillow on the host (``fallback="pillow"``, the default), so one odd file never fails a pool.  ``jpeg_info`` and
``decode_jpeg_batch`` are the strict entry points: baseline only, no host decode, ever.

``pool.loader(subset)`` yields ``([image], [None])`` batches of one (``batch_size=`` makes them larger), i.e. it can be passed wherever the reference
passes ``unlabeled_loader`` (``cald_amd.sweep.get_uncertainty`` takes uint8 HWC CUDA tensors as they are).
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi


def jpeg_info(data):
    """(H, W, ncomp) of a JPEG byte string (host-only header parse)."""
    buf = np.frombuffer(data, np.uint8)
    H, W, nc = C.c_int(), C.c_int(), C.c_int()
    _ffi.check(_ffi.lib().cald_jpeg_info(buf.ctypes.data, buf.size, C.byref(H), C.byref(W), C.byref(nc)))
    return H.value, W.value, nc.value


def decode_jpeg_batch(blobs, outs=None, ctx=None):
    """Decodes JPEG byte strings on the GPU.  Returns a list of uint8 [H][W][3] CUDA tensors (RGB), equal to
    ``np.asarray(Image.open(io.BytesIO(b)).convert('RGB'))``.  ``outs`` (optional): preallocated tensors."""
    from .detector import get_ctx
    L = _ffi.lib()
    n = len(blobs)
    if n == 0:
        return []
    bufs = [np.frombuffer(b, np.uint8) for b in blobs]
    if outs is None:
        dev = torch.device("cuda", torch.cuda.current_device())
        outs = []
        for b in blobs:
            H, W, _ = jpeg_info(b)
            outs.append(torch.empty((H, W, 3), dtype=torch.uint8, device=dev))
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (C.c_size_t * n)(*[b.size for b in bufs])
    optrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    _ffi.check(L.cald_jpeg_decode_batch(ctx if ctx is not None else get_ctx(), n, ptrs, sizes, optrs))
    return outs


JPEG_BASELINE, JPEG_GPU_EXTENDED, JPEG_HOST_ONLY = 0, 1, 2      # CALD_JPEG_* of include/cald_hip.h
_COUNT_KEYS = ("gpu_baseline", "gpu_extended", "host")


def jpeg_probe(data):
    """(H, W, ncomp, kind) of a JPEG byte string (host-only parse of the headers and, for a progressive file, of its
    scan script).  kind: JPEG_BASELINE (what ``decode_jpeg_batch`` takes), JPEG_GPU_EXTENDED (``decode_images`` decodes
    it on the GPU) or JPEG_HOST_ONLY (a JPEG for the host fallback).  Bytes that are not a JPEG raise RuntimeError."""
    buf = np.frombuffer(data, np.uint8)
    H, W, nc, kind = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _ffi.check(_ffi.lib().cald_jpeg_probe(buf.ctypes.data, buf.size, C.byref(H), C.byref(W), C.byref(nc), C.byref(kind)))
    return H.value, W.value, nc.value, kind.value


def decode_jpeg_host(data):
    """CPU restatement of the GPU decoder (baseline and GPU_EXTENDED files): uint8 [H][W][3] numpy array.  Needs no GPU."""
    H, W, _, kind = jpeg_probe(data)
    buf = np.frombuffer(data, np.uint8)
    out = np.empty((H, W, 3), np.uint8) if kind != JPEG_HOST_ONLY else np.empty((0, 0, 3), np.uint8)
    _ffi.check(_ffi.lib().cald_jpeg_decode_host(buf.ctypes.data, buf.size, out.ctypes.data))
    return out


def _pillow_rgb(blob, index, name=None):
    """Image.open(...).convert('RGB') of one file; Pillow's own error, with the file's position (and path) added."""
    import io
    from PIL import Image
    try:
        return np.array(Image.open(io.BytesIO(blob)).convert("RGB"))
    except Exception as e:
        where = "image %d" % index + (" (%s)" % name if name is not None else "")
        try:
            err = type(e)("%s: %s" % (where, e))
        except Exception:          # an error type with a constructor of its own: re-raise it as it is
            raise e
        raise err from e


class _Plan:
    """What a decode does with each file: its probe result, and the host-decoded array where the GPU does not take it."""

    def __init__(self, blobs, fallback="pillow", names=None):
        if fallback not in ("pillow", None):
            raise ValueError("fallback must be 'pillow' or None")
        self.kinds, self.shapes, self.host = [], [], {}
        for i, b in enumerate(blobs):
            kind, H, W = JPEG_HOST_ONLY, 0, 0
            try:
                H, W, _, kind = jpeg_probe(b)
            except RuntimeError:
                if fallback is None:
                    raise
            if kind == JPEG_HOST_ONLY:
                if fallback is None:
                    raise NotImplementedError("image %d: a JPEG flavour the GPU path does not decode, and fallback=None" % i)
                self.host[i] = _pillow_rgb(b, i, None if names is None else names[i])
                H, W = self.host[i].shape[:2]
            self.kinds.append(kind)
            self.shapes.append((H, W))

    def counts(self):
        return {k: self.kinds.count(v) for k, v in zip(_COUNT_KEYS, (JPEG_BASELINE, JPEG_GPU_EXTENDED, JPEG_HOST_ONLY))}


def _decode_planned(blobs, outs, kinds, host, ctx=None):
    """One GPU call for the files whose kind is not HOST_ONLY, one copy for each array in host = {index: uint8 HWC}."""
    from .detector import get_ctx
    gpu = [i for i in range(len(blobs)) if kinds[i] != JPEG_HOST_ONLY]
    if gpu:
        bufs = [np.frombuffer(blobs[i], np.uint8) for i in gpu]
        ptrs = (C.c_void_p * len(gpu))(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * len(gpu))(*[b.size for b in bufs])
        optrs = (C.c_void_p * len(gpu))(*[outs[i].data_ptr() for i in gpu])
        _ffi.check(_ffi.lib().cald_jpeg_decode_batch_any(ctx if ctx is not None else get_ctx(), len(gpu), ptrs, sizes, optrs))
    for i, a in host.items():
        outs[i].copy_(torch.from_numpy(a))
    return outs


def decode_images(blobs, outs=None, fallback="pillow", ctx=None):
    """Decodes image files to uint8 [H][W][3] CUDA tensors (RGB), each equal to
    ``np.asarray(Image.open(io.BytesIO(b)).convert('RGB'))``.  Baseline and GPU_EXTENDED JPEGs (see ``jpeg_probe``) go to
    the GPU in one ``cald_jpeg_decode_batch_any`` call.  With ``fallback="pillow"`` every other file -- HOST_ONLY JPEGs
    and files that are no JPEG, such as PNG or BMP -- is decoded by Pillow on the host and copied into its output; a file
    Pillow cannot open raises Pillow's error with the index added.  With ``fallback=None`` such a file raises
    NotImplementedError (HOST_ONLY) or RuntimeError (not a JPEG), as the strict API does.  ``outs`` (optional):
    preallocated tensors."""
    if len(blobs) == 0:
        return []
    plan = _Plan(blobs, fallback)
    if outs is None:
        dev = torch.device("cuda", torch.cuda.current_device())
        outs = [torch.empty((H, W, 3), dtype=torch.uint8, device=dev) for H, W in plan.shapes]
    return _decode_planned(blobs, outs, plan.kinds, plan.host, ctx)


class DevicePool:
    """uint8 HWC images resident in one HBM arena, addressed by pool position."""

    def __init__(self, arena, offsets, shapes):
        self.arena = arena            # 1-D uint8 CUDA tensor
        self.offsets = offsets        # int64 [n]
        self.shapes = shapes          # [(H, W)]
        self.decode_counts = dict.fromkeys(_COUNT_KEYS, 0)   # files per decode route (from_jpeg_bytes / from_files)

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, i):
        H, W = self.shapes[i]
        o = int(self.offsets[i])
        return self.arena[o:o + H * W * 3].view(H, W, 3)

    @property
    def nbytes(self):
        return int(self.arena.numel())

    @staticmethod
    def _layout(shapes):
        offsets = np.zeros(len(shapes), np.int64)
        off = 0
        for i, (H, W) in enumerate(shapes):
            offsets[i] = off
            off += (H * W * 3 + 255) & ~255            # 256-byte aligned images
        return offsets, off

    @classmethod
    def from_jpeg_bytes(cls, blobs, chunk=512, device=None, fallback="pillow", _names=None):
        """Decode-once constructor: header parse on the host, everything else on the GPU, ``chunk`` files per call
        (bounds the coefficient workspace: about 0.9 MB per VOC-sized image).  Files the GPU path does not take are
        decoded by Pillow, one by one (``fallback="pillow"``; see ``decode_images``); ``fallback=None`` raises instead.
        ``pool.decode_counts`` says how many files took which route."""
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        plan = _Plan(blobs, fallback, _names)                 # each file is probed (or opened by Pillow) once
        shapes = plan.shapes
        offsets, total = cls._layout(shapes)
        arena = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        pool = cls(arena, offsets, shapes)
        pool.decode_counts = plan.counts()
        for s in range(0, len(blobs), chunk):
            idx = range(s, min(s + chunk, len(blobs)))
            _decode_planned([blobs[i] for i in idx], [pool[i] for i in idx], [plan.kinds[i] for i in idx],
                            {i - s: plan.host[i] for i in idx if i in plan.host})
        return pool

    @classmethod
    def from_files(cls, paths, chunk=512, device=None, fallback="pillow"):
        blobs = []
        for p in paths:
            with open(p, "rb") as f:
                blobs.append(f.read())
        return cls.from_jpeg_bytes(blobs, chunk, device, fallback, _names=[str(p) for p in paths])

    @classmethod
    def from_arrays(cls, arrays, device=None):
        """Already-decoded uint8 HWC arrays (decoded by the caller)."""
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        arrays = [np.array(a, dtype=np.uint8, order="C") for a in arrays]
        shapes = [a.shape[:2] for a in arrays]
        offsets, total = cls._layout(shapes)
        arena = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        pool = cls(arena, offsets, shapes)
        for i, a in enumerate(arrays):
            pool[i].copy_(torch.from_numpy(a), non_blocking=True)
        return pool

    def loader(self, subset=None, rank=0, world_size=1, batch_size=1):
        """Iterable with the reference loader's batch shape: (images: list of batch_size, targets: list of batch_size; the
        last batch may be short).  With world_size > 1 only this rank's strided shard subset[rank::world_size] is yielded
        (pass ``loader_is_sharded=True`` to get_uncertainty).  batch_size > 1 is what the learning-loss sweep's loader has
        (ll_train.py:265-268; ``baselines.ll_get_uncertainty`` pads a batch's images to their common size)."""
        order = range(len(self)) if subset is None else subset
        mine = list(order)[rank::world_size]
        for s in range(0, len(mine), batch_size):
            part = mine[s:s + batch_size]
            yield [self[int(i)] for i in part], [None] * len(part)
