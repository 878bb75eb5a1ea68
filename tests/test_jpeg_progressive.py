"""Input side: progressive JPEGs on the GPU, and a pool that never fails on one file.

Chain of evidence: Pillow (= what the reference runs: Image.open(path).convert('RGB')) -> golden fixtures
(tests/golden/jpeg_progressive_cases.npz, written by tools/make_golden_jpeg_progressive.py) -> cald_jpeg_decode_host (the
kernels' own __host__ __device__ functions driven by loops, no GPU) -> the HIP decoder (cald_jpeg_decode_batch_any).
Bit-exact at every link.  A progressive file carries the same quantised coefficients as the baseline file of the same
image, quality and subsampling, so the new decoder on the one must equal the old decoder on the other: a check that
needs no Pillow at decode time.
"""
import io

import numpy as np
import pytest

try:
    from PIL import Image, ImageFile
    ImageFile.MAXBLOCK = 1 << 24
except Exception:  # pragma: no cover
    Image = None

needs_pillow = pytest.mark.skipif(Image is None, reason="Pillow not importable")

SIZES = [(1, 1), (2, 3), (8, 8), (16, 16), (17, 23), (33, 31), (5, 40), (3, 200), (200, 3), (64, 48), (100, 75), (120, 160),
         (375, 500), (480, 640)]


def _golden_cases(golden, name="jpeg_progressive_cases"):
    g = golden(name)
    return [(g["file_%d" % i].tobytes(), g["rgb_%d" % i]) for i in range(int(g["n"]))]


def _encode(a, gray=False, mode=None, fmt="JPEG", **kw):
    im = Image.fromarray(a)
    if gray:
        im = im.convert("L")
    if mode:
        im = im.convert(mode)
    bio = io.BytesIO()
    im.save(bio, fmt, **kw)
    return bio.getvalue()


def _pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _sweep():
    """[(progressive file, baseline file)] of the same image, quality and subsampling: every size crossed with
    subsampling 0 / 1 / 2 and gray, qualities 35 / 75 / 90 / 97 in turn, restart markers on every fifth case."""
    from cald_amd import synth
    rng = np.random.default_rng(11)
    pairs, k = [], 0
    for H, W in SIZES:
        a = np.ascontiguousarray(synth.synth_image(5000 + k, max(H, 33), max(W, 33))[:H, :W])
        if (H * W) % 3 == 0:
            a = (a.astype(np.int32) + rng.integers(-20, 21, a.shape)).clip(0, 255).astype(np.uint8)
        for sub in (0, 1, 2, None):
            kw = dict(quality=[35, 75, 90, 97][k % 4])
            if sub is not None:
                kw["subsampling"] = sub
            if k % 5 == 4:
                kw["restart_marker_blocks"] = 1 + k % 7
            pairs.append((_encode(a, gray=sub is None, progressive=True, **kw), _encode(a, gray=sub is None, optimize=True, **kw)))
            k += 1
    return pairs


def _cut_script(blob, keep_scans):
    """The file up to its SOS marker number `keep_scans` (0-based), closed with an EOI: a progressive file whose scan
    script stops early.  Pillow opens it without error and smooths what is missing."""
    at, p = [], 0
    while True:
        p = blob.find(b"\xff\xda", p)
        if p < 0:
            break
        at.append(p)
        p += 2
    return blob[:at[keep_scans]] + b"\xff\xd9", len(at)


def _flavours():
    """name -> (file bytes, expected probe kind or None for "not a JPEG", ncomp)"""
    from cald_amd import pool, synth
    a = np.ascontiguousarray(synth.synth_image(77, 56, 72))
    prog = _encode(a, progressive=True, quality=85)
    cut, nscan = _cut_script(prog, -1)
    assert nscan == 10
    return {
        "baseline": (_encode(a, quality=85), pool.JPEG_BASELINE, 3),
        "progressive": (prog, pool.JPEG_GPU_EXTENDED, 3),
        "progressive_gray": (_encode(a, gray=True, progressive=True), pool.JPEG_GPU_EXTENDED, 1),
        "keep_rgb": (_encode(a, keep_rgb=True), pool.JPEG_GPU_EXTENDED, 3),
        "cmyk": (_encode(a, mode="CMYK"), pool.JPEG_HOST_ONLY, 4),
        "cmyk_progressive": (_encode(a, mode="CMYK", progressive=True), pool.JPEG_HOST_ONLY, 4),
        "cut_script": (cut, pool.JPEG_HOST_ONLY, 3),
        "png": (_encode(a, fmt="PNG"), None, 0),
    }


# ------------------------------------------------------------------ CPU
@needs_pillow
def test_probe_sorts_files_into_baseline_gpu_extended_and_host_only():
    from cald_amd import pool
    for name, (blob, kind, nc) in _flavours().items():
        if kind is None:
            with pytest.raises(RuntimeError):
                pool.jpeg_probe(blob)
            continue
        assert pool.jpeg_probe(blob) == (56, 72, nc, kind), name
    with pytest.raises(RuntimeError):
        pool.jpeg_probe(b"\x89PNG not a jpeg")
    # a script cut at any of its SOS markers leaves some coefficient short of Al = 0: never for the GPU
    prog = _flavours()["progressive"][0]
    for k in range(1, 10):
        cut, _ = _cut_script(prog, k)
        assert pool.jpeg_probe(cut) == (56, 72, 3, pool.JPEG_HOST_ONLY), k
        with pytest.raises(NotImplementedError):
            pool.decode_jpeg_host(cut)
    # a file that stops in the middle of a scan is for libjpeg to diagnose
    assert pool.jpeg_probe(prog[:len(prog) * 2 // 3])[3] == pool.JPEG_HOST_ONLY
    # the strict entry point still refuses what the probe sorts
    with pytest.raises(NotImplementedError):
        pool.jpeg_info(prog)


def test_host_decode_matches_pillow_golden(golden):
    from cald_amd import pool
    cases = _golden_cases(golden) + _golden_cases(golden, "jpeg_cases")       # progressive + RGB-coded, then baseline
    assert len(cases) > 13
    for i, (data, ref) in enumerate(cases):
        H, W, _, kind = pool.jpeg_probe(data)
        assert (H, W) == ref.shape[:2] and kind != pool.JPEG_HOST_ONLY, i
        assert np.array_equal(pool.decode_jpeg_host(data), ref), i
    assert sum(pool.jpeg_probe(d)[3] == pool.JPEG_GPU_EXTENDED for d, _ in cases) == 13


@needs_pillow
def test_host_decode_matches_live_pillow_over_the_sweep():
    from cald_amd import pool
    for i, (prog, base) in enumerate(_sweep()):
        assert pool.jpeg_probe(prog)[3] == pool.JPEG_GPU_EXTENDED and pool.jpeg_probe(base)[3] == pool.JPEG_BASELINE, i
        assert np.array_equal(pool.decode_jpeg_host(prog), _pil_decode(prog)), i
        assert np.array_equal(pool.decode_jpeg_host(base), _pil_decode(base)), i
    rgb = _flavours()["keep_rgb"][0]
    assert np.array_equal(pool.decode_jpeg_host(rgb), _pil_decode(rgb))


@needs_pillow
def test_progressive_decode_equals_baseline_decode_of_the_same_coefficients():
    """No Pillow at decode time: progression only reorders the quantised coefficients."""
    from cald_amd import pool
    for i, (prog, base) in enumerate(_sweep()):
        assert np.array_equal(pool.decode_jpeg_host(prog), pool.decode_jpeg_host(base)), i


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@needs_pillow
def test_gpu_mixed_batch_is_bit_exact(golden):
    import torch
    from cald_amd import pool
    pairs = _sweep()
    blobs, want = [], []
    for i, (prog, base) in enumerate(pairs):          # every progressive case, every other baseline case, interleaved
        blobs.append(prog)
        if i % 2:
            blobs.append(base)
    want = [_pil_decode(b) for b in blobs]
    for data, ref in _golden_cases(golden):
        blobs.append(data)
        want.append(ref)
    outs = pool.decode_images(blobs, fallback=None)
    torch.cuda.synchronize()
    baseline = [i for i, b in enumerate(blobs) if pool.jpeg_probe(b)[3] == pool.JPEG_BASELINE]
    assert len(baseline) == len(pairs) // 2
    strict = pool.decode_jpeg_batch([blobs[i] for i in baseline])
    for i, (b, o, ref) in enumerate(zip(blobs, outs, want)):
        got = o.cpu().numpy()
        assert np.array_equal(got, ref), i
        assert np.array_equal(got, pool.decode_jpeg_host(b)), i
    for i, o in zip(baseline, strict):
        assert torch.equal(o, outs[i]), i


@pytest.mark.gpu
@needs_pillow
def test_gpu_pool_falls_back_per_file(tmp_path):
    from cald_amd import pool
    fl = _flavours()
    order = ["baseline", "cmyk", "progressive", "png", "progressive_gray", "cut_script", "keep_rgb"]
    paths = []
    for name in order:
        p = tmp_path / (name + (".png" if name == "png" else ".jpg"))
        p.write_bytes(fl[name][0])
        paths.append(str(p))
    dp = pool.DevicePool.from_files(paths, chunk=3)
    assert dp.decode_counts == {"gpu_baseline": 1, "gpu_extended": 3, "host": 3}
    assert len(dp) == len(paths)
    for i, p in enumerate(paths):
        assert np.array_equal(dp[i].cpu().numpy(), np.asarray(Image.open(p).convert("RGB"))), order[i]
    with pytest.raises(NotImplementedError):
        pool.DevicePool.from_files(paths, chunk=3, fallback=None)
    with pytest.raises(NotImplementedError):
        pool.decode_images([fl["baseline"][0], fl["cmyk"][0]], fallback=None)
    with pytest.raises(RuntimeError):
        pool.decode_images([fl["png"][0]], fallback=None)
    broken = tmp_path / "broken.jpg"
    broken.write_bytes(fl["progressive"][0][:len(fl["progressive"][0]) // 2])
    with pytest.raises(OSError, match="broken.jpg"):
        pool.DevicePool.from_files(paths[:2] + [str(broken)], chunk=3)


@pytest.mark.gpu
@needs_pillow
def test_gpu_progressive_device_pool_sweep_equals_loader_sweep():
    """Progressive files -> DevicePool (GPU decode) -> get_uncertainty == the same sweep fed by a reference-style loader of
    PIL-decoded float CHW tensors, position for position."""
    import torch
    from cald_amd import detector, pool, synth, sweep
    model = detector.fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=300, max_size=500).to("cuda")
    model.load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0))
    model.eval()
    imgs = [np.ascontiguousarray(synth.synth_image(40 + i, 200 + 16 * i, 300 - 8 * i)) for i in range(5)]
    blobs = [_encode(a, quality=88, subsampling=2, progressive=True) for a in imgs]
    dp = pool.DevicePool.from_jpeg_bytes(blobs, chunk=2)
    assert dp.decode_counts == {"gpu_baseline": 0, "gpu_extended": 5, "host": 0}
    for i, b in enumerate(blobs):
        assert np.array_equal(dp[i].cpu().numpy(), _pil_decode(b))
    augs = ["flip", "cut_out", "smaller_resize"]
    subset = [3, 0, 4, 1]
    u_pool, c_pool = sweep.get_uncertainty(model, dp.loader(subset), augs, 21, base_seed=9)
    ref_loader = [([torch.from_numpy(_pil_decode(blobs[i]).copy()).permute(2, 0, 1).float().div(255)], [None]) for i in subset]
    u_ref, c_ref = sweep.get_uncertainty(model, ref_loader, augs, 21, base_seed=9)
    assert u_pool == u_ref
    assert all(np.array_equal(a, b) for a, b in zip(c_pool, c_ref))


@pytest.mark.gpu
@needs_pillow
def test_gpu_voc_dataset_pool_takes_progressive_and_cmyk_files(tmp_path):
    from cald_amd import synth, voc_utils as vu
    imgs = synth.make_pool(9, "voc", 5, scale=0.5)
    base = tmp_path / "VOCdevkit" / "VOC2007"
    for d in ("ImageSets/Main", "Annotations", "JPEGImages"):
        (base / d).mkdir(parents=True)
    stems = ["%06d" % (7 * i + 3) for i in range(len(imgs))]
    for i, (im, stem) in enumerate(zip(imgs, stems)):
        pil = Image.fromarray(im)
        if i == 4:
            pil = pil.convert("CMYK")
        pil.save(str(base / "JPEGImages" / (stem + ".jpg")), quality=92, subsampling=(0, 1, 2)[i % 3], progressive=i % 3 == 2)
        H, W = im.shape[:2]
        obj = ("<object><name>%s</name><difficult>0</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax>"
               "</bndbox></object>" % (vu.VOC_CLASSES[1 + i], 2, 3, W // 2, H // 2))
        (base / "Annotations" / (stem + ".xml")).write_text("<annotation><filename>%s.jpg</filename>%s</annotation>" % (stem, obj))
    (base / "ImageSets" / "Main" / "trainval.txt").write_text("".join(s + "\n" for s in stems))
    ds = vu.get_voc2007(str(tmp_path), "trainval", None)
    dp = ds.device_pool()
    assert dp.decode_counts == {"gpu_baseline": 5, "gpu_extended": 3, "host": 1}
    for i in range(len(ds)):
        assert np.array_equal(dp[i].cpu().numpy(), np.asarray(Image.open(ds.images[i]).convert("RGB"))), i
