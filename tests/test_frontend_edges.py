"""The augmentation front end (cald_amd/csrc/elementwise.hip) against LIVE torch and Pillow at its edges.

Chain of evidence: live torch / Pillow calls (= what the reference's cald_helper executes) -> the CPU oracle's restatement
(oracle/cald_oracle.c) -> the HIP kernels (noise_stream_kernel, pil_horizontal_kernel / pil_vertical_kernel,
affine_nearest_kernel, color_brightness_kernel / color_contrast_saturation_kernel).  The CPU half pins the first link
without a GPU, the GPU half the kernels against both the oracle (bit for bit) and the live calls.

Integer results (uniform draws, salt-and-pepper / resized / rotated / colour-adjusted images) are compared exactly.  The
Gaussian term randn * std / 255 is compared within 2e-6 * std / 16: torch evaluates log / sin / cos with its vector math
library, the contract with det_logf / det_sincosf; 2e-6 is the project's bound for std 16 (test_gpu_parity.py) and the
term is linear in std.  Kernel against oracle the Gaussian term is bit-exact too.

Shapes are the smallest that hit each edge; n = 3 * H * W draws per view, 624 draws per MT19937 twist, 16 per Box-Muller
chunk, and a Gaussian view whose n is no multiple of 16 consumes 16 more draws for its tail.
"""
import ctypes as C

import numpy as np
import pytest
import torch

try:
    from PIL import Image, ImageEnhance
except Exception:  # pragma: no cover
    Image = None

needs_pillow = pytest.mark.skipif(Image is None, reason="Pillow not importable")

# ------------------------------------------------------------------ cases
NOISE_SHAPES = [
    (4, 4),      # n = 48: exactly three chunks, no tail
    (1, 6),      # n = 18: one chunk, 2 over (the smallest accepted Gaussian size)
    (7, 7),      # n = 147: rem 3
    (13, 16),    # n = 624: exactly one twist, no tail
    (1, 203),    # n = 609: the tail starts exactly at the next twist's first chunk start (624 - 15)
    (9, 23),     # n = 621: the tail straddles twists 0 and 1
    (1, 208),    # n = 624, flat image
    (17, 19),    # n = 969
    (26, 16),    # n = 1248: two twists
    (31, 33),    # n = 3069
]
SEEDS = [0, 5, 2 ** 33 + 7]
G = lambda std: (0, float(std))
SP = lambda prob: (1, float(prob))
SEG_LISTS = {
    "g16_sp": [G(16), SP(0.1)],
    "sp_g8": [SP(0.0), G(8)],
    "g8_g16_sp_g4": [G(8), G(16), SP(1.0), G(4)],
    "sp_sp_g16": [SP(2.0), SP(0.1), G(16)],
    "full16": [G(8 * (i // 2 + 1)) if i % 2 == 0 else SP((0.05, 0.1, 0.2, 0.3, 1.0, 0.0, 2.0, 0.15)[i // 2]) for i in range(16)],
}
SP_PROBS = [0.0, 0.1, 1.0, 2.0]
GAUSS_ATOL_STD16 = 2e-6

RESIZE_CASES = [   # (H, W, oh, ow)
    (1, 1, 1, 1), (1, 7, 1, 3), (7, 1, 3, 1), (2, 2, 5, 5), (3, 5, 1, 1), (61, 47, 1, 1),
    (61, 47, 61, 20),      # horizontal pass only
    (61, 47, 20, 47),      # vertical pass only
    (17, 19, 17, 19),      # copy branch
    (5, 300, 5, 7), (300, 5, 7, 5),      # a window of about 86 taps
    (33, 65, 99, 130),     # upscale
    (64, 64, 3, 200),      # down in one axis, up in the other
]
RESIZE_RATIOS = [0.7, 0.8, 0.9, 1.2]      # on 40 x 52 through cald_helper.resize's int(W * ratio) rule

ROTATE_SIZES = [(1, 1), (2, 3), (17, 19), (5, 60), (60, 5), (40, 52)]
ROTATE_ANGLES = [5, -5, 3.3, -17, 45, 0, 180, 90, 270]

COLOR_SIZES = [(1, 1), (2, 3), (17, 19), (513, 512)]      # 513 x 512: the smallest size above the 1024 x 256 grid cap
COLOR_FACTORS = [0.0, 0.5, 0.999, 1.0, 1.001, 1.5, 2, 3, 7.5]


def _image(H, W, seed, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, (H, W, 3)).astype(np.uint8)


# ------------------------------------------------------------------ the live calls of the reference
def _live_stream(seed, H, W, segs):
    """torch.manual_seed(seed), then GaussianNoise's `torch.randn(size) * std / 255.0` (cald_helper.py:74) resp. SaltPepperNoise's
    `torch.rand(size)` (:80) per segment, in order.  The global generator is restored afterwards."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return [(torch.randn(3, H, W) * p / 255.0 if k == 0 else torch.rand(3, H, W)).numpy() for k, p in segs]


def _live_salt_pepper(img, prob, noise):
    """cald_helper.SaltPepperNoise (:78-85) on to_tensor(img) given its torch.rand draws; back to uint8 (every value is some k / 255)."""
    image = torch.from_numpy(img).permute(2, 0, 1).float().div(255)
    noise = torch.from_numpy(np.array(noise))      # a copy: the shared reference arrays are read-only
    salt = torch.max(image)
    pepper = torch.min(image)
    image[noise < prob / 2] = salt
    image[noise > 1 - prob / 2] = pepper
    return (image * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()


_REF = {}


def _stream_reference(oracle, H, W, seed, name):
    """(live torch outputs, oracle outputs) of one segment list, computed once per case and shared by the CPU and GPU halves."""
    key = (H, W, seed, name)
    if key not in _REF:
        segs = SEG_LISTS[name]
        live = _live_stream(seed, H, W, segs)
        orc = oracle.torch_stream(seed, 3 * H * W, segs).reshape(len(segs), 3, H, W)
        for a in live:
            a.setflags(write=False)
        orc.setflags(write=False)
        _REF[key] = (live, orc)
    return _REF[key]


def _noise_image(H, W):
    return _image(H, W, 1000 * H + W, 3, 251)      # max and min are the image's own, not 255 and 0


def _live_rotate(img, angle):
    """cald_helper.rotate's two Pillow calls (:153, :215)."""
    H, W, _ = img.shape
    return np.asarray(Image.fromarray(img).rotate(angle, expand=True).resize((W, H)))


def _live_color_adjust(img, factor):
    """cald_helper.ColorAdjust (:65-69): torchvision's adjust_brightness / _contrast / _saturation on a PIL image."""
    im = Image.fromarray(img)
    im = ImageEnhance.Brightness(im).enhance(factor)
    im = ImageEnhance.Contrast(im).enhance(factor)
    im = ImageEnhance.Color(im).enhance(factor)
    return np.asarray(im)


def _color_images(H, W):
    rs = np.random.RandomState(7 * H + W)
    out = {
        "random": _image(H, W, 31 * H + W),
        "black": np.zeros((H, W, 3), np.uint8),
        "white": np.full((H, W, 3), 255, np.uint8),
        "saturated": (rs.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8),
    }
    if H * W > 1024 * 256:
        # gray 100 / 101 with mean luma 100.55: after brightness 1.5 (150 / 151) the mean is 150.55 and rounds to 151 only if
        # every pixel is in the sum; losing the 512 pixels past the first grid stride (0.2 % of the sum) rounds it to 150
        g = np.full(H * W, 100, np.uint8)
        g[rs.permutation(H * W)[:int(round(0.55 * H * W))]] = 101
        out["mean_on_the_rounding_edge"] = np.repeat(g.reshape(H, W, 1), 3, axis=2)
        lum = 150.0 + (g == 101)
        assert int(lum.sum() / (H * W) + 0.5) == 151 and int(lum[:1024 * 256].sum() / (H * W) + 0.5) == 150
    return out


def _boxes(H, W):
    rs = np.random.RandomState(H * 100 + W)
    x0 = rs.rand(5) * W * 0.6
    y0 = rs.rand(5) * H * 0.6
    b = np.stack([x0, y0, x0 + rs.rand(5) * W * 0.4, y0 + rs.rand(5) * H * 0.4], 1).astype(np.float32)
    return np.concatenate([b, np.array([[0, 0, W, H]], np.float32)])


# ================================================================== CPU: the oracle against live torch / Pillow
def test_oracle_uniform_draws_equal_live_torch_rand(oracle):
    for seed in SEEDS:
        for n in (1, 5, 18, 623, 624, 625, 1248, 3069):
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                want = torch.rand(n).numpy()
            np.testing.assert_array_equal(oracle.torch_rand(seed, n), want, err_msg="seed %d n %d" % (seed, n))


@pytest.mark.parametrize("shape", NOISE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_stream_equals_live_torch(oracle, shape):
    H, W = shape
    img = _noise_image(H, W)
    for seed in SEEDS:
        for name, segs in SEG_LISTS.items():
            live, orc = _stream_reference(oracle, H, W, seed, name)
            for g, (k, p) in enumerate(segs):
                tag = "seed %d list %s segment %d" % (seed, name, g)
                if k == 1:
                    np.testing.assert_array_equal(orc[g], live[g], err_msg=tag)
                    np.testing.assert_array_equal(oracle.salt_pepper_from_uniforms(img, p, orc[g]), _live_salt_pepper(img, p, live[g]), err_msg=tag)
                else:
                    err = float(np.abs(orc[g].astype(np.float64) - live[g]).max())
                    assert err <= GAUSS_ATOL_STD16 * p / 16, (tag, err)


@pytest.mark.parametrize("shape", NOISE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_single_view_helpers_equal_live_torch(oracle, shape):
    """oracle.gaussian_noise / oracle.salt_pepper (one view from a fresh generator), every probability, and a constant image."""
    H, W = shape
    img = _noise_image(H, W)
    flat = np.full((H, W, 3), 77, np.uint8)
    for seed in SEEDS:
        (ga,) = _live_stream(seed, H, W, [G(16)])
        assert float(np.abs(oracle.gaussian_noise(seed, H, W, 16).astype(np.float64) - ga).max()) <= GAUSS_ATOL_STD16, seed
        (u,) = _live_stream(seed, H, W, [SP(0)])
        for prob in SP_PROBS:
            np.testing.assert_array_equal(oracle.salt_pepper(img, prob, seed), _live_salt_pepper(img, prob, u), err_msg="seed %d prob %g" % (seed, prob))
            np.testing.assert_array_equal(oracle.salt_pepper(flat, prob, seed), flat)
            np.testing.assert_array_equal(_live_salt_pepper(flat, prob, u), flat)


def test_oracle_refuses_gaussian_noise_on_fewer_than_16_elements(oracle):
    """torch.randn takes its scalar path below 16 elements; the oracle raises instead of returning unwritten memory."""
    for H, W in ((1, 1), (1, 5)):
        with pytest.raises(NotImplementedError):
            oracle.gaussian_noise(3, H, W, 16)
        with pytest.raises(NotImplementedError):
            oracle.torch_stream(3, 3 * H * W, [SP(0.1), G(16)])
        with pytest.raises(NotImplementedError):
            oracle.gaussian_noise_seq(3, H, W, [8, 16])
        # uniform draws have no such limit
        (u,) = _live_stream(3, H, W, [SP(0.1)])
        np.testing.assert_array_equal(oracle.torch_stream(3, 3 * H * W, [SP(0.1)]).reshape(3, H, W), u)
        img = _noise_image(H, W)
        np.testing.assert_array_equal(oracle.salt_pepper(img, 1.0, 3), _live_salt_pepper(img, 1.0, u))
    (ga,) = _live_stream(3, 1, 6, [G(16)])      # the first accepted size
    assert float(np.abs(oracle.gaussian_noise(3, 1, 6, 16).astype(np.float64) - ga).max()) <= GAUSS_ATOL_STD16


@needs_pillow
def test_oracle_resize_equals_live_pillow(oracle):
    cases = RESIZE_CASES + [(40, 52, int(40 * r), int(52 * r)) for r in RESIZE_RATIOS]
    for H, W, oh, ow in cases:
        img = _image(H, W, H * 1000 + W)
        pil = Image.fromarray(img)
        np.testing.assert_array_equal(oracle.pil_resize_bilinear(img, oh, ow), np.asarray(pil.resize((ow, oh), Image.BILINEAR)), err_msg=str((H, W, oh, ow)))
        np.testing.assert_array_equal(oracle.pil_resize_bicubic(img, oh, ow), np.asarray(pil.resize((ow, oh), Image.BICUBIC)), err_msg=str((H, W, oh, ow)))


@needs_pillow
@pytest.mark.parametrize("size", ROTATE_SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_rotate_equals_live_pillow(oracle, size):
    H, W = size
    img = _image(H, W, H * 1000 + W)
    for angle in ROTATE_ANGLES:
        exp = np.asarray(Image.fromarray(img).rotate(angle, expand=True))
        np.testing.assert_array_equal(oracle.pil_rotate_expand(img, angle), exp, err_msg="angle %g (expanded)" % angle)
        np.testing.assert_array_equal(oracle.rotate_aug(img, _boxes(H, W), angle)[0], _live_rotate(img, angle), err_msg="angle %g" % angle)
    np.testing.assert_array_equal(oracle.pil_rotate_expand(img, 450), np.asarray(Image.fromarray(img).rotate(450, expand=True)))
    np.testing.assert_array_equal(oracle.pil_rotate_expand(img, -90), np.asarray(Image.fromarray(img).rotate(-90, expand=True)))


@needs_pillow
@pytest.mark.parametrize("size", COLOR_SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_color_adjust_equals_live_pillow(oracle, size):
    H, W = size
    for name, img in _color_images(H, W).items():
        for f in COLOR_FACTORS:
            np.testing.assert_array_equal(oracle.color_adjust(img, f), _live_color_adjust(img, f), err_msg="%s factor %g" % (name, f))


# ================================================================== GPU: the kernels against the oracle and the live calls
@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run with -m gpu on a GPU box); no CPU fallback exists for the product path")
    from cald_amd import _ffi, cald_helper, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), ch=cald_helper)


GUARD = 256      # bytes of 0xA5 before, between and after the views of one launch: a stray store shows


def _gpu_noise_stream(hip, img, seed, segs):
    """One cald_op_noise_stream launch; the views lie in one arena separated by guard bytes.  Gaussian views are pre-filled with NaN
    and salt-and-pepper views with 0xA5, so an element the kernel does not write shows as well."""
    ffi, L = hip["ffi"], hip["L"]
    H, W, _ = img.shape
    n = 3 * H * W
    sizes = [n * 4 if k == 0 else n for k, _ in segs]
    offs, at = [], GUARD
    for s in sizes:
        offs.append(at)
        at += (s + 255) // 256 * 256 + GUARD
    host = np.full(at, 0xA5, np.uint8)
    for (k, _), o in zip(segs, offs):
        if k == 0:
            host[o:o + n * 4].view(np.float32)[:] = np.nan
    arena = torch.from_numpy(host).cuda()
    src = torch.from_numpy(img).cuda()
    kinds = np.array([ffi.AUG_GAUSS if k == 0 else ffi.AUG_SALT_PEPPER for k, _ in segs], np.int32)
    params = np.array([p for _, p in segs], np.float64)
    dsts = (C.c_void_p * len(segs))(*[arena.data_ptr() + o for o in offs])
    ffi.check(L.cald_op_noise_stream(hip["ctx"], seed, src.data_ptr(), H, W, len(segs), ffi.ptr(kinds, ffi.c_i), ffi.ptr(params, ffi.c_d), dsts))
    back = arena.cpu().numpy()
    keep = np.ones(at, bool)
    out = []
    for (k, _), o, s in zip(segs, offs, sizes):
        keep[o:o + s] = False
        out.append(back[o:o + s].view(np.float32).reshape(3, H, W).copy() if k == 0 else back[o:o + s].reshape(H, W, 3).copy())
    assert np.all(back[keep] == 0xA5), "noise_stream_kernel wrote outside its views"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", NOISE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_noise_stream_kernel_equals_oracle_and_live_torch(hip, oracle, shape):
    H, W = shape
    img = _noise_image(H, W)
    for seed in SEEDS:
        for name, segs in SEG_LISTS.items():
            live, orc = _stream_reference(oracle, H, W, seed, name)
            got = _gpu_noise_stream(hip, img, seed, segs)
            for g, (k, p) in enumerate(segs):
                tag = "seed %d list %s segment %d" % (seed, name, g)
                if k == 1:
                    np.testing.assert_array_equal(got[g], oracle.salt_pepper_from_uniforms(img, p, orc[g]), err_msg=tag)
                    np.testing.assert_array_equal(got[g], _live_salt_pepper(img, p, live[g]), err_msg=tag)
                else:
                    assert got[g].tobytes() == orc[g].tobytes(), (tag, float(np.abs(got[g] - orc[g]).max()))
                    err = float(np.abs(got[g].astype(np.float64) - live[g]).max())
                    assert err <= GAUSS_ATOL_STD16 * p / 16, (tag, err)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", NOISE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_noise_helpers_equal_live_torch(hip, oracle, shape):
    """cald_helper.GaussianNoise / SaltPepperNoise (cald_op_augment, one view): every probability, and a constant image."""
    H, W = shape
    ch = hip["ch"]
    img = _noise_image(H, W)
    flat = np.full((H, W, 3), 77, np.uint8)
    u8 = lambda t: (t * 255).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    for seed in SEEDS:
        (ga,) = _live_stream(seed, H, W, [G(16)])
        noise = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
        ch._augment(hip["ffi"].AUG_GAUSS, 16, seed, torch.from_numpy(img).cuda(), noise)
        got = noise.cpu().numpy()
        assert got.tobytes() == oracle.gaussian_noise(seed, H, W, 16).tobytes(), seed
        assert float(np.abs(got.astype(np.float64) - ga).max()) <= GAUSS_ATOL_STD16, seed
        seen = ch.GaussianNoise(torch.from_numpy(img), 16, seed=seed).cpu().numpy().astype(np.float64)      # image / 255 + noise, in float32
        assert float(np.abs(seen - (img.transpose(2, 0, 1) / 255.0 + got)).max()) <= 2.0 ** -22, seed
        (u,) = _live_stream(seed, H, W, [SP(0)])
        for prob in SP_PROBS:
            np.testing.assert_array_equal(u8(ch.SaltPepperNoise(torch.from_numpy(img), prob, seed=seed)), _live_salt_pepper(img, prob, u), err_msg="seed %d prob %g" % (seed, prob))
            np.testing.assert_array_equal(u8(ch.SaltPepperNoise(torch.from_numpy(flat), prob, seed=seed)), flat)


@pytest.mark.gpu
def test_gaussian_noise_on_fewer_than_16_elements_is_refused(hip, oracle):
    ch, ffi = hip["ch"], hip["ffi"]
    for H, W in ((1, 1), (1, 5)):
        img = _noise_image(H, W)
        src = torch.from_numpy(img).cuda()
        dst = torch.full((3, H, W), 123.0, dtype=torch.float32, device="cuda")
        with pytest.raises(NotImplementedError, match="scalar path"):
            ch._augment(ffi.AUG_GAUSS, 16, 3, src, dst)
        assert bool((dst == 123.0).all())
        with pytest.raises(NotImplementedError, match="scalar path"):
            ch.GaussianNoise(torch.from_numpy(img), 16, seed=3)
        with pytest.raises(NotImplementedError, match="scalar path"):
            _gpu_noise_stream(hip, img, 3, [SP(0.1), G(16)])
        # salt and pepper draws uniforms only: no such limit
        (u,) = _live_stream(3, H, W, [SP(1.0)])
        (sp,) = _gpu_noise_stream(hip, img, 3, [SP(1.0)])
        np.testing.assert_array_equal(sp, _live_salt_pepper(img, 1.0, u))
    img = _noise_image(1, 6)      # the first accepted size
    (ga,) = _live_stream(3, 1, 6, [G(16)])
    (got,) = _gpu_noise_stream(hip, img, 3, [G(16)])
    assert got.tobytes() == oracle.gaussian_noise(3, 1, 6, 16).tobytes()
    assert float(np.abs(got.astype(np.float64) - ga).max()) <= GAUSS_ATOL_STD16


@pytest.mark.gpu
def test_noise_stream_hook_rejects_bad_segment_lists(hip):
    img = _noise_image(4, 4)
    with pytest.raises(RuntimeError):
        _gpu_noise_stream(hip, img, 0, [G(8)] * (hip["ffi"].MAX_NOISE_SEG + 1))
    with pytest.raises(RuntimeError):
        _gpu_noise_stream(hip, img, 0, [])


@needs_pillow
@pytest.mark.gpu
def test_pil_resize_kernels_equal_live_pillow(hip, oracle):
    """Every branch of pil_resize: both passes, one pass only, the copy; 1-pixel dimensions; an 86-tap window.  Each case runs twice on
    different pixels, so the second run is served by the context's coefficient cache."""
    ffi, L = hip["ffi"], hip["L"]
    for H, W, oh, ow in RESIZE_CASES:
        for rep in range(2):
            img = _image(H, W, H * 1000 + W + rep)
            src = torch.from_numpy(img).cuda()
            dst = torch.full((oh, ow, 3), 0xA5, dtype=torch.uint8, device="cuda")
            ffi.check(L.cald_op_pil_resize(hip["ctx"], src.data_ptr(), H, W, dst.data_ptr(), oh, ow))
            want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
            np.testing.assert_array_equal(dst.cpu().numpy(), want, err_msg=str((H, W, oh, ow, rep)))
            np.testing.assert_array_equal(want, oracle.pil_resize_bilinear(img, oh, ow))


@needs_pillow
@pytest.mark.gpu
def test_resize_helper_equals_live_pillow_at_every_ratio(hip):
    ch = hip["ch"]
    H, W = 40, 52
    img = _image(H, W, 4052)
    boxes = torch.from_numpy(_boxes(H, W))
    for r in RESIZE_RATIOS:
        ri, rb = ch.resize(torch.from_numpy(img), boxes, r)
        want = np.asarray(Image.fromarray(img).resize((int(W * r), int(H * r)), Image.BILINEAR))
        np.testing.assert_array_equal((ri * 255).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy(), want, err_msg=str(r))
        np.testing.assert_array_equal(rb.numpy(), (boxes * r).numpy())


@needs_pillow
@pytest.mark.gpu
@pytest.mark.parametrize("size", ROTATE_SIZES, ids=lambda s: "%dx%d" % s)
def test_rotate_helper_equals_live_pillow(hip, oracle, size):
    ch = hip["ch"]
    H, W = size
    img = _image(H, W, H * 1000 + W)
    boxes = _boxes(H, W)
    for angle in ROTATE_ANGLES:
        ri, rb = ch.rotate(torch.from_numpy(img), torch.from_numpy(boxes), angle)
        got = (ri * 255).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        np.testing.assert_array_equal(got, _live_rotate(img, angle), err_msg="angle %g" % angle)
        np.testing.assert_array_equal(rb.numpy(), oracle.rotate_aug(img, boxes, angle)[1], err_msg="angle %g" % angle)


@needs_pillow
@pytest.mark.gpu
@pytest.mark.parametrize("size", COLOR_SIZES, ids=lambda s: "%dx%d" % s)
def test_color_adjust_helper_equals_live_pillow(hip, oracle, size):
    ch = hip["ch"]
    H, W = size
    for name, img in _color_images(H, W).items():
        src = torch.from_numpy(img).cuda()
        for f in COLOR_FACTORS:
            got = (ch.ColorAdjust(src, f) * 255).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
            np.testing.assert_array_equal(got, _live_color_adjust(img, f), err_msg="%s factor %g" % (name, f))
