"""GPU tests of the VAAL sweep (cald_sweep_vaal, cald_op_vaal_*, cald_amd.vaal): every kernel bit for bit against the CPU restatement
(tests/_vaal_restatement.py) and the oracle's convolution, the whole sweep against the restatement, the reference's recorded float64 values
and query indices (tests/golden/vaal.npz), batching and order invariance, and the drop-in entry."""
import ctypes as C

import numpy as np
import pytest

import _vaal_restatement as R

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run with -m gpu on a GPU box); no CPU fallback exists for the product path")
    from cald_amd import _ffi, detector, vaal
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), torch=torch, vaal=vaal)


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("vaal")
    return dict(g=g, images=[g["image%d" % i] for i in range(int(g["n_images"]))], budget=int(g["budget"]))


@pytest.fixture(scope="module")
def weights(fx):
    return R.make_weights(int(fx["g"]["seed"]))


@pytest.fixture(scope="module")
def model(hip, weights):
    m = hip["vaal"].VaalModel(weights, weights)
    yield m
    m.close()


@pytest.fixture(scope="module")
def restated(fx, weights, oracle):
    """The restatement of the whole sweep in both modes, its float64 evaluation and bound, and the stages of image 0: computed once."""
    out = {}
    wt = R.fc_weight_kprime(weights["fc_mu.weight"])
    for tag, running in (("train", False), ("eval", True)):
        mu, preds = R.sweep(oracle, weights, fx["images"], running, wt)
        _, _, mub, pb = R.sweep64(weights, fx["images"], running, oracle)
        keep = []
        R.encode(oracle, weights, fx["images"][0], running, keep)
        out[tag] = dict(mu=mu, preds=preds, mub=mub, pb=pb, keep=keep)
    out["wt"] = wt
    return out


def dev_images(hip, imgs):
    return [hip["torch"].from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]


# ----------------------------------------------------------------------------- resize
@pytest.mark.parametrize("H,W", [(1, 1), (1333, 1), (1, 1333), (2, 255), (255, 2), (256, 257), (257, 256), (333, 500), (500, 1333), (256, 256)])
def test_resize_op(hip, H, W):
    img = np.random.RandomState(H * 2048 + W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    out = np.full((256, 256, 3), np.nan, F32)
    hip["ffi"].check(hip["L"].cald_op_vaal_resize(hip["ctx"], hip["ffi"].ptr(img, hip["ffi"].c_u8), H, W, hip["ffi"].ptr(out)))
    assert np.array_equal(out, R.resize(img))


# ----------------------------------------------------------------------------- normalisation + ReLU
def bn_op(hip, x, n, HW, Cn, g, b):
    x = np.ascontiguousarray(x, F32)
    out = np.full((n, HW, Cn), np.nan, F32)
    hip["ffi"].check(hip["L"].cald_op_vaal_bn_relu(hip["ctx"], hip["ffi"].ptr(x), x.size, n, HW, Cn, hip["ffi"].ptr(g), hip["ffi"].ptr(b),
                                                   hip["ffi"].ptr(out)))
    return out


def bn_inputs(seed, n, HW, Cn):
    rs = np.random.RandomState(seed)
    x = (rs.randn(n, HW, Cn) * rs.uniform(0.5, 3.0, (n, 1, Cn)) + rs.randn(n, 1, Cn) * 2).astype(F32)
    return x, rs.uniform(0.4, 1.6, Cn).astype(F32), (rs.randn(Cn) * 0.3).astype(F32)


@pytest.mark.parametrize("HW,Cn,n", [(64, 1024, 2), (256, 512, 2), (1024, 256, 2), (4096, 128, 1), (16384, 64, 1), (1, 8, 3), (63, 4, 2), (65, 12, 2),
                                      (257, 68, 2), (255, 64, 1)])
def test_bn_relu_op(hip, HW, Cn, n):
    x, g, b = bn_inputs(HW * 7 + Cn, n, HW, Cn)
    got = bn_op(hip, x, n, HW, Cn, g, b)
    for i in range(n):
        assert np.array_equal(got[i], R.bn_relu(x[i], g, b)), i
        r = x[i].astype(np.float64)
        y64 = np.maximum((r - r.mean(axis=0)) / np.sqrt(r.var(axis=0) + R.EPS) * g + b, 0.0)
        bound = R.bn_batch_bound(x[i][None], np.zeros((1, HW, Cn)), g, b)[0]
        assert np.all(np.abs(got[i] - y64) <= bound)
    assert (got > 0).any() and (got == 0).any()


def test_bn_relu_constant_map_gives_relu_beta(hip):
    """Variance exactly 0: every centred value is 0, so y = relu(0 * istd * gamma + beta) = relu(beta) exactly.  The constants have eight
    significant bits, so every partial sum k * c (k <= 300) and the division by N are exact and the float32 mean IS the constant; for an
    arbitrary constant the float32 mean is off by a rounding in any summation order, the variance is tiny rather than 0, and what is
    pinned is equality with the restatement (second half)."""
    HW, Cn = 300, 16
    rs = np.random.RandomState(5)
    g, b = rs.uniform(0.5, 1.5, Cn).astype(F32), (rs.randn(Cn)).astype(F32)
    assert (b > 0).any() and (b < 0).any()
    cst = (rs.randint(-127, 128, Cn) / 4.0).astype(F32)
    x = np.broadcast_to(cst[None, None], (2, HW, Cn)).copy()
    got = bn_op(hip, x, 2, HW, Cn, g, b)
    assert np.array_equal(got, np.broadcast_to(np.maximum(b, 0)[None, None], got.shape))
    assert np.array_equal(got[0], R.bn_relu(x[0], g, b))
    x = np.broadcast_to((rs.randn(Cn) * 100).astype(F32)[None, None], (2, HW, Cn)).copy()
    got = bn_op(hip, x, 2, HW, Cn, g, b)
    assert np.array_equal(got[0], R.bn_relu(x[0], g, b)) and np.array_equal(got[1], got[0])


def test_bn_relu_with_one_huge_outlier(hip):
    HW, Cn = 1024, 8
    x, g, b = bn_inputs(11, 1, HW, Cn)
    x[0, 517, :] = 1e6
    x[0, 3, 2] = -3e7
    got = bn_op(hip, x, 1, HW, Cn, g, b)
    assert np.array_equal(got[0], R.bn_relu(x[0], g, b))
    r = x[0].astype(np.float64)
    y64 = np.maximum((r - r.mean(axis=0)) / np.sqrt(r.var(axis=0) + R.EPS) * g + b, 0.0)
    assert np.all(np.abs(got[0] - y64) <= R.bn_batch_bound(x[0][None], np.zeros((1, HW, Cn)), g, b)[0])
    assert np.isfinite(got).all()


def test_bn_relu_does_not_read_past_the_last_row(hip):
    """NaN after the last valid row of the last image (a short last chunk): one read of it would poison a sum."""
    n, HW, Cn = 2, 300, 64
    x, g, b = bn_inputs(13, n, HW, Cn)
    buf = np.concatenate([x.reshape(-1), np.full(5 * 256 * Cn, np.nan, F32)])
    got = bn_op(hip, buf, n, HW, Cn, g, b)
    assert np.isfinite(got).all()
    for i in range(n):
        assert np.array_equal(got[i], R.bn_relu(x[i], g, b))


# ----------------------------------------------------------------------------- convolutions
def conv_op(hip, x, w, bias=None, scale=None, shift=None, relu=False):
    """cald_op_conv2d on x [H][W][Cin] with a torch-layout weight; a channel count that is no multiple of 4 is zero-padded, as the sweep
    pads the image's three channels."""
    x, w = np.ascontiguousarray(x, F32), np.ascontiguousarray(w, F32)
    Cin = x.shape[2]
    if Cin % 4:
        pad = 4 - Cin % 4
        x = np.concatenate([x, np.zeros(x.shape[:2] + (pad,), F32)], axis=2)
        w = np.concatenate([w, np.zeros((w.shape[0], pad) + w.shape[2:], F32)], axis=1)
        x, w = np.ascontiguousarray(x), np.ascontiguousarray(w)
    H, W, Cp = x.shape
    Ho, Wo = (H + 2 - 4) // 2 + 1, (W + 2 - 4) // 2 + 1
    out = np.full((Ho, Wo, w.shape[0]), np.nan, F32)
    p = hip["ffi"].ptr
    hip["ffi"].check(hip["L"].cald_op_conv2d(hip["ctx"], p(x), H, W, Cp, p(w), w.shape[0], 4, 4, 2, 1, p(bias), p(scale), p(shift), None, int(relu), p(out)))
    return out


@pytest.mark.parametrize("l", range(5))
def test_each_encoder_convolution_alone(hip, fx, weights, restated, l):
    """Layer l on image 0's own input (the restatement's previous activation) against oracle.conv2d with the same weights -- the
    restatement's convolution output is exactly that."""
    keep = restated["train"]["keep"]
    x = keep[l - 1][1] if l else R.resize(fx["images"][0])
    got = conv_op(hip, x, weights["encoder.%d.weight" % (3 * l)], weights["encoder.%d.bias" % (3 * l)])
    assert np.array_equal(got, keep[l][0])


@pytest.mark.parametrize("l", [0, 4])
def test_encoder_convolution_with_folded_statistics(hip, fx, weights, restated, l):
    keep = restated["eval"]["keep"]
    x = keep[l - 1][1] if l else R.resize(fx["images"][0])
    sc, sh = R.folded_bn(weights, l)
    got = conv_op(hip, x, weights["encoder.%d.weight" % (3 * l)], weights["encoder.%d.bias" % (3 * l)], sc, sh, relu=True)
    assert np.array_equal(got, keep[l][1])


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (8, 8)])
@pytest.mark.parametrize("Cin", [3, 64])
def test_convolution_where_padding_matters_at_every_border(hip, oracle, H, W, Cin):
    rs = np.random.RandomState(H * 100 + W * 10 + Cin)
    x = rs.randn(H, W, Cin).astype(F32)
    w = (rs.randn(64, Cin, 4, 4) / np.sqrt(16 * Cin)).astype(F32)
    b = rs.randn(64).astype(F32)
    assert np.array_equal(conv_op(hip, x, w, b), oracle.conv2d(x, R.kmajor(w), 4, 4, 2, 1, bias=b))


# ----------------------------------------------------------------------------- fc_mu and the head
def test_fc_mu_op(hip, model, weights, restated):
    """1, 2 and 5 rows, and 17: the second tile of 16 images.  Rows are independent, so the restatement runs on five of the 17 only."""
    rs = np.random.RandomState(3)
    act = np.maximum(rs.randn(17, 65536), 0).astype(F32)
    rows = [0, 1, 4, 15, 16]
    want = dict(zip(rows, R.fc_mu(act[rows], restated["wt"], weights["fc_mu.bias"])))
    for n in (1, 2, 5, 17):
        got = np.full((n, 256), np.nan, F32)
        hip["ffi"].check(hip["L"].cald_op_vaal_fc_mu(model.h, n, hip["ffi"].ptr(np.ascontiguousarray(act[:n])), hip["ffi"].ptr(got)))
        assert np.isfinite(got).all()
        for r in rows:
            if r < n:
                assert np.array_equal(got[r], want[r]), (n, r)


def head_op(hip, model, mu):
    mu = np.ascontiguousarray(mu, F32)
    out = np.full(mu.shape[0], np.nan, F32)
    hip["ffi"].check(hip["L"].cald_op_vaal_head(model.h, mu.shape[0], hip["ffi"].ptr(mu), hip["ffi"].ptr(out)))
    return out


@pytest.mark.parametrize("n", [1, 7])
def test_head_op(hip, model, weights, n):
    mu = (np.random.RandomState(n).randn(n, 256) * 3).astype(F32)
    got = head_op(hip, model, mu)
    assert np.array_equal(got, R.head(weights, mu))
    assert np.all((got > 0) & (got < 1))


def test_head_saturates_without_nan(hip, model, weights):
    """Pre-sigmoid values beyond +-100: exp overflows to inf or underflows to 0, the prediction is exactly 0 or 1, never NaN."""
    mu = (np.random.RandomState(0).randn(16, 256) * 400).astype(F32)
    z = R.head_logit(weights, mu)
    assert (z > 100).any() and (z < -100).any()
    got = head_op(hip, model, mu)
    assert np.array_equal(got, R.head(weights, mu)) and np.isfinite(got).all()
    assert np.all(got[z > 100] == 1.0) and np.all(got[z < -100] == 0.0)


# ----------------------------------------------------------------------------- the whole sweep
@pytest.fixture(scope="module")
def swept(hip, model, fx):
    dev = dev_images(hip, fx["images"])
    return {tag: hip["vaal"].vaal_sweep_device_images(model, None, dev, return_mu=True, bn_running=running)
            for tag, running in (("train", False), ("eval", True))}


@pytest.mark.parametrize("tag", ["train", "eval"])
def test_sweep_equals_the_restatement_and_the_reference(tag, swept, restated, fx, hip):
    preds, mu = swept[tag]
    r, g = restated[tag], fx["g"]
    assert np.array_equal(mu, r["mu"])
    assert np.array_equal(preds, r["preds"])
    assert np.all(np.abs(mu.astype(np.float64) - g["mu64_" + tag]) <= r["mub"])
    assert np.all(np.abs(preds.astype(np.float64) - g["preds64_" + tag]) <= r["pb"])
    for name, mine, ref32, ref64 in (("mu", mu, g["mu_" + tag], g["mu64_" + tag]), ("preds", preds, g["preds_" + tag], g["preds64_" + tag])):
        scale = np.abs(ref64).max()
        d_mine, d_ref = np.abs(mine - ref64).max() / scale, np.abs(ref32 - ref64).max() / scale
        print("%s %s: sweep %.3g, reference float32 %.3g of max|%s|" % (tag, name, d_mine, d_ref, name))
        assert d_mine <= 4.0 * d_ref            # tests/test_vaal_sweep.py MARGIN
    assert np.array_equal(hip["vaal"].select_lowest(preds, fx["budget"]), g["idx_" + tag])


@pytest.mark.parametrize("tag,running", [("train", False), ("eval", True)])
def test_sweep_does_not_depend_on_batching_or_order(tag, running, swept, hip, model, fx):
    dev = dev_images(hip, fx["images"])
    preds, mu = swept[tag]
    for b in (1, 3):
        p2, m2 = hip["vaal"].vaal_sweep_device_images(model, None, dev, batch_images=b, return_mu=True, bn_running=running)
        assert np.array_equal(p2, preds) and np.array_equal(m2, mu), b
    p3, m3 = hip["vaal"].vaal_sweep_device_images(model, None, dev[::-1], batch_images=3, return_mu=True, bn_running=running)
    assert np.array_equal(p3[::-1], preds) and np.array_equal(m3[::-1], mu)
    p4, m4 = hip["vaal"].vaal_sweep_device_images(model, None, dev, return_mu=True, bn_running=running)
    assert np.array_equal(p4, preds) and np.array_equal(m4, mu)


def test_drop_in_entry(hip, weights, fx, swept):
    """sample_for_labeling through list loaders of PIL images and of float CHW tensors in [0, 1]; dict weights mean train mode."""
    from PIL import Image
    torch, vaal = hip["torch"], hip["vaal"]
    want = vaal.select_lowest(swept["train"][0], fx["budget"])
    assert np.array_equal(want, fx["g"]["idx_train"])
    pil = [([Image.fromarray(im)], None) for im in fx["images"]]
    chw = [([torch.from_numpy(im).permute(2, 0, 1).float().div(255)], None) for im in fx["images"]]
    idx, preds = vaal.sample_for_labeling(weights, weights, pil, fx["budget"], return_preds=True)
    assert isinstance(idx, np.ndarray) and np.array_equal(idx, want) and np.array_equal(preds, swept["train"][0])
    assert np.array_equal(vaal.sample_for_labeling(weights, weights, chw, fx["budget"]), want)
    assert np.array_equal(vaal.AdversarySampler(fx["budget"]).sample(weights, weights, chw), want)
    assert np.array_equal(np.sort(vaal.sample_for_labeling(weights, weights, chw[:3], 10)), np.arange(3))
    with pytest.raises(ValueError):
        vaal.sample_for_labeling(weights, weights, [(chw[0][0] * 2, None)], 1)


def test_eval_mode_is_taken_from_the_module(hip, weights, fx, swept):
    torch, vaal = hip["torch"], hip["vaal"]
    vae, disc = vaal.VAE(), vaal.Discriminator()
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items() if not k.startswith("net.")}, strict=False)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items() if k.startswith("net.")})
    dev = dev_images(hip, fx["images"][:3])
    vae.eval()
    assert np.array_equal(vaal.vaal_sweep_device_images(vae, disc, dev), swept["eval"][0][:3])
    vae.train()
    assert np.array_equal(vaal.vaal_sweep_device_images(vae, disc, dev), swept["train"][0][:3])


def test_library_rejects_missing_and_misshaped_tensors(hip, weights):
    L, ffi = hip["L"], hip["ffi"]

    def finalize(sd):
        h = C.c_void_p()
        ffi.check(L.cald_vaal_create(hip["ctx"], C.byref(h)))
        try:
            for k, a in sd.items():
                a = np.ascontiguousarray(a, F32)
                assert L.cald_vaal_load_tensor(h, k.encode(), ffi.ptr(a), (C.c_int64 * a.ndim)(*a.shape), a.ndim) == 0
            return L.cald_vaal_finalize(h)
        finally:
            L.cald_vaal_destroy(h)

    small = {k: v for k, v in weights.items() if k != "fc_mu.weight"}          # fails before the large tensor matters
    assert finalize(small) == -4 and b"fc_mu.weight" in L.cald_last_error()
    assert finalize({k: v for k, v in weights.items() if k not in ("encoder.7.running_mean", "fc_mu.weight")}) == -4
    bad = dict(small); bad["encoder.3.weight"] = np.zeros((128, 64, 3, 3), F32)
    assert finalize(bad) == -1 and b"encoder.3.weight" in L.cald_last_error()
    extra = dict(small); extra["decoder.0.weight"] = np.zeros((7, 3), F32); extra["fc_logvar.bias"] = np.zeros(256, F32)
    assert finalize(extra) == -4 and b"fc_mu.weight" in L.cald_last_error()      # the decoder keys were accepted and ignored
