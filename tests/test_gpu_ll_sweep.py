"""GPU tests of the learning-loss sweep (cald_sweep_ll, cald_op_gap, cald_op_lossnet; cald_amd.baselines.ll_get_uncertainty): pooled vectors
and scores bit for bit against the CPU restatement (tests/_ll_restatement.py) applied to the oracle's backbone, the reference's recorded
scores (tests/golden/lossnet.npz), the group padding, batching invariance, and the detector left as it was."""
import ctypes as C

import numpy as np
import pytest

import _ll_restatement as R

pytestmark = pytest.mark.gpu

MIN_SIZE, MAX_SIZE = 300, 500
POOL_IDX = [0, 1, 7, 8, 3]            # of synth.make_pool(12, "voc", 0, scale=0.5): landscape, portrait, wide, tall, landscape
BATCHES = [2, 2, 1]


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run with -m gpu on a GPU box); no CPU fallback exists for the product path")
    from cald_amd import _ffi, baselines, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch, bl=baselines)


@pytest.fixture(scope="module")
def lossnet_sd(golden):
    g = golden("lossnet")
    return {k[3:]: g[k] for k in g.files if k.startswith("sd_")}


@pytest.fixture(scope="module")
def images():
    from cald_amd import synth
    pool = synth.make_pool(12, "voc", 0, scale=0.5)
    return [pool[i] for i in POOL_IDX]


@pytest.fixture(scope="module")
def small_model(hip, oracle):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    model = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=MIN_SIZE, max_size=MAX_SIZE)
    model.to("cuda").load_state_dict(sd)
    model.eval()
    return model, oracle.prepare_frcnn(sd, 21, 50)


@pytest.fixture(scope="module")
def small_retina(hip, oracle):
    from cald_amd import synth
    sd = synth.pseudo_trained_retinanet(21, 50, seed=0)
    model = hip["det"].retinanet_resnet50_fpn_cal(num_classes=21, min_size=MIN_SIZE, max_size=MAX_SIZE)
    model.to("cuda").load_state_dict(sd)
    model.eval()
    return model, oracle.prepare_retinanet(sd, 21, 50)


@pytest.fixture(scope="module")
def small_model_f16x3(hip, oracle):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    model = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=MIN_SIZE, max_size=MAX_SIZE, precision="f16x3")
    model.to("cuda").load_state_dict(sd)
    model.eval()
    P = oracle.prepare_frcnn(sd, 21, 50)
    P["precision"] = "f16x3"
    return model, P


def groups_of(batches):
    return [b for b, n in enumerate(batches) for _ in range(n)]


def loader_of(torch, imgs, batches):
    out, at = [], 0
    for n in batches:
        out.append(([torch.from_numpy(im).cuda() for im in imgs[at:at + n]], [None] * n))
        at += n
    return out


def padded_inputs(oracle, hip, imgs, batches):
    """oracle.preprocess_view's output of every image, zero-padded to its loader batch's common size (ll_group_padding)."""
    pads = hip["bl"].ll_group_padding([im.shape[:2] for im in imgs], groups_of(batches), MIN_SIZE, MAX_SIZE)
    xs = []
    for im, (Hq, Wq) in zip(imgs, pads):
        x, (Hr, Wr, Hp, Wp) = oracle.preprocess_view(im, MIN_SIZE, MAX_SIZE)
        xp = np.zeros((Hq, Wq, 4), np.float32)
        xp[:Hp, :Wp] = x
        xs.append(xp)
    return xs, pads


def sweep(hip, model, sd, imgs, batches, **kw):
    torch = hip["torch"]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    out, pooled = hip["bl"].ll_sweep_device_images(model, sd, dev, groups_of(batches), return_pooled=True, **kw)
    return out.astype(np.float32), pooled


@pytest.fixture(scope="module")
def frcnn_reference(hip, oracle, small_model, images):
    """The oracle's P2..P5 of the five images padded as loader batches [2, 2, 1]: computed once, read by several tests."""
    _, P = small_model
    xs, pads = padded_inputs(oracle, hip, images, BATCHES)
    feats = [oracle.frcnn_backbone(P, x)[:4] for x in xs]
    return dict(xs=xs, pads=pads, feats=[[f[l] for f in feats] for l in range(4)])


# ---------------------------------------------------------------- 1. pooling operator
PIXELS = [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1027]


def op_gap(hip, x):
    ffi, L = hip["ffi"], hip["L"]
    x = np.ascontiguousarray(x, np.float32)
    out = np.full(256, np.nan, np.float32)
    ffi.check(L.cald_op_gap(hip["ctx"], ffi.ptr(x), x.shape[0], x.shape[1], x.shape[2], ffi.ptr(out)))
    return out


@pytest.mark.parametrize("n", PIXELS)
def test_gap_operator_is_the_stated_order(hip, n):
    rs = np.random.RandomState(n)
    for shape in ((1, n), (n, 1)):
        x = (rs.randn(*shape, 256) + 0.7).astype(np.float32)
        got = op_gap(hip, x)
        assert got.tobytes() == R.gap(x).tobytes(), "max abs diff %g" % float(np.abs(got - R.gap(x)).max())
        err, bound = np.abs(got.astype(np.float64) - R.gap64(x)), R.gap_bound(x)
        print(n, shape, "err/bound", float((err / bound).max()))
        assert np.all(err <= bound)
        # integers in {-2..2}, another pattern for every pixel and channel: every order gives the exact sum, a dropped or doubled pixel does not
        p, c = np.meshgrid(np.arange(n), np.arange(256), indexing="ij")
        xi = (((p * 7 + c * 3 + (p * c) % 5 + (p // 4) * 11) % 5) - 2).astype(np.float32).reshape(*shape, 256)
        want = (xi.reshape(-1, 256).sum(axis=0, dtype=np.float64).astype(np.float32) / np.float32(n)).astype(np.float32)
        assert op_gap(hip, xi).tobytes() == want.tobytes()


def test_gap_operator_rejects_other_channel_counts(hip):
    ffi, L = hip["ffi"], hip["L"]
    x = np.zeros((2, 2, 128), np.float32); out = np.zeros(256, np.float32)
    assert L.cald_op_gap(hip["ctx"], ffi.ptr(x), 2, 2, 128, ffi.ptr(out)) != 0


# ---------------------------------------------------------------- 2. LossNet operator
def test_lossnet_operator_on_the_reference_fixture(hip, golden, lossnet_sd):
    g = golden("lossnet")
    feats = [[np.ascontiguousarray(g["feat%d" % l][i].transpose(1, 2, 0)) for i in range(g["feat0"].shape[0])] for l in range(4)]
    for model, levels in (("faster_rcnn", (0, 1, 2, 3)), ("retina", (0, 0, 0, 0))):
        want, pooled = R.score_features(lossnet_sd, feats, levels)
        got = hip["bl"].lossnet_scores(lossnet_sd, pooled, hip["ctx"])
        assert got.tobytes() == want.tobytes(), (model, got, want)
        _, bound = R.score_features64(lossnet_sd, feats, levels)
        err = np.abs(got.astype(np.float64) - g["out_" + model])
        print(model, "err/bound vs the reference", err / bound)
        assert np.all(err <= bound)


@pytest.mark.parametrize("D", [1, 100])
def test_lossnet_operator_other_interm_dims(hip, D):
    rs = np.random.RandomState(D)
    sd = {}
    for j in range(1, 5):
        sd["FC%d.weight" % j] = (rs.randn(D, 256) / 16).astype(np.float32)
        sd["FC%d.bias" % j] = (rs.randn(D) * 0.2).astype(np.float32)
    sd["linear.weight"] = (rs.randn(1, 4 * D) / np.sqrt(4 * D)).astype(np.float32)
    sd["linear.bias"] = np.array([0.3], np.float32)
    pooled = (rs.randn(5, 4, 256) * 0.5 + 0.2).astype(np.float32)
    got = hip["bl"].lossnet_scores(sd, pooled, hip["ctx"])
    assert got.tobytes() == R.lossnet(sd, pooled).tobytes()


# ---------------------------------------------------------------- 3. end to end, Faster R-CNN
def test_inputs_are_padded_in_both_dimensions(oracle, hip, images):
    """A condition on the inputs: in loader batches [2, 2, 1] one image grows in H and one in W."""
    pads = hip["bl"].ll_group_padding([im.shape[:2] for im in images], groups_of(BATCHES), MIN_SIZE, MAX_SIZE)
    own = [oracle.transform_size(im.shape[0], im.shape[1], MIN_SIZE, MAX_SIZE)[2:] for im in images]
    assert any(p[0] > o[0] for p, o in zip(pads, own)) and any(p[1] > o[1] for p, o in zip(pads, own))
    assert pads[4] == own[4]


def test_sweep_frcnn_matches_restatement_on_oracle_backbone(hip, oracle, small_model, lossnet_sd, images, frcnn_reference):
    model, _ = small_model
    got, pooled = sweep(hip, model, lossnet_sd, images, BATCHES)
    want, want_pooled = R.score_features(lossnet_sd, frcnn_reference["feats"], (0, 1, 2, 3))
    assert pooled.tobytes() == want_pooled.tobytes(), "pooled vectors differ: max abs %g" % float(np.abs(pooled - want_pooled).max())
    assert got.tobytes() == want.tobytes(), (got, want)
    # the drop-in: a float32 CPU tensor in loader order
    torch = hip["torch"]
    t = hip["bl"].ll_get_uncertainty(model, lossnet_sd, loader_of(torch, images, BATCHES))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device.type == "cpu" and t.numpy().tobytes() == want.tobytes()
    # the input of a padded view: the view's own pixels, zeros beyond them
    sweep(hip, model, lossnet_sd, images[:2], [2])
    for v in range(2):
        x = model.debug_tensor("input", v)
        assert x.shape == frcnn_reference["xs"][v].shape and x.tobytes() == frcnn_reference["xs"][v].tobytes()


# ---------------------------------------------------------------- 4. batching and grouping
def test_batching_is_invisible_and_grouping_is_not(hip, small_model, lossnet_sd, images):
    torch = hip["torch"]
    model, _ = small_model
    a, pa = sweep(hip, model, lossnet_sd, images, BATCHES)
    b, pb = sweep(hip, model, lossnet_sd, images, BATCHES, batch_views=2)
    c, pc = sweep(hip, model, lossnet_sd, images, BATCHES, batch_views=3)      # loader batches straddle launch batches
    assert a.tobytes() == b.tobytes() == c.tobytes() and pa.tobytes() == pb.tobytes() == pc.tobytes()
    s, ps = sweep(hip, model, lossnet_sd, images, [1, 1, 1, 1, 1])
    assert (s != a).any() and (ps[:4] != pa[:4]).any()          # the padding is live
    assert ps[4].tobytes() == pa[4].tobytes() and s[4].tobytes() == a[4].tobytes()      # image 4 is alone either way
    # a group of one: the pooled vectors of the batch-1 forward's own pyramid
    model.forward_views([(torch.from_numpy(images[2]).cuda(), False, None)])
    want = np.stack([R.gap(model.debug_tensor("P%d" % (l + 2), 0)) for l in range(4)])
    assert ps[2].tobytes() == want.tobytes()


def test_bad_groups_and_levels_are_refused(hip, small_model, lossnet_sd, images):
    model, _ = small_model
    torch = hip["torch"]
    dev = [torch.from_numpy(im).cuda() for im in images[:3]]
    with pytest.raises(RuntimeError):
        hip["bl"].ll_sweep_device_images(model, lossnet_sd, dev, [0, 1, 0])
    with pytest.raises(RuntimeError):
        hip["bl"].ll_sweep_device_images(model, lossnet_sd, dev, [0, 0, 1], levels=(0, 1, 2, 4))      # Faster R-CNN pools P2..P5


# ---------------------------------------------------------------- 5. the detector is left intact
def test_detector_is_unchanged_by_an_ll_sweep(hip, small_model, lossnet_sd, images):
    torch = hip["torch"]
    from cald_amd import sweep as cald_sweep
    model, _ = small_model
    dev = [torch.from_numpy(im).cuda() for im in images[:3]]

    def snapshot():
        out = model.forward_views([(dev[0], False, None)])[0]
        cons, cls = cald_sweep.sweep_device_images(model, dev, [0, 1, 2], ["flip", "cut_out"], bp=1.3, base_seed=3, batch_images=2)
        return [out[k].cpu().numpy().tobytes() for k in sorted(out)] + [cons.tobytes(), cls.tobytes()]

    before = snapshot()
    sweep(hip, model, lossnet_sd, images, BATCHES)
    assert snapshot() == before


# ---------------------------------------------------------------- 6. RetinaNet
def test_sweep_retina_levels(hip, oracle, small_retina, lossnet_sd, images):
    model, P = small_retina
    imgs, batches = [images[0], images[1], images[4]], [2, 1]
    xs, _ = padded_inputs(oracle, hip, imgs, batches)
    outs = [oracle.retina_backbone(P, x) for x in xs]
    feats = [[o[l] for o in outs] for l in range(5)]
    for levels, kw in (((0, 0, 0, 0), {}), ((0, 1, 2, 3), dict(levels=(0, 1, 2, 3))), ((4, 3, 0, 0), dict(levels=(4, 3, 0, 0)))):
        got, pooled = sweep(hip, model, lossnet_sd, imgs, batches, **kw)
        want, want_pooled = R.score_features(lossnet_sd, feats, levels)
        assert pooled.tobytes() == want_pooled.tobytes(), levels
        assert got.tobytes() == want.tobytes(), levels
    with pytest.raises(RuntimeError):
        sweep(hip, model, lossnet_sd, imgs, batches, levels=(0, 1, 2, 5))


# ---------------------------------------------------------------- 7. f16x3
def test_sweep_f16x3_matches_restatement_on_oracle_backbone(hip, oracle, small_model_f16x3, lossnet_sd, images):
    model, P = small_model_f16x3
    imgs, batches = images[:2], [2]
    xs, _ = padded_inputs(oracle, hip, imgs, batches)
    outs = [oracle.frcnn_backbone(P, x)[:4] for x in xs]
    want, want_pooled = R.score_features(lossnet_sd, [[o[l] for o in outs] for l in range(4)], (0, 1, 2, 3))
    got, pooled = sweep(hip, model, lossnet_sd, imgs, batches)
    assert pooled.tobytes() == want_pooled.tobytes(), "pooled vectors differ: max abs %g" % float(np.abs(pooled - want_pooled).max())
    assert got.tobytes() == want.tobytes()


def test_sweep_retina_f16x3_pools_split_form_levels_as_hi_plus_lo(hip, lossnet_sd, images):
    """A RetinaNet in CALD_PRECISION_F16X3 keeps P3..P5 in split form only: they are pooled as the values cald_debug_tensor hands out."""
    torch = hip["torch"]
    from cald_amd import synth
    model = hip["det"].retinanet_resnet50_fpn_cal(num_classes=21, min_size=MIN_SIZE, max_size=MAX_SIZE, precision="f16x3")
    model.to("cuda").load_state_dict(synth.pseudo_trained_retinanet(21, 50, seed=0))
    model.eval()
    got, pooled = sweep(hip, model, lossnet_sd, images[3:4], [1], levels=(0, 1, 2, 3))
    model.forward_views([(torch.from_numpy(images[3]).cuda(), False, None)])
    want = np.stack([R.gap(model.debug_tensor("P%d" % (l + 3), 0)) for l in range(4)])
    assert pooled[0].tobytes() == want.tobytes()
    assert got.tobytes() == R.lossnet(lossnet_sd, want[None]).tobytes()


# ---------------------------------------------------------------- 8. a torch module as ll_model
def test_torch_module_as_ll_model(hip, small_model, lossnet_sd, images):
    torch = hip["torch"]
    model, _ = small_model

    class FourLinear(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.FC1 = torch.nn.Linear(256, 128); self.FC2 = torch.nn.Linear(256, 128)
            self.FC3 = torch.nn.Linear(256, 128); self.FC4 = torch.nn.Linear(256, 128)
            self.linear = torch.nn.Linear(512, 1)

    mod = FourLinear()
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in lossnet_sd.items()})
    loader = loader_of(torch, images[:3], [2, 1])
    a = hip["bl"].ll_get_uncertainty(model, mod, loader)
    b = hip["bl"].ll_get_uncertainty(model, mod.state_dict(), loader)
    c = hip["bl"].ll_get_uncertainty(model, lossnet_sd, loader)
    assert torch.equal(a, b) and torch.equal(a, c) and a.shape == (3,)
    short = {k: v for k, v in lossnet_sd.items() if k != "FC3.bias"}
    with pytest.raises(RuntimeError):
        hip["bl"].ll_get_uncertainty(model, short, loader)
    bad = dict(lossnet_sd); bad["linear.weight"] = np.zeros((1, 500), np.float32)
    with pytest.raises(RuntimeError):
        hip["bl"].ll_get_uncertainty(model, bad, loader)
