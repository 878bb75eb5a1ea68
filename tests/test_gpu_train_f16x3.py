"""forward_precision="f16x3" of the trainers: the forward of the training step on the split-fp16 kernels (conv_h3 / conv_h4), the
backward, the weight gradients and SGD on the exact fp32 ones.

  1. the device-side weight pack against the numpy restatement (tests/_train_f16x3_restatement.py), byte for byte;
  2. single launches through the dense-batch calls against the oracle of the kernel that took them, which is asserted;
  3. a trainer's body / FPN maps against HipDetector(precision="f16x3") on the same weights and image, before and after SGD steps;
  4. every trainable tensor's gradient against float64 autograd, the existing bound 1e-4 * max |grad|;
  5. run-to-run reproducibility, and forward_precision="fp32" == no keyword, in bytes;
  6. a weight that outgrows fp16's range under a stale scale: non-finite losses, no fault.
"""
import numpy as np
import pytest

import _train_f16x3_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    from cald_amd import train_ops
    if not torch.cuda.is_available():      # module-scoped: runs before conftest's function-scoped auto-skip
        pytest.skip("needs an MI355X")
    return torch, train_ops


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _w16_words(torch, pk):
    torch.cuda.synchronize()
    return pk.w16.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------------ 1. the pack
PACK_LAYERS = {                       # torch weight shape, PackedConv keywords, restatement keywords
    "3x3_64_16": ((64, 16, 3, 3), {}, {}),
    "stem_rgb0": ((64, 4, 7, 7), {}, {}),
    "linear_taps49": ((64, 16 * 49), dict(mode=2, taps=49), dict(taps=49)),
    "predictor_21+84": ((105, 1024), {}, {}),
}
PACK_CASES = [("3x3_64_16", c) for c in sorted(R.weight_cases((2, 2)))] + [(l, "pow2_minus_ulp") for l in sorted(PACK_LAYERS) if l != "3x3_64_16"]


@pytest.mark.parametrize("layer,case", PACK_CASES, ids=lambda v: v)
def test_device_pack_equals_the_restatement(T, layer, case):
    """cald_train_pack_conv16 and the plan's launches write the restatement's words; the fp32 part of the pack is the one without a twin."""
    torch, ops = T
    shape, kw, rkw = PACK_LAYERS[layer]
    w_np = R.weight_cases(shape, seed=11)[case]
    if layer == "stem_rgb0":
        w_np[:, 3] = 0.0
    w = _dev(torch, w_np)
    S, unscale = R.f16x3_scale(np.abs(w_np).max())
    assert ops.f16x3_scale(float(w.abs().max())) == (S, unscale)
    want = R.pack_w16(R.kmajor(w_np, **rkw), S)
    pk = ops.PackedConv(w, w16_S=S, **kw)
    assert pk.w16 is not None and pk.w16.numel() == want.size and pk.w16_unscale == unscale
    assert np.array_equal(_w16_words(torch, pk).reshape(want.shape), want)
    plain = ops.PackedConv(w, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pk.buf.view(torch.int32), plain.buf.view(torch.int32))
    lazy = ops.PackedConv(w, w16_S=S, pack=False, **kw)
    lazy.w16.fill_(-1); lazy.buf.fill_(float("nan"))
    ops.PackPlan([lazy], w.device).run()
    assert np.array_equal(_w16_words(torch, lazy).reshape(want.shape), want)
    assert torch.equal(lazy.buf.view(torch.int32), plain.buf.view(torch.int32))


def test_no_twin_where_the_split_kernels_take_no_such_shape(T):
    torch, ops = T
    head = ops.PackedConv(torch.randn(15, 256, 1, 1, device="cuda"), w16_S=3)          # the RPN head: 15 -> 32 padded output channels
    grad = ops.PackedConv(torch.randn(64, 64, 3, 3, device="cuda"), mode=1, w16_S=3)   # a data-gradient pack
    assert head.w16 is None and grad.w16 is None


# ------------------------------------------------------------------------------------------------------------------ 2. single launches
def _launch(T, oracle, w_np, x_np, stride=1, pad=0, relu=False, bias=None, bn=None, residual=None, up=None, cin_k=None, want_kernel="conv_h3"):
    """One ops.conv launch on N images against the oracle, image by image; returns the kernel's name."""
    torch, ops = T
    w = _dev(torch, w_np)
    S = R.f16x3_scale(np.abs(w_np).max())[0]
    d = lambda a: None if a is None else _dev(torch, a)
    pk = ops.PackedConv(w, d(bias), d(bn[0]) if bn else None, d(bn[1]) if bn else None, CinK=cin_k, w16_S=S)
    with ops.record_kernels() as log:
        got = ops.conv(d(x_np), pk, stride=stride, pad=pad, relu=relu, residual=d(residual), up=d(up))
    torch.cuda.synchronize()
    (label, kernel), = log
    assert kernel.startswith(want_kernel), (label, kernel)
    kh, kw_ = (w_np.shape[2], w_np.shape[3]) if w_np.ndim == 4 else (1, 1)
    ref = oracle.conv2d_f16x3 if kernel.startswith("conv_h") else oracle.conv2d
    rows = R.hwc_rows(w_np, cin_k)
    for n in range(x_np.shape[0]):
        want = ref(x_np[n], rows, kh, kw_, stride, pad, bias=bias, bn=bn, residual=None if residual is None else residual[n],
                   up=None if up is None else up[n], relu=relu)
        assert np.array_equal(got[n].cpu().numpy().view(np.uint32), want.view(np.uint32)), (label, kernel, n)
    return kernel


def _rand(rs, *shape, scale=1.0):
    return (rs.standard_normal(shape) * scale).astype(np.float32)


def test_launch_1x1_partial_tile_narrow(T, oracle):
    rs = np.random.RandomState(0)
    assert _launch(T, oracle, _rand(rs, 64, 64, 1, 1, scale=0.1), _rand(rs, 2, 9, 13, 64)) == "conv_h3_kernel<0,1,false>"


def test_launch_3x3_relu_residual(T, oracle):
    rs = np.random.RandomState(1)
    k = _launch(T, oracle, _rand(rs, 128, 64, 3, 3, scale=0.05), _rand(rs, 2, 10, 13, 64), pad=1, relu=True, residual=_rand(rs, 2, 10, 13, 128))
    assert k == "conv_h3_kernel<1,2,false>"


def test_launch_3x3_stride2(T, oracle):
    rs = np.random.RandomState(2)
    assert _launch(T, oracle, _rand(rs, 128, 128, 3, 3, scale=0.05), _rand(rs, 2, 11, 13, 128), stride=2, pad=1) == "conv_h3_kernel<0,2,false>"


def test_launch_stem_rgb0_bn_relu(T, oracle):
    rs = np.random.RandomState(3)
    w = np.concatenate([_rand(rs, 64, 3, 7, 7, scale=0.1), np.zeros((64, 1, 7, 7), np.float32)], axis=1)
    x = _rand(rs, 2, 37, 45, 4); x[..., 3] = 0.0
    bn = ((0.5 + rs.rand(64)).astype(np.float32), _rand(rs, 64, scale=0.1))
    assert _launch(T, oracle, w, x, stride=2, pad=3, relu=True, bn=bn) == "conv_h3_kernel<0,1,true>"


def test_launch_lateral_with_upsample_add(T, oracle):
    rs = np.random.RandomState(4)
    k = _launch(T, oracle, _rand(rs, 256, 512, 1, 1, scale=0.05), _rand(rs, 2, 10, 13, 512), bias=_rand(rs, 256, scale=0.1), up=_rand(rs, 2, 5, 7, 256))
    assert k == "conv_h3_kernel<2,2,false>"


def test_launch_rpn_head_falls_through_to_the_exact_kernel(T, oracle):
    """15 output channels: no split twin, the dispatcher's exact kernel, the exact oracle."""
    rs = np.random.RandomState(5)
    k = _launch(T, oracle, _rand(rs, 15, 256, 1, 1, scale=0.05), _rand(rs, 2, 10, 13, 256), bias=_rand(rs, 15, scale=0.1), want_kernel="conv_")
    assert not k.startswith("conv_h")


def test_launch_fc6_form_and_predictor(T, oracle):
    torch, ops = T
    rs = np.random.RandomState(6)
    w6 = _rand(rs, 1024, 256 * 49, scale=0.01); b6 = _rand(rs, 1024, scale=0.1)
    rows = _rand(rs, 40, 49 * 256)
    S = R.f16x3_scale(np.abs(w6).max())[0]
    pk = ops.PackedConv(_dev(torch, w6), _dev(torch, b6), mode=2, taps=49, w16_S=S)
    with ops.record_kernels() as log:
        f6 = ops.conv(_dev(torch, rows).view(1, 1, 40, -1), pk, relu=True)
    assert log[0][1] == "conv_h3_kernel<0,2,false>", log
    want = oracle.conv2d_f16x3(rows[None], R.kmajor(w6, taps=49)[:49 * 256, :1024], 1, 1, 1, 0, bias=b6, relu=True)
    assert np.array_equal(f6.cpu().numpy().reshape(40, 1024).view(np.uint32), want.reshape(40, 1024).view(np.uint32))
    # the merged predictor: 21 class logits + 84 box deltas in rows of 108 floats
    wp = _rand(rs, 105, 1024, scale=0.02); bp = _rand(rs, 105, scale=0.1)
    pkp = ops.PackedConv(_dev(torch, wp), _dev(torch, bp), w16_S=R.f16x3_scale(np.abs(wp).max())[0])
    x = f6.cpu().numpy().reshape(40, 1024)
    with ops.record_kernels() as log:
        pred = ops.conv(f6, pkp, out_ld=108)
    assert log[0][1] == "conv_h3_kernel<0,2,false>", log
    want = oracle.conv2d_f16x3(x[None], R.hwc_rows(wp), 1, 1, 1, 0, bias=bp)
    got = pred.cpu().numpy().reshape(40, 108)
    assert np.array_equal(got[:, :105].view(np.uint32), want.reshape(40, 105).view(np.uint32)) and not got[:, 105:].any()


def test_launch_grouped_3x3_over_five_levels_one_weight(T, oracle):
    torch, ops = T
    rs = np.random.RandomState(7)
    w = _rand(rs, 256, 256, 3, 3, scale=0.02); b = _rand(rs, 256, scale=0.1)
    pk = ops.PackedConv(_dev(torch, w), _dev(torch, b), w16_S=R.f16x3_scale(np.abs(w).max())[0])
    xs = [_rand(rs, 2, h, ww, 256) for h, ww in ((10, 13), (5, 7), (3, 4), (2, 2), (1, 1))]
    with ops.record_kernels() as log:
        ys = ops.conv_group([_dev(torch, x) for x in xs], pk, pad=1, relu=True)
    torch.cuda.synchronize()
    assert [k for _, k in log] == ["conv_h3_group_kernel<0,2,false>"] * 5, log
    rows = R.hwc_rows(w)
    for x, y in zip(xs, ys):
        for n in range(2):
            want = oracle.conv2d_f16x3(x[n], rows, 3, 3, 1, 1, bias=b, relu=True)
            assert np.array_equal(y[n].cpu().numpy().view(np.uint32), want.view(np.uint32)), x.shape


# ------------------------------------------------------------------------------------------------------------------ 3. trainer == inference mode
def _case(torch, arch, n_images=1, seed=0):
    import test_gpu_train as tg
    from cald_amd import synth
    sd, images, targets = tg._train_case(torch, n_images=n_images, seed=seed)
    if arch == "retinanet":
        sd = synth.pseudo_trained_retinanet(21, 50, seed=2)
    return sd, images, targets


def _trainer(torch, arch, sd, **kw):
    from cald_amd import train
    if arch == "frcnn":
        return train.FasterRCNNTrainer(sd, 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(7), **kw)
    return train.RetinaNetTrainer(sd, 21, min_size=160, max_size=256, **kw)


def _detector(arch, sd):
    from cald_amd import detector
    make = detector.fasterrcnn_resnet50_fpn_feature if arch == "frcnn" else detector.retinanet_resnet50_fpn_cal
    m = make(num_classes=21, min_size=160, max_size=256, precision="f16x3").to("cuda")
    m.load_state_dict(sd)
    return m


def _join_twin(twin):
    """The values of a split-form tensor (h16.h: per 16-channel chunk [16 fp16 hi | 16 fp16 lo] of 16 x), as cald_debug_tensor hands them out."""
    raw = twin.cpu().numpy().view(np.float16)                          # [..., C * 2] halves
    c = raw.reshape(raw.shape[:-1] + (raw.shape[-1] // 32, 2, 16)).astype(np.float32)
    return ((c[..., 0, :] + c[..., 1, :]) * np.float32(0.0625)).reshape(raw.shape[:-1] + (raw.shape[-1] // 2,))


def _maps(T, net):
    """{debug_tensor name: [H, W, C] values} of the last forward's image 0: the body stages, the laterals, the pyramid levels.  Where the
    trainer wrote a split twin (what every later epilogue added), its values; else the fp32 tensor."""
    torch, ops = T
    L = net.last
    first = 2 if len(net.lat) == 4 else 3
    out = {}
    named = [("C%d" % (2 + i), t, net.split_twins["feats"][i]) for i, t in enumerate(L["feats"])]
    named += [("inner%d" % (first + i), t, net.split_twins["inner"][i]) for i, t in enumerate(L["inner"])]
    named += [("P%d" % (first + i), t, None) for i, t in enumerate(L["P"])]
    for name, t, twin in named:
        assert twin is None or twin.shape == t.shape
        out[name] = (_join_twin(twin) if twin is not None else t.cpu().numpy())[0]
    return out


def _assert_maps_equal(T, net, det, image, oracle, what):
    """Byte for byte -- with one limit.  The inference mode keeps C2..C5 and the laterals in split form only; the trainer's twins of those
    hold the same words, compared as such.  It also keeps some pyramid levels in split form only (Faster R-CNN: P6; RetinaNet: all but
    P6), and debug_tensor can hand out only their 22-bit values, while the trainer has the fp32 tensor: that one is passed through
    oracle.f16x3_requantize first.  The mapping is many-to-one, so on THOSE levels a difference in the trainer's two lowest bits would
    pass; Faster R-CNN's P2..P5 and RetinaNet's P6, which both sides hold in fp32, are compared on all 32 bits."""
    torch, ops = T
    det([image])
    retina = len(net.lat) == 3
    requantized = {"P3", "P4", "P5", "P7"} if retina else {"P6"}
    maps = _maps(T, net)
    assert len(maps) == (12 if retina else 13) and all(np.isfinite(m).all() for m in maps.values())
    assert all(t is not None for t in net.split_twins["feats"] + net.split_twins["inner"])
    for name, got in maps.items():
        want = det.debug_tensor(name, 0)
        assert want.shape == got.shape, (what, name, want.shape, got.shape)
        if name in requantized:
            got = oracle.f16x3_requantize(got)
        got = np.ascontiguousarray(got, np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %s differs (max |d| %.3g)" % (what, name, float(np.abs(got - want).max()))


@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_trainer_maps_equal_the_inference_mode(T, oracle, arch):
    torch, ops = T
    from cald_amd import train
    sd, images, targets = _case(torch, arch)
    net = _trainer(torch, arch, sd, forward_precision="f16x3")
    with ops.record_kernels() as log:
        net.forward(images, targets)
    assert sum(k.startswith("conv_h") for _, k in log) > 50 and log[0][1].startswith("conv_h3_kernel<0,1,true>"), log[:3]
    _assert_maps_equal(T, net, _detector(arch, sd), images[0], oracle, "fresh weights")
    # Three SGD steps under one fixed set of scales (three plan repacks of drifting weights), ONE refresh that really moves a scale, and the
    # same again on the weights they left.  The learning rates are those at which tests/test_gpu_train.py's loops train these pseudo-trained
    # weights: at 0.01 they diverge in the fp32 mode too (measured: Faster R-CNN's loss 5.9 -> 88 -> 2.0e4, RetinaNet's 2.1 -> 311 -> 3e15).
    # Three such steps need not carry any layer's max |w| over a power of two, so one trainable lateral is doubled by hand before the refresh.
    model = train.TrainableDetector(net)
    opt = train.SGD(model.parameters(), lr=2e-3 if arch == "frcnn" else 2e-5, momentum=0.9, weight_decay=1e-4, net=net)
    scales = [cv.w16_S for cv in net.convs]
    for _ in range(3):
        losses = sum(model(images, targets).values())
        opt.zero_grad(); losses.backward(); opt.step()
        assert [cv.w16_S for cv in net.convs] == scales, "a step must not touch the scales"
    with torch.no_grad():
        net.params["backbone.fpn.inner_blocks.1.weight"].mul_(2.0)
    net.parameters_changed()
    assert net.refresh_f16x3_scales() >= 1 and net.lat[1].w16_S < scales[net.convs.index(net.lat[1])], "the refresh must move a scale"
    net.forward(images, targets)
    assert bool(torch.isfinite(net.flat).all())
    moved = [not torch.equal(v.cpu(), torch.as_tensor(sd[k]).float()) for k, v in net.state_dict().items() if k in net.params]
    assert sum(moved) > len(moved) // 2, "the steps must have moved the trainable tensors"
    _assert_maps_equal(T, net, _detector(arch, net.state_dict()), images[0], oracle, "after three SGD steps and a refresh")


def test_split_activations_are_refused_where_conv_h3_would_not_take_the_launch(T):
    """Residual AND up with a split addend (conv_h3 refuses both together; the exact kernel would read the twin as fp32), and split tensors
    without a twinned pack: loud on both sides of the C ABI, nothing launched."""
    torch, ops = T
    import ctypes as C
    from cald_amd import _ffi
    from cald_amd.detector import get_ctx
    w = torch.randn(64, 64, 1, 1, device="cuda") * 0.1
    pk = ops.PackedConv(w, w16_S=R.f16x3_scale(float(w.abs().max()))[0])
    x = torch.randn(1, 4, 4, 64, device="cuda"); r = torch.randn(1, 4, 4, 64, device="cuda"); u = torch.randn(1, 2, 2, 64, device="cuda")
    twin = torch.zeros((1, 4, 4, 64), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.conv(x, pk, residual=r, up=u, ex16=twin)
    with pytest.raises(ValueError):
        ops.conv(x, ops.PackedConv(w), x16=twin)
    out = torch.empty_like(r)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda res, up_, w16, ex16: _ffi.lib().cald_train_conv_f16x3(
        get_ctx(0), 1, 4, 4, p(x), 64, p(pk.buf), 64, 64, 1, 1, 1, 0, 0, 0, res, up_, 2, 2, None, p(out), 64, w16, pk.w16_unscale, None, ex16, None, None)
    assert call(p(twin), p(u), p(pk.w16), 1) != 0          # residual and up with a split addend
    assert call(p(twin), None, None, 1) != 0               # a split addend without the pack's twin
    assert call(p(twin), None, p(pk.w16), 1) == 0          # the launch conv_h3 takes
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 4. gradients
def _worst_gradient_ratio(torch, grads, tr):
    worst = ("", 0.0)
    for k, g in grads.items():
        w = tr[k].grad
        assert w is not None and float(w.abs().max()) > 0, k
        err = float((g.double().cpu() - w).abs().max()) / float(w.abs().max())
        if err > worst[1]:
            worst = (k, err)
    return worst


@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_gradients_vs_float64_autograd(T, oracle, arch):
    """The exact backward on the activations the f16x3 forward saved: every trainable tensor within 1e-4 of its largest magnitude of
    float64 autograd on the same proposals, samples and ReLU decisions (the bound of the fp32 step's test)."""
    torch, ops = T
    from oracle import torch_train as tt
    sd, images, targets = _case(torch, arch, n_images=2, seed=0 if arch == "frcnn" else 6)
    net = _trainer(torch, arch, sd, forward_precision="f16x3")
    net.forward(images, targets)
    grads = {k: v.clone() for k, v in net.backward().items()}
    if arch == "frcnn":
        ref = tt.TorchTrainFRCNN(sd, 21, min_size=160, max_size=256)
        ref.masks = net.relu_decisions()
        want, rec = ref.losses(images, targets, [p.cpu() for p in net.last["proposals"]], None, cfg=dict(box_batch=64), samples=net.last["samples"])
        assert torch.equal(rec["roi_labels"], net.last["roi_labels"]), "same sampled RoIs"
    else:
        ref = tt.TorchTrainRetinaNet(sd, 21, min_size=160, max_size=256)
        ref.masks = net.relu_decisions()
        want, rec = ref.losses(images, targets)
        assert torch.equal(rec["matched"].int(), torch.from_numpy(net.last["matched_host"])), "same anchor matching"
    sum(want.values()).backward()
    tr = ref.trainable()
    assert sorted(tr) == sorted(grads)
    name, ratio = _worst_gradient_ratio(torch, grads, tr)
    print("forward_precision=f16x3 %s: worst gradient error / max|grad| = %.3g at %s" % (arch, ratio, name))
    assert ratio <= 1e-4, "largest gradient error %.3g at %s" % (ratio, name)


# ------------------------------------------------------------------------------------------------------------------ 5. reproducibility, default
def _three_steps(T, arch, sd, images, targets, **kw):
    """Three SGD steps at the learning rates tests/test_gpu_train.py's loops use on these pseudo-trained weights."""
    torch, ops = T
    from cald_amd import train
    net = _trainer(torch, arch, sd, **kw)
    model = train.TrainableDetector(net)
    opt = train.SGD(model.parameters(), lr=2e-3 if arch == "frcnn" else 2e-5, momentum=0.9, weight_decay=1e-4, net=net)
    for _ in range(3):
        losses = sum(model(images, targets).values())
        opt.zero_grad(); losses.backward(); opt.step()
    torch.cuda.synchronize()
    return net.flat.clone(), opt._mflat.clone()


@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_three_steps_are_bit_reproducible(T, arch):
    torch, ops = T
    sd, images, targets = _case(torch, arch, n_images=2, seed=21)
    a = _three_steps(T, arch, sd, images, targets, forward_precision="f16x3")
    b = _three_steps(T, arch, sd, images, targets, forward_precision="f16x3")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert bool(torch.isfinite(a[0]).all())


@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_fp32_keyword_is_the_default_in_bytes(T, arch):
    torch, ops = T
    sd, images, targets = _case(torch, arch, n_images=2, seed=21)
    a = _three_steps(T, arch, sd, images, targets)
    b = _three_steps(T, arch, sd, images, targets, forward_precision="fp32")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    c = _three_steps(T, arch, sd, images, targets, forward_precision="f16x3")
    assert not torch.equal(a[0].view(torch.int32), c[0].view(torch.int32)), "the f16x3 forward must not be the fp32 one"


def test_ll_trainers_take_the_keyword(T):
    torch, ops = T
    from cald_amd import train
    sd, images, targets = _case(torch, "frcnn", n_images=2, seed=21)
    net = train.FasterRCNNTrainer(sd, 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(7), loss_mode="ll",
                                  forward_precision="f16x3")
    with ops.record_kernels() as log:
        losses, pooled = net.forward(images, targets)
    assert sum(k.startswith("conv_h") for _, k in log) > 50 and all(bool(torch.isfinite(v).all()) for v in losses.values())
    sd, images, targets = _case(torch, "retinanet", n_images=2, seed=21)
    net = train.RetinaNetLLTrainer(sd, 21, min_size=160, max_size=256, forward_precision="f16x3")
    with ops.record_kernels() as log:
        losses, pooled = net.forward(images, targets)
    assert sum(k.startswith("conv_h") for _, k in log) > 50 and all(bool(torch.isfinite(v).all()) for v in losses.values())


# ------------------------------------------------------------------------------------------------------------------ 6. overflow under a stale scale
def test_weight_outgrowing_the_stale_scale_gives_non_finite_losses(T):
    """The predictor's class rows x 2^20 without a refresh: their hi halves pack as inf, the class logits and the classification loss
    turn non-finite (train_one_epoch's "Loss is ..., stopping training"), nothing faults; after a refresh the same weights pack finite.
    (A layer with a ReLU would hide it: max(NaN, 0) = 0 -- DESIGN.md section 8 says so; the heads' output layers have none.)"""
    torch, ops = T
    sd, images, targets = _case(torch, "frcnn", n_images=1, seed=3)
    net = _trainer(torch, "frcnn", sd, forward_precision="f16x3")
    first = {k: float(v) for k, v in net.forward(images, targets).items()}
    assert all(np.isfinite(v) for v in first.values())
    with torch.no_grad():
        net.params["roi_heads.box_predictor.cls_score.weight"].mul_(2.0 ** 20)
    losses = {k: float(v) for k, v in net.forward(images, targets).items()}
    torch.cuda.synchronize()
    assert not np.isfinite(losses["loss_classifier"]), losses
    assert np.isfinite(losses["loss_objectness"]) and np.isfinite(losses["loss_rpn_box_reg"]), losses
    assert net.refresh_f16x3_scales() == 1
    net.forward(images, targets)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(net.last["pred"]).all())
