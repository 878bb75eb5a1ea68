"""backward_precision="f16x3" of the trainers: the data gradients of the training step on conv_h3 (three fp16 MFMAs per product) with a
per-tensor gradient scale; the weight gradients, the RoIAlign backward, the losses and SGD stay exact fp32.

  1. the device twin of a data-gradient pack against the restatement (tests/_train_f16x3_grad_restatement.py), word for word;
  2. single data-gradient launches, bit for bit against the restatement (checked on the CPU against float64 by tests/test_train_f16x3_grad.py);
  3. the grouped launch over five levels with masks;
  4. a gradient that outgrows a stale scale: still exact at x 16, non-finite at x 2^8, no fault;
  5. the trainers: gradients against float64 autograd, the calibration step, reproducibility, the default in bytes.
"""
import numpy as np
import pytest

import _train_f16x3_grad_restatement as GR
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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rand(rs, *shape, scale=1.0):
    return (rs.standard_normal(shape) * scale).astype(np.float32)


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ 1. the pack
PACK_LAYERS = {                       # torch weight shape, PackedConv keywords, restatement keywords
    "3x3_64<-16": ((16, 64, 3, 3), dict(mode=1), {}),
    "1x1_80<-32_npad128": ((32, 80, 1, 1), dict(mode=1), {}),
    "linear_taps49": ((32, 16 * 49), dict(mode=3, taps=49), dict(taps=49)),
}


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn_rowscale"])
@pytest.mark.parametrize("layer", sorted(PACK_LAYERS))
def test_device_grad_twin_equals_the_restatement(T, layer, bn):
    """cald_train_pack_conv16 and the plan write the restatement's words for a data-gradient pack (transposed, flipped, row scale folded in;
    weights just below a power of two); the fp32 part of the pack is the one without a twin."""
    torch, ops = T
    shape, kw, rkw = PACK_LAYERS[layer]
    w_np = R.weight_cases(shape, seed=13)["pow2_minus_ulp"]
    sc_np = (0.5 + np.random.RandomState(5).rand(shape[0])).astype(np.float32) if bn else None
    wd = GR.grad_filter(w_np, sc_np, **rkw)
    S, want = GR.grad_twin(wd)
    w, sc = _dev(torch, w_np), _dev(torch, sc_np)
    assert ops.f16x3_scale(float(np.abs(wd).max()))[0] == S
    pk = ops.PackedConv(w, scale=sc, grad16_S=S, **kw)
    assert pk.w16 is not None and pk.w16.numel() == want.size and pk.w16_S == S
    torch.cuda.synchronize()
    assert np.array_equal(pk.w16.cpu().numpy().view(np.uint16).reshape(want.shape), want)
    plain = ops.PackedConv(w, scale=sc, **kw)
    assert plain.w16 is None and ops.PackedConv(w, scale=sc, w16_S=S, **kw).w16 is None       # the forward keyword asks for no grad twin
    torch.cuda.synchronize()
    nw = pk.w16.numel()                  # 2 Kpad NPad: the two weight layouts (a data-gradient pack writes no epilogue vectors behind them)
    assert torch.equal(pk.buf[:nw].view(torch.int32), plain.buf[:nw].view(torch.int32))
    lazy = ops.PackedConv(w, scale=sc, grad16_S=S, pack=False, **kw)
    lazy.w16.fill_(-1); lazy.buf.fill_(float("nan"))
    ops.PackPlan([lazy], w.device).run()
    torch.cuda.synchronize()
    assert np.array_equal(lazy.w16.cpu().numpy().view(np.uint16).reshape(want.shape), want)
    assert torch.equal(lazy.buf[:nw].view(torch.int32), plain.buf[:nw].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 2. single launches
MAGS = [1e-8, 1e-3, 1e3, 0.0]


def _masks(rs, shape):
    """{name: saved activation}: random signs with whole pixel rows <= 0, and a single positive entry."""
    rows = _rand(rs, *shape)
    rows[:, ::2] = -np.abs(rows[:, ::2])
    rows[:, 1, 1::2] = 0.0
    one = -np.ones(shape, np.float32)
    one.reshape(-1)[shape[-1] + 3] = 2.0
    return {"rows_nonpositive": rows, "single_positive": one}


def _dgrad_launch(T, oracle, w_np, hw, g_np, stride=1, pad=0, scale=None, residual=None, mask=None, want_kernel=None, G=None, g_launch=None, compare=True):
    """ops.conv_dgrad of N images on the twinned pack against the restatement, image by image.  G: the exponent to launch with (default: the
    policy's for g_np); g_launch: the tensor actually launched (default g_np).  Returns (kernel name, output as numpy)."""
    torch, ops = T
    H, W = hw
    K = w_np.shape[2]
    wd = GR.grad_filter(w_np, scale)
    S = R.f16x3_scale(np.abs(wd).max())[0]
    pkd = ops.PackedConv(_dev(torch, w_np), scale=_dev(torch, scale), mode=1, grad16_S=S)
    assert pkd.w16 is not None
    if G is None:
        G = GR.grad_scale(np.abs(g_np).max())[0]
        assert ops.f16x3_grad_scale(float(np.abs(g_np).max()))[0] == G
    g_run = g_np if g_launch is None else g_launch
    with ops.record_dgrad_kernels() as log, ops.record_kernels() as fwd_log:
        got = ops.conv_dgrad(_dev(torch, g_run), pkd, H, W, stride, pad, residual=_dev(torch, residual), mask=_dev(torch, mask), G=G)
    torch.cuda.synchronize()
    (label, kernel), = log
    assert not fwd_log, "a data gradient is no forward launch"
    if want_kernel is not None:
        assert kernel == want_kernel, (label, kernel)
    wp = GR.prepare(oracle, wd)
    got = got.cpu().numpy()
    for n in range(g_run.shape[0] if compare else 0):
        if stride > 1 and K == 1:            # strided 1 x 1: the product on the coarse grid, then scattered
            want = GR.dilate(GR.dgrad(oracle, g_run[n], wd, 0, G, prepared=wp), stride, H, W)
        else:
            gd = GR.dilate(g_run[n], stride, H + 2 * pad - K + 1, W + 2 * pad - K + 1) if stride > 1 else g_run[n]
            want = GR.dgrad(oracle, gd, wd, K - 1 - pad, G, residual=None if residual is None else residual[n],
                            mask=None if mask is None else mask[n], prepared=wp)
        assert np.array_equal(_bits(got[n]), _bits(want)), (label, kernel, n, float(np.nanmax(np.abs(got[n] - want))))
    return kernel, got


@pytest.mark.parametrize("mag", MAGS)
def test_dgrad_1x1_partial_tile_narrow(T, oracle, mag):
    rs = np.random.RandomState(0)
    _dgrad_launch(T, oracle, _rand(rs, 64, 64, 1, 1, scale=0.1), (9, 13), _rand(rs, 2, 9, 13, 64, scale=mag), want_kernel="conv_h3_kernel<0,1,false>")


@pytest.mark.parametrize("mask", ["rows_nonpositive", "single_positive"])
@pytest.mark.parametrize("mag", MAGS)
def test_dgrad_3x3_residual_and_mask_small(T, oracle, mag, mask):
    rs = np.random.RandomState(1)
    w = _rand(rs, 64, 128, 3, 3, scale=0.05)
    bn = (0.5 + rs.rand(64)).astype(np.float32)
    k, got = _dgrad_launch(T, oracle, w, (5, 7), _rand(rs, 1, 5, 7, 64, scale=mag), pad=1, scale=bn, residual=_rand(rs, 1, 5, 7, 128, scale=mag),
                           mask=_masks(rs, (1, 5, 7, 128))[mask], want_kernel="conv_h3_kernel<5,2,false>")
    if mask == "single_positive":
        assert np.count_nonzero(got) <= 1


@pytest.mark.parametrize("mag", MAGS)
def test_dgrad_3x3_residual_and_mask_several_m_tiles(T, oracle, mag):
    rs = np.random.RandomState(2)
    w = _rand(rs, 64, 64, 3, 3, scale=0.05)
    _dgrad_launch(T, oracle, w, (24, 24), _rand(rs, 2, 24, 24, 64, scale=mag), pad=1, residual=_rand(rs, 2, 24, 24, 64, scale=mag),
                  mask=_masks(rs, (2, 24, 24, 64))["rows_nonpositive"], want_kernel="conv_h3_kernel<5,1,false>")


@pytest.mark.parametrize("mag", MAGS)
def test_dgrad_3x3_stride2_odd_sizes_through_dilate(T, oracle, mag):
    rs = np.random.RandomState(3)
    w = _rand(rs, 64, 64, 3, 3, scale=0.05)
    _dgrad_launch(T, oracle, w, (9, 13), _rand(rs, 2, 5, 7, 64, scale=mag), stride=2, pad=1, mask=_masks(rs, (2, 9, 13, 64))["rows_nonpositive"],
                  want_kernel="conv_h3_kernel<4,1,false>")


@pytest.mark.parametrize("mag", MAGS)
def test_dgrad_strided_1x1_on_the_coarse_grid(T, oracle, mag):
    rs = np.random.RandomState(4)
    _dgrad_launch(T, oracle, _rand(rs, 128, 64, 1, 1, scale=0.05), (9, 13), _rand(rs, 2, 5, 7, 128, scale=mag), stride=2,
                  want_kernel="conv_h3_kernel<0,1,false>")


@pytest.mark.parametrize("rows", [3, 257])
@pytest.mark.parametrize("mag", MAGS)
def test_dgrad_linear_forms(T, oracle, mag, rows):
    """fc6's form (mode 3: gradient rows -> [tap][Cin] rows) and the predictor's (105 outputs in rows of 112 floats, the pad columns zero),
    the latter with the mask of the hidden layer it flows into."""
    torch, ops = T
    rs = np.random.RandomState(6)
    w6 = _rand(rs, 64, 16 * 49, scale=0.01)
    wd6 = GR.grad_filter(w6, cin_k=64, taps=49)
    pk6 = ops.PackedConv(_dev(torch, w6), mode=3, taps=49, grad16_S=R.f16x3_scale(np.abs(wd6).max())[0])
    g6 = _rand(rs, rows, 64, scale=mag)
    G6 = GR.grad_scale(np.abs(g6).max())[0]
    with ops.record_dgrad_kernels() as log:
        d6 = ops.conv(_dev(torch, g6).view(1, 1, rows, 64), pk6, G=G6)
    assert log[0][1] == "conv_h3_kernel<0,2,false>", log
    assert np.array_equal(_bits(d6).reshape(rows, -1), _bits(GR.dgrad(oracle, g6[None], wd6, 0, G6)).reshape(rows, -1))
    wp = _rand(rs, 105, 128, scale=0.02)
    wdp = GR.grad_filter(wp, cin_k=112)
    pkp = ops.PackedConv(_dev(torch, wp), CinK=112, mode=1, grad16_S=R.f16x3_scale(np.abs(wdp).max())[0])
    gp = np.zeros((rows, 112), np.float32); gp[:, :105] = _rand(rs, rows, 105, scale=mag)
    Gp = GR.grad_scale(np.abs(gp).max())[0]
    hidden = _rand(rs, rows, 128)
    with ops.record_dgrad_kernels() as log:
        dp = ops.conv(_dev(torch, gp).view(1, 1, rows, 112), pkp, mask=_dev(torch, hidden).view(1, 1, rows, 128), G=Gp)
    assert log[0][1] == "conv_h3_kernel<4,2,false>", log
    assert np.array_equal(_bits(dp).reshape(rows, -1), _bits(GR.dgrad(oracle, gp[None], wdp, 0, Gp, mask=hidden[None])).reshape(rows, -1))


def test_dgrad_of_a_shape_conv_h3_does_not_take_runs_the_exact_kernel(T):
    """A 15-channel input: the data gradient has 15 -> 32 padded output channels, the pack gets no twin, the launch with a gradient exponent
    is the exact kernel's, byte for byte the launch without one, and the dgrad log names that kernel."""
    torch, ops = T
    rs = np.random.RandomState(8)
    w = _dev(torch, _rand(rs, 64, 15, 1, 1, scale=0.1))
    g = _dev(torch, _rand(rs, 2, 9, 13, 64, scale=1e-3))
    pkd = ops.PackedConv(w, mode=1, grad16_S=3)
    assert pkd.w16 is None and ops.packed_grad16_bytes(64, 15, 1, 1, 64, 1) == 0 and ops.packed_grad16_bytes(64, 64, 3, 3, 64, 1) > 0
    with ops.record_dgrad_kernels() as log:
        a = ops.conv_dgrad(g, pkd, 9, 13, 1, 0, G=12)
    b = ops.conv_dgrad(g, ops.PackedConv(w, mode=1), 9, 13, 1, 0)
    torch.cuda.synchronize()
    assert len(log) == 1 and log[0][1].startswith("conv_") and not log[0][1].startswith("conv_h"), log
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 3. the grouped launch
def test_dgrad_grouped_3x3_over_five_levels_with_masks(T, oracle):
    torch, ops = T
    rs = np.random.RandomState(7)
    w = _rand(rs, 256, 256, 3, 3, scale=0.02)
    wd = GR.grad_filter(w)
    pkd = ops.PackedConv(_dev(torch, w), mode=1, grad16_S=R.f16x3_scale(np.abs(wd).max())[0])
    levels = ((25, 34), (13, 17), (7, 9), (4, 5), (2, 3))
    gs = [_rand(rs, 2, h, ww, 256, scale=1e-3 * 4.0 ** -i) for i, (h, ww) in enumerate(levels)]
    masks = [_masks(rs, g.shape)["rows_nonpositive"] for g in gs]
    Gs = [GR.grad_scale(np.abs(g).max())[0] for g in gs]
    assert len(set(Gs)) > 1, "the levels must carry different exponents"
    with ops.record_dgrad_kernels() as log:
        ys = ops.conv_group([_dev(torch, g) for g in gs], pkd, pad=1, masks=[_dev(torch, m) for m in masks], Gs=Gs)
    torch.cuda.synchronize()
    assert [k for _, k in log] == ["conv_h3_group_kernel<4,2,false>"] * 5, log
    wp = GR.prepare(oracle, wd)
    for g, m, G, y in zip(gs, masks, Gs, ys):
        for n in range(2):
            want = GR.dgrad(oracle, g[n], wd, 1, G, mask=m[n], prepared=wp)
            assert np.array_equal(_bits(y[n]), _bits(want)), g.shape


# ------------------------------------------------------------------------------------------------------------------ 4. a stale scale
def test_gradient_outgrowing_a_stale_scale(T, oracle):
    """x 16 under the unchanged G: max |g| 2^(4 + G) < 2^15, every half finite, still the restatement bit for bit.  x 2^8: >= 2^18, the hi
    halves are inf and the lo halves -inf -- non-finite outputs by IEEE arithmetic on finite inputs, no error code, nothing faults."""
    torch, ops = T
    rs = np.random.RandomState(9)
    w = _rand(rs, 64, 64, 3, 3, scale=0.05)
    g = _rand(rs, 1, 10, 13, 64, scale=1e-3)
    G = GR.grad_scale(np.abs(g).max())[0]
    _, got = _dgrad_launch(T, oracle, w, (10, 13), g, pad=1, G=G, g_launch=g * np.float32(16.0))
    assert np.isfinite(got).all()
    _, got = _dgrad_launch(T, oracle, w, (10, 13), g, pad=1, G=G, g_launch=g * np.float32(256.0), compare=False)     # (NaN payloads are not pinned)
    assert not np.isfinite(got).all()
    _, got = _dgrad_launch(T, oracle, w, (10, 13), g, pad=1, G=G)                                                    # and the device is fine afterwards
    assert np.isfinite(got).all()


# ------------------------------------------------------------------------------------------------------------------ 5. the trainers
def _fx():
    import test_gpu_train_f16x3 as fx              # the forward mode's cases, trainers and step loop
    return fx


def _grads_after(torch, ops, net, images, targets, backwards):
    """The gradients of the `backwards`-th backward on the same batch (a clone), and that backward's dgrad log."""
    for i in range(backwards):
        net.forward(images, targets)
        with ops.record_dgrad_kernels() as log:
            g = net.backward()
    torch.cuda.synchronize()
    return net.gflat.clone(), {k: v.clone() for k, v in g.items()}, log


@pytest.mark.parametrize("fwd", ["fp32", "f16x3"])
@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_gradients_vs_float64_autograd(T, oracle, arch, fwd):
    """The second backward (the first is the calibration step) with the data gradients on conv_h3: every trainable tensor within 1e-4 of its
    largest magnitude of float64 autograd on the same proposals, samples and ReLU decisions -- the bound of the fp32 step's test and of the
    f16x3 forward's.  Measured worst ratios (max over tensors, 2 images, 160 / 256): see the printed line; DESIGN.md section 8 quotes them."""
    torch, ops = T
    fx = _fx()
    from oracle import torch_train as tt
    sd, images, targets = fx._case(torch, arch, n_images=2, seed=0 if arch == "frcnn" else 6)
    net = fx._trainer(torch, arch, sd, forward_precision=fwd, backward_precision="f16x3")
    net.forward(images, targets); net.backward()                 # calibration
    assert net._calib is None and len(net._grad_G) > 40
    net.generator.manual_seed(7) if arch == "frcnn" else None
    net.forward(images, targets)
    with ops.record_dgrad_kernels() as log:
        grads = {k: v.clone() for k, v in net.backward().items()}
    assert sum(k.startswith("conv_h3") for _, k in log) > 40, log
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
    name, ratio = fx._worst_gradient_ratio(torch, grads, tr)
    print("forward_precision=%s backward_precision=f16x3 %s: worst gradient error / max|grad| = %.3g at %s" % (fwd, arch, ratio, name))
    assert ratio <= 1e-4, "largest gradient error %.3g at %s" % (ratio, name)


@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_first_backward_calibrates_on_the_exact_kernels(T, arch):
    """The first backward after construction equals the fp32 trainer's byte for byte and launches no conv_h3; from the second on the dgrad
    log shows more than 40 conv_h3 launches and the gradients differ from the fp32 trainer's in at least one word."""
    torch, ops = T
    fx = _fx()
    sd, images, targets = fx._case(torch, arch, n_images=2, seed=21)
    ref1, _, ref_log = _grads_after(torch, ops, fx._trainer(torch, arch, sd), images, targets, 1)
    assert ref_log and not any(k.startswith("conv_h") for _, k in ref_log)
    net = fx._trainer(torch, arch, sd, backward_precision="f16x3")
    assert net._calib == [] and not net._grad_G
    got1, _, log1 = _grads_after(torch, ops, net, images, targets, 1)
    assert not any(k.startswith("conv_h") for _, k in log1) and net._calib is None and net._grad_G
    assert torch.equal(got1.view(torch.int32), ref1.view(torch.int32))
    ref2, _, _ = _grads_after(torch, ops, fx._trainer(torch, arch, sd), images, targets, 2)
    net = fx._trainer(torch, arch, sd, backward_precision="f16x3")
    got2, _, log2 = _grads_after(torch, ops, net, images, targets, 2)
    assert sum(k.startswith("conv_h3") for _, k in log2) > 40, log2
    assert bool(torch.isfinite(got2).all()) and not torch.equal(got2.view(torch.int32), ref2.view(torch.int32))
    assert net.refresh_f16x3_scales() == 0 and net._calib == [], "a refresh marks the next backward as a calibration step"


@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_three_steps_are_bit_reproducible(T, arch):
    torch, ops = T
    fx = _fx()
    sd, images, targets = fx._case(torch, arch, n_images=2, seed=21)
    a = fx._three_steps(T, arch, sd, images, targets, backward_precision="f16x3")
    b = fx._three_steps(T, arch, sd, images, targets, backward_precision="f16x3")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert bool(torch.isfinite(a[0]).all())


@pytest.mark.parametrize("arch", ["frcnn", "retinanet"])
def test_fp32_keyword_is_the_default_in_bytes(T, arch):
    """backward_precision="fp32" == no keyword after three steps (the existing default path, which tests/test_gpu_train_f16x3.py pins);
    with the f16x3 forward it reproduces the forward-only mode; the f16x3 backward is not the fp32 one."""
    torch, ops = T
    fx = _fx()
    sd, images, targets = fx._case(torch, arch, n_images=2, seed=21)
    eq = lambda p, q: torch.equal(p[0].view(torch.int32), q[0].view(torch.int32)) and torch.equal(p[1].view(torch.int32), q[1].view(torch.int32))
    a = fx._three_steps(T, arch, sd, images, targets)
    assert eq(a, fx._three_steps(T, arch, sd, images, targets, backward_precision="fp32"))
    f = fx._three_steps(T, arch, sd, images, targets, forward_precision="f16x3")
    assert eq(f, fx._three_steps(T, arch, sd, images, targets, forward_precision="f16x3", backward_precision="fp32"))
    assert not eq(a, fx._three_steps(T, arch, sd, images, targets, backward_precision="f16x3")), "the f16x3 backward must not be the fp32 one"


def test_ll_trainers_take_the_keyword(T):
    torch, ops = T
    fx = _fx()
    from cald_amd import train
    sd, images, targets = fx._case(torch, "frcnn", n_images=2, seed=21)
    net = train.FasterRCNNTrainer(sd, 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(7), loss_mode="ll",
                                  backward_precision="f16x3")
    for _ in range(2):
        losses, pooled = net.forward(images, targets)
        with ops.record_dgrad_kernels() as log:
            net.backward()
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()) and sum(k.startswith("conv_h3") for _, k in log) > 40
    assert bool(torch.isfinite(net.gflat).all())
    sd, images, targets = fx._case(torch, "retinanet", n_images=2, seed=21)
    net = train.RetinaNetLLTrainer(sd, 21, min_size=160, max_size=256, backward_precision="f16x3")
    for _ in range(2):
        losses, pooled = net.forward(images, targets)
        with ops.record_dgrad_kernels() as log:
            net.backward()
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()) and sum(k.startswith("conv_h3") for _, k in log) > 40
    assert bool(torch.isfinite(net.gflat).all())


def test_bad_keyword_raises(T):
    torch, ops = T
    fx = _fx()
    sd, images, targets = fx._case(torch, "frcnn")
    with pytest.raises(ValueError, match="backward_precision"):
        fx._trainer(torch, "frcnn", sd, backward_precision="bf16")
