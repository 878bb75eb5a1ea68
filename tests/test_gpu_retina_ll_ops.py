"""GPU tests of the operators RetinaNetLLTrainer adds or reuses (train_loss.hip's per-image focal loss and the batch mean, smooth_l1_seg as
the per-image L1, cald_train_gap on P3..P6): against the float64 restatement (tests/_retina_ll_restatement.py, pinned to the executed
reference by tests/test_retina_ll_train.py), against the executed reference itself (tests/golden/retina_ll_train.npz), and bit for bit
where the summation geometry promises bits.  Bounds: loss 2e-6 and gradient 1e-5 of the largest entry, those of
test_gpu_train.py::test_focal_and_l1_losses_value_and_gradient.  The tests that build a trainer are in tests/test_gpu_train_retina_ll.py."""
import numpy as np
import pytest

import _retina_ll_restatement as R

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GS = [0.7, 1.3, 0.4]
# (A, K, ld, level_pix): fewer anchors than one block; per-image totals 256, 257, 512, 513 with one anchor per pixel; the 160 x 256 training
# batch (31 blocks per image, the last one partial); COCO's class count
SHAPES = [(9, 3, 28, [6, 2, 1, 1, 1]), (1, 1, 4, [249, 3, 2, 1, 1]), (1, 1, 4, [250, 3, 2, 1, 1]), (1, 1, 4, [505, 3, 2, 1, 1]),
          (1, 1, 4, [506, 3, 2, 1, 1]), (9, 20, 180, [640, 160, 40, 12, 4]), (9, 91, 820, [6, 2, 1, 1, 1])]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():      # module-scoped: runs before conftest's function-scoped auto-skip
        pytest.skip("needs an MI355X")
    from cald_amd import train_ops
    return torch, train_ops


@pytest.fixture(scope="module")
def fx(golden):
    return golden("retina_ll_train")


def _close(got, want, tol, what):
    got = got.detach().double().cpu().numpy() if hasattr(got, "detach") else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if hasattr(want, "detach") else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    scale = max(1e-30, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    print("%s: max err / max|ref| = %.3g" % (what, err))
    assert err <= tol, "%s: max err / max|ref| = %.3g > %.3g" % (what, err, tol)


def _each(got, want, tol, what):
    """every entry within tol of ITS reference value (a per-image loss is a value of its own, not a part of a tensor)"""
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
    err[want == 0] = np.where(got[want == 0] == 0, 0.0, np.inf)
    print("%s: largest relative error %.3g" % (what, float(err.max())))
    assert float(err.max()) <= tol, "%s: relative errors %s > %.3g" % (what, err, tol)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _blocks(flat, N, level_pix, ld):
    """the five [N, pix_l, ld] views of a flat head buffer"""
    out, o = [], 0
    for n in level_pix:
        out.append(flat[o:o + N * n * ld].view(N, n, ld)); o += N * n * ld
    return out


def _image_logits(flat, N, level_pix, ld, A, K, i):
    """image i's logits [A_tot][K] in anchor order (level, pixel, anchor)"""
    import torch
    return torch.cat([b[i, :, :A * K].reshape(-1, K) for b in _blocks(flat, N, level_pix, ld)])


def _alone(flat, N, level_pix, ld, i):
    """the flat buffer of image i submitted alone"""
    import torch
    return torch.cat([b[i:i + 1].reshape(-1) for b in _blocks(flat, N, level_pix, ld)]).contiguous()


def _case(torch, A, K, ld, level_pix, seed=0, N=3):
    """Logits gaussian * 3 with 0, -0 and +-30 planted, NaN in the pad columns.  Image 0: everything background (#fg 0, denom 1); image 1:
    every anchor ignored; image 2 (and any further one): mixed, with a foreground anchor at its first and at its last anchor."""
    g = torch.Generator().manual_seed(seed)
    At = A * sum(level_pix)
    flat = torch.full((N * sum(level_pix) * ld,), float("nan"))
    for b in _blocks(flat, N, level_pix, ld):
        b[:, :, :A * K] = torch.randn(b.shape[0], b.shape[1], A * K, generator=g) * 3
    first = _blocks(flat, N, level_pix, ld)[0]
    for i in range(N):
        for j, v in enumerate((0.0, -0.0, 30.0, -30.0, 30.0)[:first.shape[1]]):
            first[i, j, 0 if j < 4 else A * K - 1] = v      # pixels 0..4 of level 0: channel 0, and the last valid channel
    n_gt = [2, 1] + [3] * (N - 2)
    gt_off = np.cumsum([0] + n_gt[:N])
    gt_labels = torch.randint(0, K, (int(gt_off[-1]),), generator=g, dtype=torch.int64)
    matched = torch.full((N, At), -1, dtype=torch.int32)
    if N > 1:
        matched[1] = -2
    for i in range(2, N):
        matched[i] = torch.randint(-2, 3, (At,), generator=g, dtype=torch.int32)
        matched[i, 0], matched[i, At - 1] = 1, 2
    nfg = [int((matched[i] >= 0).sum()) for i in range(N)]
    return dict(flat=flat, matched=matched, gt_labels=gt_labels, gt_off=torch.from_numpy(gt_off.astype(np.int32)), nfg=nfg,
                denom=[float(max(1, n)) for n in nfg], N=N, A=A, K=K, ld=ld, level_pix=level_pix, At=At)


def _want(torch, c, gs):
    """float64: the per-image losses [N] and the gradient of sum_n gs[n] * loss_n with respect to the flat buffer (0 in the pad columns)"""
    from oracle import torch_train as tt
    fd = c["flat"].double().requires_grad_(True)
    out = []
    for i in range(c["N"]):
        logits = _image_logits(fd, c["N"], c["level_pix"], c["ld"], c["A"], c["K"], i)
        m = c["matched"][i].long()
        fg, valid = m >= 0, m != -2
        tgt = torch.zeros_like(logits)
        tgt[fg, c["gt_labels"][c["gt_off"][i].long() + m[fg]]] = 1.0
        out.append(tt.sigmoid_focal_loss_sum(logits[valid], tgt[valid]) / c["denom"][i])
    out = torch.stack(out)
    (out * torch.tensor(gs, dtype=torch.float64)).sum().backward()
    return out.detach(), torch.nan_to_num(fd.grad)


def _grad_buffer(torch, c, N=None):
    N = c["N"] if N is None else N
    g = torch.full((N * sum(c["level_pix"]) * c["ld"],), SENTINEL)
    for b in _blocks(g, N, c["level_pix"], c["ld"]):
        b[:, :, :c["A"] * c["K"]] = 0.0
    return g.cuda()


def _valid(c, grad, N=None):
    """(valid columns of the gradient as one vector, True when every pad word still holds the sentinel)"""
    import torch
    N = c["N"] if N is None else N
    bl = _blocks(grad, N, c["level_pix"], c["ld"])
    ak = c["A"] * c["K"]
    return torch.cat([b[:, :, :ak].reshape(-1) for b in bl]), all(bool((b[:, :, ak:] == SENTINEL).all()) for b in bl)


def _run(torch, ops, c, gs=None, mean=False, flat=None, matched=None, gt_labels=None, gt_off=None, denom=None, N=None):
    N = c["N"] if N is None else N
    grad = _grad_buffer(torch, c, N)
    mean_out = torch.full((1,), SENTINEL, device="cuda") if mean else None
    loss = ops.focal_loss_seg((c["flat"] if flat is None else flat).cuda(), c["level_pix"], N, c["A"], c["K"], c["ld"],
                              (c["matched"] if matched is None else matched).cuda().contiguous(), (c["gt_labels"] if gt_labels is None else gt_labels).cuda(),
                              (c["gt_off"] if gt_off is None else gt_off).cuda(), c["denom"] if denom is None else denom, grad=grad,
                              gscale=None if gs is None else torch.tensor(gs, dtype=torch.float32, device="cuda"), mean_out=mean_out)
    return loss, grad, mean_out


@pytest.mark.parametrize("A,K,ld,level_pix", SHAPES)
def test_focal_loss_seg_value_gradient_bits_and_batch_independence(T, A, K, ld, level_pix):
    torch, ops = T
    c = _case(torch, A, K, ld, level_pix, seed=A * 1000 + K + level_pix[0])
    assert c["nfg"][0] == 0 and c["nfg"][1] == 0 and c["nfg"][2] >= 2 and c["denom"][:2] == [1.0, 1.0]
    want, want_grad = _want(torch, c, GS)
    loss, grad, mean = _run(torch, ops, c, GS, mean=True)
    # value and gradient against float64, unequal per-image scales; everything finite; the pad columns untouched
    _each(loss, want, 2e-6, "per-image focal loss")
    gv, intact = _valid(c, grad)
    assert intact, "a pad column of the gradient was written"
    wv, _ = _valid(c, _pad_sentinel(c, want_grad))
    _close(gv, wv, 1e-5, "focal loss gradient")
    for i in (0, 2):                                        # and image by image: the scales gs[n] / denom[n] differ by orders of magnitude
        _close(_valid(c, _alone(grad, c["N"], level_pix, ld, i), N=1)[0], _valid(c, _alone(want_grad, c["N"], level_pix, ld, i), N=1)[0], 1e-5,
               "focal loss gradient of image %d" % i)
    # the image with every anchor ignored: loss exactly 0, its gradient block exactly 0
    assert float(loss[1]) == 0.0 and float(want[1]) == 0.0
    per = [_valid(c, _alone(grad, c["N"], level_pix, ld, i), N=1)[0] for i in range(c["N"])]
    assert float(per[1].abs().max()) == 0.0 and float(per[0].abs().max()) > 0 and float(per[2].abs().max()) > 0
    # mean_out: the float32 left-to-right sum / N
    l = loss.cpu().numpy()
    s = l[0]
    for v in l[1:]:
        s = np.float32(s + v)
    assert mean.cpu().numpy().tobytes() == np.array([s / np.float32(c["N"])], np.float32).tobytes()
    # two runs are bit-identical
    loss2, grad2, mean2 = _run(torch, ops, c, GS, mean=True)
    assert _bits(loss2) == _bits(loss) and _bits(grad2) == _bits(grad) and _bits(mean2) == _bits(mean)
    # a zero scale leaves that image's gradient at zero; a null gscale is 1
    loss0, grad0, _ = _run(torch, ops, c, [1.0, 1.0, 0.0])
    assert _bits(loss0) == _bits(loss)
    assert float(_valid(c, _alone(grad0, c["N"], level_pix, ld, 2), N=1)[0].abs().max()) == 0.0
    loss1, grad1, _ = _run(torch, ops, c, None)
    ones = _run(torch, ops, c, [1.0, 1.0, 1.0])
    assert _bits(loss1) == _bits(ones[0]) and _bits(grad1) == _bits(ones[1])
    # batch independence: each image submitted alone gives the bits of its row in the batch
    for i in range(c["N"]):
        o0, o1 = int(c["gt_off"][i]), int(c["gt_off"][i + 1])
        la, ga, _ = _run(torch, ops, c, [GS[i]], flat=_alone(c["flat"], c["N"], level_pix, ld, i), matched=c["matched"][i:i + 1],
                         gt_labels=c["gt_labels"][o0:o1], gt_off=torch.tensor([0, o1 - o0], dtype=torch.int32), denom=[c["denom"][i]], N=1)
        assert _bits(la) == _bits(loss[i:i + 1]), i
        assert _bits(ga) == _bits(_alone(grad, c["N"], level_pix, ld, i)), i
    # the per-image values times 1 / N, summed, against the batch kernel: both within the project's bound of one float64 value
    img_w = torch.tensor([1.0 / (d * c["N"]) for d in c["denom"]], dtype=torch.float32)
    batch = ops.focal_loss(c["flat"].cuda(), level_pix, c["N"], A, K, ld, c["matched"].cuda(), c["gt_labels"].cuda(), c["gt_off"].cuda(), img_w.cuda())
    w = float(want.sum()) / c["N"]
    assert abs(float(loss.double().sum()) / c["N"] - w) <= 2e-6 * abs(w) and abs(float(batch) - w) <= 2e-6 * abs(w), (float(loss.double().sum()) / c["N"], float(batch), w)


def _pad_sentinel(c, g64):
    g = g64.clone()
    for b in _blocks(g, c["N"], c["level_pix"], c["ld"]):
        b[:, :, c["A"] * c["K"]:] = SENTINEL
    return g


def test_focal_loss_seg_takes_64_images_and_refuses_65_before_any_launch(T):
    torch, ops = T
    c = _case(torch, 1, 2, 4, [3, 1, 1, 1, 1], seed=5, N=64)
    want, _ = _want(torch, c, [1.0] * 64)
    loss, grad, mean = _run(torch, ops, c, [1.0] * 64, mean=True)
    _each(loss, want, 2e-6, "64 images")
    assert _valid(c, grad)[1] and float(mean) != SENTINEL
    c = _case(torch, 1, 2, 4, [3, 1, 1, 1, 1], seed=5, N=65)
    grad = _grad_buffer(torch, c)
    before = _bits(grad)
    mean_out = torch.full((1,), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="65"):
        ops.focal_loss_seg(c["flat"].cuda(), c["level_pix"], 65, 1, 2, 4, c["matched"].cuda(), c["gt_labels"].cuda(), c["gt_off"].cuda(), c["denom"],
                           grad=grad, mean_out=mean_out)
    torch.cuda.synchronize()
    assert _bits(grad) == before and float(mean_out) == SENTINEL
    c = _case(torch, 1, 2, 4, [3, 1, 1, 1, 1], seed=5, N=2)
    with pytest.raises(RuntimeError, match="positive"):
        ops.focal_loss_seg(c["flat"].cuda(), c["level_pix"], 2, 1, 2, 4, c["matched"].cuda(), c["gt_labels"].cuda(), c["gt_off"].cuda(), [1.0, 0.0])


def test_smooth_l1_seg_is_the_per_image_l1_on_the_regression_layout(T):
    """beta = 0 on the regression head's layout (rows of 36 floats, train_core.anchor_slots indices) for the three images of the focal
    test: counts = #fg_n, denoms = max(1, #fg_n); the image without foreground gives loss 0 and no gradient; mean_out as for the focal loss."""
    torch, ops = T
    from cald_amd.train_core import anchor_slots
    level_pix, N = [20, 6, 2, 1, 1], 3
    c = _case(torch, 9, 3, 28, level_pix, seed=21)
    g = torch.Generator().manual_seed(22)
    reg = torch.randn(N * sum(level_pix) * 36, generator=g)
    idx, tgt = [], []
    for i in range(N):
        fg = np.flatnonzero(c["matched"][i].numpy() >= 0)
        row, a = anchor_slots(i, fg, level_pix, 9, 36, N)
        idx.append(row + 4 * a); tgt.append(torch.randn(len(fg), 4, generator=g))
    idx = torch.from_numpy(np.concatenate(idx).astype(np.int64)); tgt = torch.cat(tgt)
    rd = reg.double().requires_grad_(True)
    want, o = [], 0
    for i in range(N):
        n = c["nfg"][i]
        sel = torch.stack([rd[idx[o:o + n] + j] for j in range(4)], dim=1) if n else rd.new_zeros(0, 4)
        want.append((sel - tgt[o:o + n].double()).abs().sum() / c["denom"][i]); o += n
    want = torch.stack(want)
    (want * torch.tensor(GS, dtype=torch.float64)).sum().backward()
    grad = torch.zeros_like(reg, device="cuda")
    mean_out = torch.full((1,), SENTINEL, device="cuda")
    loss = ops.smooth_l1_seg(reg.cuda(), idx.cuda(), tgt.cuda().contiguous(), 0.0, c["nfg"], c["denom"], grad=grad,
                             gscale=torch.tensor(GS, device="cuda"), mean_out=mean_out)
    _each(loss, want, 1e-5, "per-image L1"); _close(grad, rd.grad, 1e-5, "per-image L1 gradient")
    assert float(loss[0]) == 0.0 and float(loss[1]) == 0.0 and float(loss[2]) > 0
    lv = [b for b in _blocks(grad, N, level_pix, 36)]
    assert all(float(b[:2].abs().max()) == 0.0 for b in lv), "images without foreground receive no gradient"
    l = loss.cpu().numpy()
    assert mean_out.cpu().numpy().tobytes() == np.array([np.float32(np.float32(l[0] + l[1]) + l[2]) / np.float32(3)], np.float32).tobytes()
    assert _bits(ops.seg_mean(loss)) == _bits(mean_out)


def test_both_kernels_on_the_executed_reference(T, fx):
    """Fixture (a) -- detection/retina_ll.py's two compute_loss as executed -- through focal_loss_seg and smooth_l1_seg: 2e-6 of the float64
    recording, 1e-5 of the float32 one, per image and for the means."""
    torch, ops = T
    from cald_amd.train_core import anchor_slots
    from oracle import torch_train as tt
    for cse in range(len(fx["a_names"])):
        K, level_pix, N = int(fx["a%d_K" % cse]), [int(v) for v in fx["a%d_level_pix" % cse]], int(fx["a%d_N" % cse])
        ld = (9 * K + 3) // 4 * 4
        logits, reg, anchors, matched = [fx["a%d_%s" % (cse, k)] for k in ("cls_logits", "bbox_regression", "anchors", "matched")]
        flat = torch.full((N * sum(level_pix) * ld,), float("nan")); rflat = torch.zeros(N * sum(level_pix) * 36)
        o = 0
        for b, rb in zip(_blocks(flat, N, level_pix, ld), _blocks(rflat, N, level_pix, 36)):
            n = b.shape[1] * 9
            b[:, :, :9 * K] = torch.from_numpy(logits[:, o:o + n]).reshape(N, b.shape[1], 9 * K)
            rb[:] = torch.from_numpy(reg[:, o:o + n]).reshape(N, b.shape[1], 36); o += n
        n_gt = [len(fx["a%d_gt%d" % (cse, n)]) for n in range(N)]
        gt_off = np.cumsum([0] + n_gt)
        gt_labels = torch.from_numpy(np.concatenate([fx["a%d_labels%d" % (cse, n)] for n in range(N)]))
        nfg = [int((matched[n] >= 0).sum()) for n in range(N)]
        den = [float(max(1, n)) for n in nfg]
        means = torch.empty(2, device="cuda")
        cl = ops.focal_loss_seg(flat.cuda(), level_pix, N, 9, K, ld, torch.from_numpy(matched.astype(np.int32)).cuda(), gt_labels.cuda(),
                                torch.from_numpy(gt_off.astype(np.int32)).cuda(), den, mean_out=means[0:1])
        idx, tgt = [], []
        for n in range(N):
            fg = np.flatnonzero(matched[n] >= 0)
            row, a = anchor_slots(n, fg, level_pix, 9, 36, N)
            idx.append(row + 4 * a)
            tgt.append(tt.encode(torch.from_numpy(fx["a%d_gt%d" % (cse, n)][matched[n][fg]]).double(), torch.from_numpy(anchors[fg]).double(), (1.0, 1.0, 1.0, 1.0)).float())
        rl = ops.smooth_l1_seg(rflat.cuda(), torch.from_numpy(np.concatenate(idx).astype(np.int64)).cuda(), torch.cat(tgt).cuda().contiguous(), 0.0, nfg, den,
                               mean_out=means[1:2])
        for got, key in ((cl, "cls"), (rl, "reg"), (means[0:1], "cls_mean"), (means[1:2], "reg_mean")):
            got = got.double().cpu().numpy()
            w64 = np.atleast_1d(fx["a%d_%s_f64" % (cse, key)]); w32 = np.atleast_1d(fx["a%d_%s_f32" % (cse, key)])
            print(cse, key, got, w64)
            assert np.all(np.abs(got - w64) <= 2e-6 * np.maximum(np.abs(w64), 1e-3)), (cse, key, got, w64)
            assert np.all(np.abs(got - w32) <= 1e-5 * np.maximum(np.abs(w32), 1e-3)), (cse, key, got, w32)


def test_train_gap_on_p3_to_p6_carries_the_sweeps_bits(T):
    """The four maps RetinaNetLLTrainer pools at the 160 x 256 batch (the last one 3 x 4): each image's vector equals cald_op_gap on its own
    map, bit for bit, as test_gpu_ll_train.py checks for P2..P5."""
    torch, ops = T
    from cald_amd import _ffi, detector
    ctx, L = detector.get_ctx(0), _ffi.lib()
    rs = np.random.RandomState(9)
    maps = [(rs.randn(2, h, w, 256) + 0.7).astype(np.float32) for h, w in ((20, 32), (10, 16), (5, 8), (3, 4))]
    got = ops.train_gap([torch.from_numpy(m).cuda() for m in maps]).cpu().numpy()
    for l, m in enumerate(maps):
        for n in range(2):
            want = np.full(256, np.nan, np.float32)
            _ffi.check(L.cald_op_gap(ctx, _ffi.ptr(np.ascontiguousarray(m[n])), m.shape[1], m.shape[2], 256, _ffi.ptr(want)))
            assert got[n, l].tobytes() == want.tobytes(), (l, n)
