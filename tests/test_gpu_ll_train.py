"""GPU tests of the learning-loss TRAINING step (cald_amd/ll_train.py, lossnet_train.hip, cald_train_gap, the segmented loss kernels and
the broadcast join of train_loss.hip / train_elementwise.hip): operators against the executed reference (tests/golden/lossnet_train.npz, frcnn_losses.npz) and the
sweep's operators bit for bit, and the epoch loop on the reference run's recorded inputs.  Tolerance: test_gpu_train.py's operator-level
1e-5 of the reference's largest entry.  The tests that build a FasterRCNNTrainer (whole steps, round trip, unchanged behaviour) are in
tests/test_gpu_train_ll_step.py, which -- like every other file that builds a trainer -- sorts behind test_gpu_parity.py (see its docstring)."""
import numpy as np
import pytest

import _ll_train_restatement as R

pytestmark = pytest.mark.gpu

PIXELS = [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1027]           # test_gpu_ll_sweep.PIXELS


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():      # module-scoped: runs before conftest's function-scoped auto-skip
        pytest.skip("needs an MI355X")
    from cald_amd import train_ops
    return torch, train_ops


@pytest.fixture(scope="module")
def fx(golden):
    return golden("lossnet_train")


def _keys():
    from cald_amd.baselines import LOSSNET_KEYS
    return LOSSNET_KEYS


def _close(got, want, tol, what):
    got = got.detach().double().cpu().numpy() if hasattr(got, "detach") else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if hasattr(want, "detach") else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-30, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    print("%s: max err / max|ref| = %.3g" % (what, err))
    assert err <= tol, "%s: max err / max|ref| = %.3g > %.3g" % (what, err, tol)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


# ---------------------------------------------------------------- 1. segmented losses
def _predictor_rows(torch, R_, Cc, ld, seed, labels=None):
    g = torch.Generator().manual_seed(seed)
    z = torch.zeros(R_, ld); z[:, :5 * Cc] = torch.randn(R_, 5 * Cc, generator=g) * 2
    lab = torch.randint(0, Cc, (R_,), generator=g) if labels is None else labels
    pos = torch.nonzero(lab > 0).squeeze(1)
    tgt = torch.randn(len(pos), 4, generator=g)
    idx = pos * ld + Cc + 4 * lab[pos]
    return z, lab, pos, tgt, idx


def test_one_segment_returns_the_unsegmented_kernels_bits(T):
    torch, ops = T
    Rr, Cc, ld = 300, 21, 108
    z, lab, pos, tgt, idx = _predictor_rows(torch, Rr, Cc, ld, 6)
    zc, labc, idxc, tgtc = z.cuda(), lab.cuda(), idx.cuda(), tgt.cuda().contiguous()
    gs = torch.tensor([0.7], device="cuda")
    g0, g1 = torch.zeros_like(zc), torch.zeros_like(zc)
    a = ops.softmax_ce(zc, labc, Cc, grad=g0, gscale=0.7); b = ops.softmax_ce_seg(zc, labc, Cc, [Rr], grad=g1, gscale=gs)
    assert _bits(a) == _bits(b) and _bits(g0) == _bits(g1)
    for beta in (1.0, 1.0 / 9, 0.0):
        g0.zero_(); g1.zero_()
        a = ops.smooth_l1(zc, idxc, tgtc, beta, Rr, grad=g0, gscale=0.7)
        b = ops.smooth_l1_seg(zc, idxc, tgtc, beta, [len(pos)], [Rr], grad=g1, gscale=gs)
        assert _bits(a) == _bits(b) and _bits(g0) == _bits(g1), beta
    g = torch.Generator().manual_seed(7)
    x = torch.randn(5000, generator=g) * 3; sel = torch.randperm(5000, generator=g)[:300]; y = (torch.rand(300, generator=g) < 0.5).float()
    g0, g1 = torch.zeros(5000, device="cuda"), torch.zeros(5000, device="cuda")
    a = ops.bce_logits(x.cuda(), sel.cuda(), y.cuda(), grad=g0, gscale=0.7)
    b = ops.bce_logits_seg(x.cuda(), sel.cuda(), y.cuda(), [300], grad=g1, gscale=gs)
    assert _bits(a) == _bits(b) and _bits(g0) == _bits(g1)
    # no gscale = 1
    assert _bits(ops.bce_logits(x.cuda(), sel.cuda(), y.cuda())) == _bits(ops.bce_logits_seg(x.cuda(), sel.cuda(), y.cuda(), [300]))


def test_three_unequal_segments_against_float64(T):
    """Row counts 5 / 300 / 3 (the block-stride loop runs twice in image 1), image 0 without a positive row (box loss 0, zero gradient),
    C = 21 in rows of stride 108, unequal gscale per image."""
    torch, ops = T
    import torch.nn.functional as F
    counts, Cc, ld = [5, 300, 3], 21, 108
    Rr = sum(counts)
    g = torch.Generator().manual_seed(11)
    lab = torch.randint(0, Cc, (Rr,), generator=g); lab[:5] = 0; lab[305:] = torch.tensor([3, 0, 20])
    z, lab, pos, tgt, idx = _predictor_rows(torch, Rr, Cc, ld, 12, labels=lab)
    gs = [0.7, 1.3, 0.4]
    zd = z.double().requires_grad_(True)
    full_tgt = torch.zeros(Rr, 4, dtype=torch.float64); full_tgt[pos] = tgt.double()
    cls, box = R.fastrcnn_loss_per_image(zd[:, :Cc], zd[:, Cc:5 * Cc], lab, full_tgt, counts)
    gsd = torch.tensor(gs, dtype=torch.float64)
    ((cls * gsd).sum() + (box * gsd.flip(0)).sum()).backward()
    zc, grad = z.cuda(), torch.zeros(Rr, ld, device="cuda")
    pos_cnt = [int((lab[a:b] > 0).sum()) for a, b in zip(np.cumsum([0] + counts)[:-1], np.cumsum(counts))]
    assert pos_cnt[0] == 0 and pos_cnt[1] > 0
    l1 = ops.softmax_ce_seg(zc, lab.cuda(), Cc, counts, grad=grad, gscale=torch.tensor(gs, device="cuda"))
    l2 = ops.smooth_l1_seg(zc, idx.cuda(), tgt.cuda().contiguous(), 1.0, pos_cnt, counts, grad=grad, gscale=torch.tensor(gs[::-1], device="cuda"))
    _close(l1, cls, 1e-5, "per-image cross entropy"); _close(l2, box, 1e-5, "per-image box loss")
    assert float(l2[0]) == 0.0 and torch.isfinite(grad).all()
    _close(grad, zd.grad, 1e-5, "d / d predictor rows")
    assert float(grad[:5, Cc:].abs().max()) == 0.0, "an image without positives leaves the box deltas' gradient at zero"
    # RPN layout: [A][1 logit + 4 deltas], per image its sampled positives then negatives
    A = 4000
    head = torch.randn(A, 5, generator=g) * 2
    tg = torch.randn(A, 4, generator=g)
    obj_idx, box_idx, labs, tsel, n_obj, n_pos, want_o, want_b = [], [], [], [], [], [], [], []
    hd = head.double().requires_grad_(True)
    for i, (npos, nneg) in enumerate([(0, 5), (128, 172), (2, 1)]):
        perm = torch.randperm(A, generator=g)
        p, n = perm[:npos].sort().values, perm[npos:npos + nneg].sort().values
        o, b = R.rpn_loss_per_image(hd[:, 0], hd[:, 1:], tg.double(), p, n)
        want_o.append(o); want_b.append(b)
        obj_idx += [p * 5, n * 5]; box_idx.append(p * 5 + 1); tsel.append(tg[p]); labs += [torch.ones(npos), torch.zeros(nneg)]
        n_obj.append(npos + nneg); n_pos.append(npos)
    want_o, want_b = torch.stack(want_o), torch.stack(want_b)
    ((want_o * gsd).sum() + (want_b * gsd.flip(0)).sum()).backward()
    hc, gh = head.cuda().contiguous(), torch.zeros(A, 5, device="cuda")
    lo = ops.bce_logits_seg(hc, torch.cat(obj_idx).cuda(), torch.cat(labs).cuda(), n_obj, grad=gh, gscale=torch.tensor(gs, device="cuda"))
    lb = ops.smooth_l1_seg(hc, torch.cat(box_idx).cuda(), torch.cat(tsel).cuda().contiguous(), 0.0, n_pos, n_obj, grad=gh,
                           gscale=torch.tensor(gs[::-1], device="cuda"))
    _close(lo, want_o, 1e-5, "per-image objectness"); _close(lb, want_b, 1e-5, "per-image RPN box loss")
    assert float(lb[0]) == 0.0
    _close(gh, hd.grad, 1e-5, "d / d RPN head")


def test_segmented_kernels_on_the_reference_copies_single_image_cases(T, golden):
    """detection/frcnn_ll.py's own per-image losses as executed (tests/golden/frcnn_losses.npz, read only), through the segmented kernels
    with one segment: 2e-6 of the float64 run, 1e-5 of the float32 run (the bounds of the unsegmented kernels' test)."""
    torch, ops = T
    g = golden("frcnn_losses")

    def close(got, key):
        w64, w32 = float(g[key + "_f64"]), float(g[key + "_f32"])
        assert abs(float(got) - w64) <= 2e-6 * max(abs(w64), 1e-3), (key, float(got), w64)
        assert abs(float(got) - w32) <= 1e-5 * max(abs(w32), 1e-3), (key, float(got), w32)
    for k in range(int(g["b_n"])):
        logits, deltas, labels, tgt = g["b%d_logits" % k], g["b%d_deltas" % k], g["b%d_labels" % k], g["b%d_targets" % k]
        Rr, Cc = logits.shape
        pred = torch.from_numpy(np.concatenate([logits, deltas], axis=1)).cuda().contiguous()
        ld = pred.shape[1]
        close(ops.softmax_ce_seg(pred, torch.from_numpy(labels).cuda(), Cc, [Rr]), "b%d_cls" % k)
        pos = np.flatnonzero(labels > 0)
        idx = torch.from_numpy((pos * ld + Cc + 4 * labels[pos]).astype(np.int64)).cuda()
        tg = torch.from_numpy(tgt[pos].reshape(-1, 4)).cuda().contiguous()
        close(ops.smooth_l1_seg(pred, idx, tg, 1.0, [len(pos)], [Rr]), "b%d_box" % k)          # also the cases without a positive row
    for k in range(int(g["r_n"])):
        obj, deltas, tgt, pos, neg = g["r%d_obj" % k], g["r%d_deltas" % k], g["r%d_targets" % k], g["r%d_pos" % k], g["r%d_neg" % k]
        head = torch.from_numpy(np.concatenate([obj, deltas], axis=1)).cuda().contiguous()
        samp = np.concatenate([pos, neg])
        lab = torch.from_numpy(np.concatenate([np.ones(len(pos), np.float32), np.zeros(len(neg), np.float32)])).cuda()
        close(ops.bce_logits_seg(head, torch.from_numpy((samp * 5).astype(np.int64)).cuda(), lab, [len(samp)]), "r%d_obj" % k)
        tg = torch.from_numpy(tgt[pos].reshape(-1, 4)).cuda().contiguous()
        close(ops.smooth_l1_seg(head, torch.from_numpy((pos * 5 + 1).astype(np.int64)).cuda(), tg, 0.0, [len(pos)], [len(samp)]), "r%d_box" % k)


# ---------------------------------------------------------------- 2. pooling in the training forward
def test_train_gap_carries_the_sweeps_bits(T):
    """N = 2 images; the four level slots take every pixel count of the sweep's pooling test in turn.  Each image's vector equals cald_op_gap
    on its own map, bit for bit."""
    torch, ops = T
    from cald_amd import _ffi, detector
    ctx, L = detector.get_ctx(0), _ffi.lib()
    rs = np.random.RandomState(5)
    shapes = [(1, n) if i % 2 else (n, 1) for i, n in enumerate(PIXELS)]
    shapes[-1] = (13, 79)                                           # 1027 pixels as a 2-D map
    for at in range(0, len(shapes), 4):
        maps = [(rs.randn(2, h, w, 256) + 0.7).astype(np.float32) for h, w in shapes[at:at + 4]]
        got = ops.train_gap([torch.from_numpy(m).cuda() for m in maps]).cpu().numpy()
        for l, m in enumerate(maps):
            for n in range(2):
                want = np.full(256, np.nan, np.float32)
                _ffi.check(L.cald_op_gap(ctx, _ffi.ptr(np.ascontiguousarray(m[n])), m.shape[1], m.shape[2], 256, _ffi.ptr(want)))
                assert got[n, l].tobytes() == want.tobytes(), (shapes[at + l], n)


# ---------------------------------------------------------------- 3. LossNet forward / backward, LossPredLoss
def _net_case(torch, fx, D):
    sd = {k: torch.from_numpy(fx["net%d_sd_%s" % (D, k)]) for k in _keys()}
    pooled = torch.stack([torch.from_numpy(fx["net_feat%d" % i]).double().mean(dim=(2, 3)) for i in range(4)], dim=1).float()
    return sd, pooled.cuda().contiguous()


@pytest.mark.parametrize("D", [1, 100, 128])
def test_lossnet_forward_equals_the_sweeps_scoring_bit_for_bit(T, D):
    torch, ops = T
    from cald_amd import baselines, ll_train
    net = ll_train.LossNet(interm_dim=D)
    rs = np.random.RandomState(D)
    for B in (2, 4, 6):
        pooled = (rs.randn(B, 4, 256) * 0.8 + 0.3).astype(np.float32)
        pred, hidden = ops.lossnet_fwd(net._plist, torch.from_numpy(pooled).cuda(), D)
        want = baselines.lossnet_scores(net, pooled)
        assert pred.cpu().numpy().tobytes() == want.tobytes(), (D, B)
        assert tuple(hidden.shape) == (B, 4, D) and float(hidden.min()) >= 0.0
        out = net({str(k): torch.from_numpy(pooled[:, k]).cuda() for k in range(4)})
        assert tuple(out.shape) == (B, 1) and _bits(out.view(-1)) == want.tobytes()


@pytest.mark.parametrize("D", [128, 1])
def test_lossnet_forward_and_backward_against_the_executed_reference(T, fx, D):
    torch, ops = T
    from cald_amd import ll_train
    sd, pooled = _net_case(torch, fx, D)
    net = ll_train.LossNet(state_dict=sd)
    pred, hidden = ops.lossnet_fwd(net._plist, pooled, D)
    _close(pred, fx["net%d_out" % D], 1e-5, "LossNet output")
    g_pred = torch.from_numpy(fx["net%d_g_pred" % D]).cuda()
    gp = ops.lossnet_bwd(net._plist, net._glist, pooled, hidden, g_pred, need_g_pooled=True)
    first = {k: net.grads[k].clone() for k in _keys()}
    for k in _keys():
        _close(first[k], fx["net%d_grad_%s" % (D, k)], 1e-5, "gradient of " + k)
    for l in range(4):
        gmap = fx["net%d_gfeat%d" % (D, l)]
        hw = gmap.shape[2] * gmap.shape[3]
        assert np.abs(gmap - gmap[:, :, :1, :1]).max() == 0.0
        _close(gp[:, l] / hw, gmap[:, :, 0, 0], 1e-5, "gradient of map %d" % l)
    # accumulate doubles; detached features skip g_pooled; two runs are bit-identical
    assert ops.lossnet_bwd(net._plist, net._glist, pooled, hidden, g_pred, accumulate=True) is None
    for k in _keys():
        assert _bits(net.grads[k]) == _bits(first[k] + first[k]), k
    gp2 = ops.lossnet_bwd(net._plist, net._glist, pooled, hidden, g_pred, need_g_pooled=True)
    assert _bits(gp2) == _bits(gp) and all(_bits(net.grads[k]) == _bits(first[k]) for k in _keys())


def test_loss_pred_loss_value_and_exact_gradient(T, fx):
    torch, ops = T
    from cald_amd import ll_train
    for n in [str(n) for n in fx["lpl_names"]]:
        x = torch.from_numpy(fx["lpl_%s_input" % n]).cuda().requires_grad_(True)
        t, m = torch.from_numpy(fx["lpl_%s_target" % n]).cuda(), float(fx["lpl_%s_margin" % n])
        loss = ll_train.LossPredLoss(x, t, margin=m)
        loss.backward()
        want = float(fx["lpl_%s_loss" % n])
        assert abs(float(loss.detach()) - want) <= 1e-6 * max(abs(want), 1e-30) or (want == 0.0 and float(loss.detach()) == 0.0), (n, float(loss.detach()), want)
        np.testing.assert_array_equal(x.grad.cpu().numpy(), fx["lpl_%s_grad" % n], err_msg=n)       # +-1 / (B / 2) or 0, tie and margin included
        terms = ll_train.LossPredLoss(x.detach(), t, margin=m, reduction='none')
        np.testing.assert_allclose(terms.cpu().numpy(), fx["lpl_%s_none" % n], rtol=1e-6, atol=0, err_msg=n)
    # the pair terms' own gradient (reduction='none') under unequal upstream gradients
    x = torch.tensor([1.0, 0.25, 0.5, 0.0], device="cuda", requires_grad=True)
    terms = ll_train.LossPredLoss(x, torch.tensor([2.0, 1.0, 1.0, 1.0], device="cuda"), reduction='none')
    (terms * torch.tensor([3.0, 0.5], device="cuda")).sum().backward()
    assert x.grad.tolist() == [-3.0, 0.5, -0.5, 3.0]
    with pytest.raises(ValueError):
        ll_train.LossPredLoss(torch.zeros(5, device="cuda"), torch.zeros(5, device="cuda"))
    with pytest.raises(RuntimeError, match="not even"):
        ops.loss_pred_loss(torch.zeros(5, device="cuda"), torch.zeros(5, device="cuda"), 1.0)      # CALD_ERR_INVALID, before any launch


# ---------------------------------------------------------------- 4. the broadcast join
@pytest.mark.parametrize("hw,C", [((1, 1), 4), ((15, 17), 4), ((8, 8), 16), ((1, 257), 4), ((1, 3), 256), ((7, 5), 256)])
def test_broadcast_add_is_numpy_float32_bit_for_bit(T, hw, C):
    """float4 counts per image 1, 255, 256, 257 (the last workgroup of an image is full, short by one, or holds one element), 3 pixels x
    256 channels (fewer float4s than one workgroup), and a map with several pixels per workgroup; N = 2 with two different vectors read
    at the stride of a level of pooled [N, 4, C].  The grid is (ceil(float4s of one image / 256), N): it has no cap."""
    torch, ops = T
    rs = np.random.RandomState(hw[0] * 100 + hw[1] + C)
    a, b = [(rs.randn(2, hw[0], hw[1], C)).astype(np.float32) for _ in range(2)]
    g = rs.randn(2, 4, C).astype(np.float32)
    gd = torch.from_numpy(g).cuda()
    for l in (0, 2):
        got = ops.add_bcast(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), gd[:, l, :]).cpu().numpy()
        want = (a + b) + (g[:, l] / np.float32(hw[0] * hw[1]))[:, None, None, :]
        assert want.dtype == np.float32 and got.tobytes() == want.tobytes(), float(np.abs(got - want).max())


# ---------------------------------------------------------------- 5. the epoch loop on recorded inputs
def test_train_one_epoch_on_the_reference_runs_recorded_inputs(T, fx):
    """Three iterations of ll_train.train_one_epoch (epoch 0) on fixture (c)'s recorded maps and losses, fed through a stub task model that
    pools with cald_train_gap: LossNet's parameters after every iteration, ll_loss and both learning rates match the executed reference;
    with task_epochs = 5 the pooled features receive the reference's gradient, with 0 none."""
    torch, ops = T
    from cald_amd import ll_train, train
    for Tk in (0, 5):
        ll = ll_train.LossNet(state_dict={k: torch.from_numpy(fx["ep_sd0_" + k]) for k in _keys()})
        theta = torch.nn.Parameter(torch.ones(1, device="cuda"))
        seen = dict(pooled=[], lr=[], sd=[])

        class StubTask:
            at = 0

            def train(self):
                return self

            def __call__(self, images, targets):
                it, StubTask.at = StubTask.at, StubTask.at + 1
                maps = [torch.from_numpy(fx["ep_feat_%d_%d" % (it, l)]).cuda().permute(0, 2, 3, 1).contiguous() for l in range(4)]
                pooled = ops.train_gap(maps).requires_grad_(True)
                seen["pooled"].append(pooled)
                losses = {k: torch.from_numpy(fx["ep%d_loss_%d_%s" % (Tk, it, k)]).cuda() * (theta / theta.detach()) for k in R.LOSS_NAMES}      # the recorded values, with a parameter in the graph
                return {str(l): pooled[:, l, :] for l in range(4)}, losses

        class Loader:
            def __len__(self):
                return 3

            def __iter__(self):
                for it in range(3):
                    if it:
                        self.snap()
                    yield [torch.zeros(3, 4, 4)] * 4, [{"boxes": torch.zeros(0, 4)}] * 4
                self.snap()

            def snap(self):
                seen["lr"].append((task_opt.param_groups[0]["lr"], ll_opt.param_groups[0]["lr"]))
                seen["sd"].append(ll.state_dict())

        task_opt = torch.optim.SGD([theta], lr=0.01, momentum=0.9, weight_decay=1e-4)
        ll_opt = train.SGD(ll.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, net=ll)
        hist = ll_train.train_one_epoch(StubTask(), task_opt, ll, ll_opt, Loader(), "cuda", 0, 0, 0, task_epochs=Tk)
        assert ll_opt._mflat is not None, "LossNet's SGD ran as one fused launch over the flat buffer"
        for it in range(3):
            for k in _keys():
                _close(seen["sd"][it][k], fx["ep%d_sd_%d_%s" % (Tk, it, k)], 1e-5, "task_epochs %d iteration %d %s" % (Tk, it, k))
            assert abs(hist[it]["ll_loss"] - float(fx["ep%d_ll_loss" % Tk][it])) <= 1e-5 * max(1.0, abs(hist[it]["ll_loss"]))
            for j, name in enumerate(("task_lr", "ll_lr")):
                assert abs(seen["lr"][it][j] - fx["ep%d_lr" % Tk][it][j]) <= 1e-5 * fx["ep%d_lr" % Tk][it][j]
                assert hist[it][name] == seen["lr"][it][j]
            if Tk == 0:
                assert seen["pooled"][it].grad is None
            else:
                for l in range(4):
                    gmap = fx["ep%d_gfeat_%d_%d" % (Tk, it, l)]
                    _close(seen["pooled"][it].grad[:, l] / (gmap.shape[2] * gmap.shape[3]), gmap[:, :, 0, 0], 1e-5, "iteration %d map %d gradient" % (it, l))
