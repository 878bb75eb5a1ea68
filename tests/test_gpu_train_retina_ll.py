"""GPU tests that build a RetinaNetLLTrainer: whole batch-4 steps against the float64 restatement (tests/_retina_ll_restatement.py, pinned
to the executed reference by tests/test_retina_ll_train.py) on the same matches and ReLU decisions, the autograd bridge under the reference's
own loop lines, the epoch loop on the reference run's recorded inputs, the plain trainer's unchanged bits and the round trip through the
sweep.  The operator-level tests are in tests/test_gpu_retina_ll_ops.py.  Tolerances are test_gpu_train.py's: whole-step losses 1e-4 *
max(1, |w|), whole-step gradients 1e-4 of each tensor's largest entry, operators 1e-5.  Like every file that builds a trainer, this one sorts
behind test_gpu_parity.py (test_gpu_train_ll_step.py's docstring says why)."""
import numpy as np
import pytest

import _retina_ll_restatement as R

pytestmark = pytest.mark.gpu

SIZES = dict(min_size=160, max_size=256)


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


def _train_case(torch, n_images=4, seed=6, scale=0.4):
    from cald_amd import synth
    sd = synth.pseudo_trained_retinanet(21, 50, seed=2)
    imgs = synth.make_pool(n_images, "voc", seed, scale=scale)
    images = [torch.from_numpy(im).permute(2, 0, 1).float().div(255) for im in imgs]
    rs = np.random.RandomState(seed + 1)
    targets = []
    for im in imgs:
        H, W = im.shape[:2]
        k = 2 + rs.randint(0, 3)
        x0 = rs.rand(k) * W * 0.6; y0 = rs.rand(k) * H * 0.6
        bw = W * (0.15 + 0.3 * rs.rand(k)); bh = H * (0.15 + 0.3 * rs.rand(k))
        boxes = np.stack([x0, y0, np.minimum(x0 + bw, W - 1), np.minimum(y0 + bh, H - 1)], axis=1).astype(np.float32)
        targets.append({"boxes": torch.from_numpy(boxes), "labels": torch.from_numpy(rs.randint(1, 21, k).astype(np.int64))})
    return sd, imgs, images, targets


@pytest.fixture(scope="module")
def step(T, golden, oracle):
    """ONE forward of RetinaNetLLTrainer at batch 4, LossNet and LossPredLoss on top, the three backward passes of the cases below, and the
    float64 restatement of the same step (same matches and ReLU decisions -- LossNet's four included; hinge and sign decisions at least
    1e-4 from flipping).  Computed once, read by the tests."""
    torch, ops = T
    from cald_amd import ll_train, train
    fxl = golden("lossnet_train")
    sd, imgs, images, targets = _train_case(torch)
    N = len(images)
    net = train.RetinaNetLLTrainer(sd, 21, **SIZES)
    ll = ll_train.LossNet(state_dict={k: torch.from_numpy(fxl["net128_sd_" + k]) for k in _keys()})
    losses, pooled = net.forward(images, targets)
    assert list(losses) == list(R.LOSS_NAMES) and all(tuple(v.shape) == (N,) for v in losses.values()) and tuple(pooled.shape) == (N, 4, 256)
    assert [tuple(p.shape[1:3]) for p in net.last["P"][:4]] == [(20, 32), (10, 16), (5, 8), (3, 4)]
    assert net.last["nfg"] == [int((m >= 0).sum()) for m in net.last["matched_host"]] and min(net.last["nfg"]) >= 1
    target = sum(losses.values())                                   # float32, left to right from 0: classification, bbox_regression
    pred, hidden = ops.lossnet_fwd(ll._plist, pooled, ll.D)
    ll_loss, _, g_pred = ops.loss_pred_loss(pred, target, 1.0)
    g_pooled = ops.lossnet_bwd(ll._plist, ll._glist, pooled, hidden, g_pred, need_g_pooled=True)
    got = dict(losses={k: v.cpu() for k, v in losses.items()}, means={k: v.cpu() for k, v in net.last["means"].items()}, ll_loss=float(ll_loss),
               ll_grads={k: ll.grads[k].clone().cpu() for k in _keys()}, target=target.cpu(), pred=pred.cpu())
    mean = [[1.0 / N] * N] * 2
    got["detached"] = {k: v.clone().cpu() for k, v in net.backward(mean).items()}
    got["pooled_only"] = {k: v.clone().cpu() for k, v in net.backward([[0.0] * N] * 2, g_pooled=g_pooled).items()}
    got["live"] = {k: v.clone().cpu() for k, v in net.backward(mean, g_pooled=g_pooled).items()}
    # ---- float64 ----
    ref = R.TorchTrainRetinaNetLL(sd, 21, **SIZES)
    ref.masks = net.relu_decisions()
    want, rec = ref.losses_ll(images, targets, matched=[torch.from_numpy(m.astype(np.int64)) for m in net.last["matched_host"]])
    own = [R.tt.matcher(R.tt.box_iou(g, rec["anchors"]), 0.5, 0.4, True) for g in ref.batch(images, targets)[1]]
    assert torch.equal(torch.stack(own), rec["matched"]), "the kernel's anchor matching is the restatement's"
    lsd = {k: R.f64(fxl["net128_sd_" + k]).requires_grad_(True) for k in _keys()}
    rpred, _ = R.lossnet(lsd, R.pooled_of(rec["P"][:4]), relu_masks=(hidden > 0).cpu())
    rll = R.loss_pred_loss(rpred, sum(want[k] for k in R.LOSS_NAMES).detach(), 1.0, guard=1e-4)
    tr = ref.trainable()
    names = list(tr)
    g_task = torch.autograd.grad(sum(rec["means"][k] for k in R.LOSS_NAMES), [tr[k] for k in names], retain_graph=True)
    g_ll = torch.autograd.grad(rll, [tr[k] for k in names] + [lsd[k] for k in _keys()], allow_unused=True)
    zero = lambda k, g: torch.zeros_like(tr[k]) if g is None else g
    want_d = dict(losses={k: v.detach() for k, v in want.items()}, means={k: v.detach() for k, v in rec["means"].items()}, ll_loss=float(rll.detach()),
                  ll_grads=dict(zip(_keys(), g_ll[len(names):])), detached=dict(zip(names, g_task)),
                  pooled_only={k: zero(k, g) for k, g in zip(names, g_ll[:len(names)])})
    want_d["live"] = {k: want_d["detached"][k] + want_d["pooled_only"][k] for k in names}       # the gradient of a sum
    return dict(got=got, want=want_d, net=net, ll=ll, sd=sd, imgs=imgs, images=images, targets=targets, g_pooled=g_pooled)


def _grads_close(got, want, what, tol=1e-4):
    assert sorted(got) == sorted(want) and len(got) == 78
    worst = ("", 0.0)
    for k, g in got.items():
        w = want[k]
        scale = float(w.abs().max())
        if scale == 0.0:                                   # a tensor this loss does not reach
            assert float(g.abs().max()) == 0.0, (what, k)
            continue
        err = float((g.double() - w).abs().max()) / scale
        if err > worst[1]:
            worst = (k, err)
    print("%s: largest gradient error %.3g at %s" % (what, worst[1], worst[0]))
    assert worst[1] <= tol, "%s: largest gradient error %.3g at %s" % (what, worst[1], worst[0])


def test_step_detached_losses_ll_loss_and_gradients(step):
    got, want = step["got"], step["want"]
    for k in R.LOSS_NAMES:
        for i, (g, w) in enumerate(zip(got["losses"][k].tolist(), want["losses"][k].tolist())):
            assert abs(g - w) <= 1e-4 * max(1.0, abs(w)), (k, i, g, w)
        g, w = float(got["means"][k]), float(want["means"][k])
        assert abs(g - w) <= 1e-4 * max(1.0, abs(w)), (k, "mean", g, w)
    assert abs(got["ll_loss"] - want["ll_loss"]) <= 1e-4 * max(1.0, abs(want["ll_loss"])), (got["ll_loss"], want["ll_loss"])
    assert want["ll_loss"] > 0, "at least one pair is inside the margin: LossNet receives a gradient"
    assert sorted(got["ll_grads"]) == sorted(want["ll_grads"])
    for k in _keys():
        _close(got["ll_grads"][k], want["ll_grads"][k], 1e-4, "LossNet " + k)
    _grads_close(got["detached"], want["detached"], "detector, features detached")


def test_step_gradient_through_the_pooled_features_only(step):
    """Both task gscales are zero: the detector's gradients arrive ONLY through g_pooled and the broadcast join into P3..P6."""
    got, want = step["got"]["pooled_only"], step["want"]["pooled_only"]
    for k, g in got.items():
        if k.startswith("head.") or k.startswith("backbone.fpn.extra_blocks.p7."):
            assert float(g.abs().max()) == 0.0 and float(want[k].abs().max()) == 0.0, k      # the heads and P7 are not upstream of the pooled maps
    for k in ("backbone.fpn.extra_blocks.p6.weight", "backbone.fpn.extra_blocks.p6.bias", "backbone.fpn.layer_blocks.0.weight",
              "backbone.fpn.inner_blocks.2.weight", "backbone.body.layer2.0.conv1.weight"):
        assert float(got[k].abs().max()) > 0, k
    _grads_close(got, want, "detector, through g_pooled only")


def test_step_live_features_full_loss(step):
    _grads_close(step["got"]["live"], step["want"]["live"], "detector, live features")
    assert any(_bits(step["got"]["live"][k]) != _bits(step["got"]["detached"][k]) for k in step["got"]["live"])


def test_detached_gradients_agree_with_the_plain_trainer_which_is_unchanged(T, step):
    """A plain RetinaNetTrainer on the same batch: its losses are the per-image losses' means, its backward() agrees with the detached
    per-image backward (gscale 1 / N) to 2e-4 of each tensor's largest entry -- both are within 1e-4 of one float64 gradient -- and it
    returns the same bits before and after a RetinaNetLLTrainer ran in the process."""
    torch, ops = T
    from cald_amd import train

    def plain():
        net = train.RetinaNetTrainer(step["sd"], 21, **SIZES)
        losses = net.forward(step["images"], step["targets"])
        assert all(v.numel() == 1 for v in losses.values()) and "means" not in net.last and "pooled" not in net.last
        grads = {k: v.clone().cpu() for k, v in net.backward().items()}
        return {k: v.cpu() for k, v in losses.items()}, grads
    l0, g0 = plain()
    net = train.RetinaNetLLTrainer(step["sd"], 21, **SIZES)
    _, pooled = net.forward(step["images"], step["targets"])
    net.backward([[0.25] * 4] * 2, g_pooled=torch.ones_like(pooled))
    l1, g1 = plain()
    assert all(_bits(l0[k]) == _bits(l1[k]) for k in l0) and all(_bits(g0[k]) == _bits(g1[k]) for k in g0)
    for k in R.LOSS_NAMES:
        w = float(step["want"]["means"][k])
        assert abs(float(l0[k]) - w) <= 1e-4 * max(1.0, abs(w)) and abs(float(step["got"]["means"][k]) - float(l0[k])) <= 2e-4 * max(1.0, abs(w))
    _grads_close(step["got"]["detached"], {k: v.double() for k, v in g0.items()}, "detached per-image backward against the plain trainer", tol=2e-4)
    _grads_close(g0, step["want"]["detached"], "plain trainer against float64")


def test_the_references_loop_lines_run_on_the_trainable_detector(T, step):
    """ll_train.py:98-123 typed out against train.TrainableDetector over a RetinaNetLLTrainer, features live (epoch < task_epochs) and
    detached: the lines run as they stand, and the gradients are those of the step fixture's direct backward() calls."""
    torch, ops = T
    from cald_amd import ll_train, train
    net = train.RetinaNetLLTrainer(step["sd"], 21, **SIZES)
    task_model = train.TrainableDetector(net)
    for epoch, task_epochs, mode in ((0, 2, "live"), (2, 2, "detached")):
        ll_model = ll_train.LossNet(state_dict=step["ll"].state_dict())
        features, task_loss_dict = task_model(step["images"], step["targets"])
        assert isinstance(features, list) and len(features) == 4 and all(tuple(f.shape) == (4, 256) for f in features)
        assert all(isinstance(v, tuple) and v[0].dim() == 0 and len(v[1]) == 4 and v[1][0].dim() == 0 for v in task_loss_dict.values())
        _task_losses = sum(torch.stack(loss[1]) for loss in task_loss_dict.values())
        task_loss_dict['classification'] = task_loss_dict['classification'][0]
        task_loss_dict['bbox_regression'] = task_loss_dict['bbox_regression'][0]
        task_losses = sum(loss for loss in task_loss_dict.values())
        if epoch >= task_epochs:
            _features = dict()
            _features['0'] = features[0].detach()
            _features['1'] = features[1].detach()
            _features['2'] = features[2].detach()
            _features['3'] = features[3].detach()
        else:
            _features = dict()
            _features['0'] = features[0]
            _features['1'] = features[1]
            _features['2'] = features[2]
            _features['3'] = features[3]
        ll_pred = ll_model(_features).cuda()
        ll_pred = ll_pred.view(ll_pred.size(0))
        ll_loss = 1.0 * ll_train.LossPredLoss(ll_pred, _task_losses, margin=1.0)
        losses = task_losses + ll_loss
        losses.backward()
        assert _bits(_task_losses) == _bits(step["got"]["target"]) and _bits(ll_pred) == _bits(step["got"]["pred"])
        assert abs(float(ll_loss.detach()) - step["want"]["ll_loss"]) <= 1e-4 * max(1.0, step["want"]["ll_loss"])
        for k in R.LOSS_NAMES:
            assert _bits(task_loss_dict[k]) == _bits(step["got"]["means"][k])
        got = {k: v.clone().cpu() for k, v in net.grads.items()}
        bit_equal = all(_bits(got[k]) == _bits(step["got"][mode][k]) for k in got)
        print("%s: gradients through the autograd bridge %s the direct backward's" % (mode, "bit-equal" if bit_equal else "NOT bit-equal"))
        _grads_close(got, {k: v.double() for k, v in step["got"][mode].items()}, "bridge, %s" % mode, tol=1e-6)
        _grads_close(got, step["want"][mode], "bridge against float64, %s" % mode)
        for k in _keys():
            _close(ll_model.params[k].grad, step["want"]["ll_grads"][k], 1e-4, "LossNet through the bridge " + k)
        for p in net.parameters():
            p.grad = None


def test_train_one_epoch_on_the_reference_runs_recorded_inputs(T, fx):
    """Three iterations of ll_train.train_one_epoch (epoch 0) on fixture (b)'s recorded maps and losses, fed through a stub task model with
    retina_ll.py's returns (a five-element feature list, (mean, [per image]) tuples): LossNet's parameters after every iteration, ll_loss
    and both learning rates match the executed reference; with task_epochs = 5 the pooled features receive its gradient, with 0 none."""
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
                out = {}
                for k in R.LOSS_NAMES:                      # the recorded values, with a parameter in the graph
                    per = list((torch.from_numpy(fx["ep%d_loss_%d_%s" % (Tk, it, k)]).cuda() * (theta / theta.detach())).unbind(0))
                    out[k] = (sum(per) / len(per), per)
                    assert _bits(out[k][0]) == fx["ep%d_mean_%d_%s" % (Tk, it, k)].tobytes()
                return [pooled[:, l, :] for l in range(4)] + [torch.zeros(4, 256, device="cuda")], out

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


def _two_sgd_steps(torch, step, task_epochs):
    from cald_amd import ll_train, train
    net = train.RetinaNetLLTrainer(step["sd"], 21, **SIZES)
    model = train.TrainableDetector(net)
    ll = ll_train.LossNet(state_dict=step["ll"].state_dict())
    task_opt = train.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, net=net)
    ll_opt = train.SGD(ll.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, net=ll)
    batch = (step["images"], step["targets"])
    hist = ll_train.train_one_epoch(model, task_opt, ll, ll_opt, [batch, batch], "cuda", 0, 1, 0, task_epochs=task_epochs)
    assert task_opt._mflat is not None and ll_opt._mflat is not None, "both optimizers ran as one fused launch"
    return net, model, ll, hist


def test_two_sgd_steps_are_finite_reproducible_and_scored_by_the_sweep(T, step):
    """Two drop-in iterations (live features, both HIP optimizers), twice from the same state: finite, one task loss per step, bit-identical.
    Then the round trip: the trained LossNet.state_dict() and the trained detector go into baselines.ll_get_uncertainty with the step's four
    images as one loader batch and levels (0, 1, 2, 3) -- the sweep's scores against the training forward's ll_pred, relative to the largest
    score (the two forwards are not bit-equal: 1e-4 is a structural bound, the observed value is printed -- 1.7e-6 when this was written,
    7e-7 for the Faster R-CNN twin); the default levels (the
    reference's features[0] four times) still run."""
    torch, ops = T
    from cald_amd import baselines, detector
    net, model, ll, hist = _two_sgd_steps(torch, step, 2)
    assert len(hist) == 2 and all(np.isfinite(h["task_loss"]) and np.isfinite(h["ll_loss"]) for h in hist) and hist[0]["ll_loss"] > 0
    assert hist[1]["task_loss"] != hist[0]["task_loss"], "the first step changed the detector"
    assert not torch.equal(step["ll"].state_dict()["FC1.weight"], ll.state_dict()["FC1.weight"])
    assert bool(torch.isfinite(net.flat).all()) and bool(torch.isfinite(ll.flat).all())
    net2, _, ll2, hist2 = _two_sgd_steps(torch, step, 2)
    assert hist2 == hist and _bits(net2.flat) == _bits(net.flat) and _bits(ll2.flat) == _bits(ll.flat)
    with torch.no_grad():
        features, loss_dict = model(step["images"], step["targets"])
        ll_pred = ll({str(k): features[k] for k in range(4)}).view(-1).cpu().numpy()
    det = detector.retinanet_resnet50_fpn_cal(num_classes=21, **SIZES).to("cuda")
    det.load_state_dict(net.state_dict())
    det.eval()
    loader = [([torch.from_numpy(im).cuda() for im in step["imgs"]], [None] * 4)]
    scores = baselines.ll_get_uncertainty(det, ll.state_dict(), loader, levels=(0, 1, 2, 3)).numpy()
    err = float(np.abs(scores - ll_pred).max() / np.abs(ll_pred).max())
    print("round trip: training forward", ll_pred, "sweep", scores, "relative to the largest score %.3g" % err,
          "bit-equal" if scores.tobytes() == ll_pred.tobytes() else "not bit-equal")
    assert err <= 1e-4
    default = baselines.ll_get_uncertainty(det, ll.state_dict(), loader).numpy()
    assert default.shape == (4,) and np.isfinite(default).all()
