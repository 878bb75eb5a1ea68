"""GPU tests of the learning-loss training step that build a FasterRCNNTrainer: whole batch-4 steps of loss_mode="ll" against the float64
restatement (tests/_ll_train_restatement.py, pinned to the executed reference by tests/test_ll_train.py) on the same sampler draws and ReLU
decisions, the round trip through the sweep, and the plain trainer's unchanged bits.  The operator-level tests are in
tests/test_gpu_ll_train.py.  Tolerances are test_gpu_train.py's: whole-step losses 1e-4 * max(1, |w|), whole-step gradients 1e-4 of each
tensor's largest entry, operators 1e-5.

Why a file of its own: pytest runs the files in name order, and this one sorts behind test_gpu_parity.py like test_gpu_train.py does.
test_gpu_parity.py::test_two_ranks_on_hardware_equal_one_rank starts two fresh processes that share the GPU with the pytest process; when
ANY trainer has run in the pytest process before it (seen with test_gpu_train.py::test_training_step_is_bit_reproducible alone, on code this
feature does not touch), one of the children returned a score off the oracle's in 3 of 5 runs, a different one each time; without a
trainer before it, 0 of 8.  That is an open defect of the sweep under a shared GPU, not of the training step, and it is not hidden by a
wider bound anywhere: the order the suite had before this file existed is kept."""
import numpy as np
import pytest

import _ll_train_restatement as R

pytestmark = pytest.mark.gpu


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


# ---------------------------------------------------------------- whole steps
def _train_case(torch, n_images=4, seed=2, scale=0.4):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=3)
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
def step(T, fx, oracle):
    """ONE ll-mode forward of the small Faster R-CNN configuration of test_gpu_train's whole-step test at batch 4, LossNet and LossPredLoss
    on top, the three backward passes of the cases below, and the float64 restatement of the same step (same proposals, sampler draws,
    ReLU decisions -- LossNet's four included; hinge and sign decisions at least 1e-4 from flipping).  Computed once, read by the tests."""
    torch, ops = T
    from cald_amd import ll_train, train
    sd, imgs, images, targets = _train_case(torch)
    N = len(images)
    net = train.FasterRCNNTrainer(sd, 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(7), loss_mode="ll")
    ll = ll_train.LossNet(state_dict={k: torch.from_numpy(fx["net128_sd_" + k]) for k in _keys()})
    losses, pooled = net.forward(images, targets)
    assert list(losses) == list(R.LOSS_NAMES) and all(tuple(v.shape) == (N,) for v in losses.values()) and tuple(pooled.shape) == (N, 4, 256)
    target = sum(losses.values())                                   # float32, left to right from 0: cls, box, obj, rpn
    pred, hidden = ops.lossnet_fwd(ll._plist, pooled, ll.D)
    ll_loss, _, g_pred = ops.loss_pred_loss(pred, target, 1.0)
    g_pooled = ops.lossnet_bwd(ll._plist, ll._glist, pooled, hidden, g_pred, need_g_pooled=True)
    got = dict(losses={k: v.cpu() for k, v in losses.items()}, ll_loss=float(ll_loss), ll_grads={k: ll.grads[k].clone().cpu() for k in _keys()})
    mean = [[1.0 / N] * N] * 4
    got["detached"] = {k: v.clone().cpu() for k, v in net.backward(mean).items()}
    got["pooled_only"] = {k: v.clone().cpu() for k, v in net.backward([[0.0] * N] * 4, g_pooled=g_pooled).items()}
    got["live"] = {k: v.clone().cpu() for k, v in net.backward(mean, g_pooled=g_pooled).items()}
    # ---- float64 ----
    ref = R.TorchTrainFRCNNLL(sd, 21, min_size=160, max_size=256)
    ref.masks = net.relu_decisions()
    want, rec = ref.losses_ll(images, targets, [p.cpu() for p in net.last["proposals"]], cfg=dict(box_batch=64), samples=net.last["samples"])
    assert torch.equal(rec["roi_labels"], net.last["roi_labels"]), "same sampled RoIs"
    lsd = {k: R.f64(fx["net128_sd_" + k]).requires_grad_(True) for k in _keys()}
    rpred, _ = R.lossnet(lsd, R.pooled_of(rec["P"][:4]), relu_masks=(hidden > 0).cpu())
    rll = R.loss_pred_loss(rpred, sum(want[k] for k in R.LOSS_NAMES).detach(), 1.0, guard=1e-4)
    tr = ref.trainable()
    names = list(tr)
    g_task = torch.autograd.grad(sum(want[k].mean() for k in R.LOSS_NAMES), [tr[k] for k in names], retain_graph=True)
    g_ll = torch.autograd.grad(rll, [tr[k] for k in names] + [lsd[k] for k in _keys()], allow_unused=True)
    zero = lambda k, g: torch.zeros_like(tr[k]) if g is None else g
    want_d = dict(losses={k: v.detach() for k, v in want.items()}, ll_loss=float(rll.detach()),
                  ll_grads=dict(zip(_keys(), g_ll[len(names):])), detached=dict(zip(names, g_task)),
                  pooled_only={k: zero(k, g) for k, g in zip(names, g_ll[:len(names)])})
    want_d["live"] = {k: want_d["detached"][k] + want_d["pooled_only"][k] for k in names}       # the gradient of a sum
    return dict(got=got, want=want_d, net=net, ll=ll, sd=sd, imgs=imgs, images=images, targets=targets)


def _grads_close(got, want, what):
    assert sorted(got) == sorted(want)
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
    assert worst[1] <= 1e-4, "%s: largest gradient error %.3g at %s" % (what, worst[1], worst[0])


def test_step_detached_losses_ll_loss_and_gradients(step):
    got, want = step["got"], step["want"]
    for k in R.LOSS_NAMES:
        for i, (g, w) in enumerate(zip(got["losses"][k].tolist(), want["losses"][k].tolist())):
            assert abs(g - w) <= 1e-4 * max(1.0, abs(w)), (k, i, g, w)
    assert abs(got["ll_loss"] - want["ll_loss"]) <= 1e-4 * max(1.0, abs(want["ll_loss"])), (got["ll_loss"], want["ll_loss"])
    assert want["ll_loss"] > 0, "at least one pair is inside the margin: LossNet receives a gradient"
    _grads_close(got["ll_grads"], want["ll_grads"], "LossNet")
    _grads_close(got["detached"], want["detached"], "detector, features detached")


def test_step_gradient_through_the_pooled_features_only(step):
    """Every task gscale is zero: the detector's gradients arrive ONLY through g_pooled and the broadcast join."""
    got, want = step["got"]["pooled_only"], step["want"]["pooled_only"]
    reached = [k for k, w in want.items() if float(w.abs().max()) > 0]
    assert any(k.startswith("backbone.fpn") for k in reached) and any(k.startswith("backbone.body.layer2") for k in reached)
    assert all(float(want[k].abs().max()) == 0 for k in want if k.startswith("rpn.") or k.startswith("roi_heads.")), "the heads are not upstream of the pyramid"
    _grads_close(got, want, "detector, through g_pooled only")


def test_step_live_features_full_loss(step):
    _grads_close(step["got"]["live"], step["want"]["live"], "detector, live features")
    assert any(not torch_equal(step["got"]["live"][k], step["got"]["detached"][k]) for k in step["got"]["live"])


def torch_equal(a, b):
    return a.numpy().tobytes() == b.numpy().tobytes()


def test_round_trip_trained_lossnet_is_scored_by_the_sweep(T, step):
    """One drop-in iteration (live features, both HIP optimizers), then the trained LossNet.state_dict() and the trained detector go into
    baselines.ll_get_uncertainty with the step's four images as one loader batch: the sweep's scores equal the training forward's ll_pred."""
    torch, ops = T
    from cald_amd import baselines, detector, ll_train, train
    net = train.FasterRCNNTrainer(step["sd"], 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(7), loss_mode="ll")
    model = train.TrainableDetector(net)
    ll = ll_train.LossNet(state_dict=step["ll"].state_dict())
    task_opt = train.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, net=net)
    ll_opt = train.SGD(ll.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, net=ll)
    before = {k: v.clone() for k, v in ll.state_dict().items()}
    w_before = net.params["backbone.fpn.layer_blocks.0.weight"].detach().clone()
    hist = ll_train.train_one_epoch(model, task_opt, ll, ll_opt, [(step["images"], step["targets"])], "cuda", 0, 1, 0, task_epochs=2)
    assert len(hist) == 1 and np.isfinite(hist[0]["task_loss"]) and hist[0]["ll_loss"] > 0
    assert not torch.equal(before["FC1.weight"], ll.state_dict()["FC1.weight"]) and not torch.equal(w_before, net.params["backbone.fpn.layer_blocks.0.weight"].detach())
    with torch.no_grad():
        features, loss_dict = model(step["images"], step["targets"])
        assert all(tuple(features[k].shape) == (4, 256) for k in "0123")
        ll_pred = ll(features).view(-1).cpu().numpy()
    det = detector.fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=160, max_size=256).to("cuda")
    det.load_state_dict(net.state_dict())
    det.eval()
    loader = [([torch.from_numpy(im).cuda() for im in step["imgs"]], [None] * 4)]
    scores = baselines.ll_get_uncertainty(det, ll, loader).numpy()
    print("round trip: training forward", ll_pred, "sweep", scores, "bit-equal" if scores.tobytes() == ll_pred.tobytes() else "not bit-equal")
    _close(scores, ll_pred, 1e-5, "sweep scores against the training forward's ll_pred")


def test_plain_trainer_is_unchanged_by_an_ll_trainer_in_the_same_process(T, step):
    """A trainer built without loss_mode returns the same losses and gradients, bit for bit, before and after ll-mode trainers ran."""
    torch, ops = T
    from cald_amd import train

    def plain():
        net = train.FasterRCNNTrainer(step["sd"], 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(7))
        losses = net.forward(step["images"][:2], step["targets"][:2])
        assert all(v.numel() == 1 for v in losses.values())
        grads = net.backward()
        return {k: _bits(v) for k, v in losses.items()}, {k: _bits(v) for k, v in grads.items()}
    first = plain()
    net = train.FasterRCNNTrainer(step["sd"], 21, min_size=160, max_size=256, box_batch=64, generator=torch.Generator().manual_seed(9), loss_mode="ll")
    _, pooled = net.forward(step["images"], step["targets"])
    net.backward([[0.25] * 4] * 4, g_pooled=torch.ones_like(pooled))
    assert plain() == first
