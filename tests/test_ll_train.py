"""Training the loss-prediction module, CPU side: the float64 restatement (tests/_ll_train_restatement.py) that the GPU tests compare the
HIP path with is itself pinned here to the EXECUTED reference (tests/golden/lossnet_train.npz from tools/make_golden_lossnet_train.py:
ll4al/main.py LossPredLoss, ll4al/models/lossnet.py LossNet under autograd, ll_train.py train_one_epoch; tests/golden/frcnn_losses.npz:
detection/frcnn_ll.py's per-image losses), and the Python surface's errors that need no GPU are checked.  Tolerances: the fixture holds
float32 results, the restatement runs in float64 -- 1e-5 of each tensor's largest entry (the project's operator-level bound)."""
import numpy as np
import pytest
import torch

import _ll_train_restatement as R


def _close(got, want, tol, what):
    got = np.asarray(got.detach() if hasattr(got, "detach") else got, np.float64); want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-30, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err <= tol, "%s: max err / max|ref| = %.3g > %.3g" % (what, err, tol)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("lossnet_train")


def test_fixture_covers_the_edge_cases_the_kernels_can_get_wrong(fx):
    names = [str(n) for n in fx["lpl_names"]]
    sizes = {len(fx["lpl_%s_input" % n]) for n in names}
    assert sizes == {2, 4, 6}
    tie = margin = inactive = False
    for n in names:
        x, t, m = fx["lpl_%s_input" % n], fx["lpl_%s_target" % n], float(fx["lpl_%s_margin" % n])
        h = len(x) // 2
        dt = (t - t[::-1])[:h]; dx = (x - x[::-1])[:h]
        one = np.where(dt > 0, 1.0, -1.0)
        tie |= bool((dt == 0).any()); margin |= bool((m - one * dx == 0).any()); inactive |= bool((m - one * dx < 0).any())
    assert tie and margin and inactive
    assert fx["ep0_lr"].shape == (3, 2) and "ep0_gfeat_0_0" not in fx.files and "ep5_gfeat_0_0" in fx.files


def test_loss_pred_loss_restatement_reproduces_the_reference(fx):
    for n in [str(n) for n in fx["lpl_names"]]:
        x = R.f64(fx["lpl_%s_input" % n]).requires_grad_(True)
        t, m = R.f64(fx["lpl_%s_target" % n]), float(fx["lpl_%s_margin" % n])
        loss = R.loss_pred_loss(x, t, m)
        loss.backward()
        assert abs(float(loss.detach()) - float(fx["lpl_%s_loss" % n])) <= 1e-6 * max(1.0, abs(float(loss.detach()))), n
        terms, want_terms = R.loss_pred_loss(x.detach(), t, m, reduction="none").numpy(), fx["lpl_%s_none" % n].astype(np.float64)
        assert np.abs(terms - want_terms).max() <= 1e-6 * max(1.0, float(np.abs(want_terms).max())), (n, terms, want_terms)
        got, want = x.grad.numpy(), fx["lpl_%s_grad" % n].astype(np.float64)
        assert np.abs(got - want).max() <= 1e-7, (n, got, want)              # +-1 / (B / 2) or 0: the tie is -1, the pair at the margin passes
    x = R.f64([1.0, 0.25, 0.5, 0.0]).requires_grad_(True)
    loss = R.loss_pred_loss(x, R.f64([2.0, 1.0, 1.0, 1.0]))
    loss.backward()
    assert float(loss.detach()) == 0.375 and x.grad.tolist() == [-0.5, 0.5, -0.5, 0.5]


@pytest.mark.parametrize("D", [128, 1])
def test_lossnet_restatement_reproduces_the_reference_with_gradients(fx, D):
    sd = {k: R.f64(fx["net%d_sd_%s" % (D, k)]).requires_grad_(True) for k in _keys()}
    maps = [R.f64(fx["net_feat%d" % i]).requires_grad_(True) for i in range(4)]
    pred, hidden = R.lossnet(sd, R.pooled_of(maps))
    assert hidden.shape == (4, 4, D)
    _close(pred, fx["net%d_out" % D], 1e-5, "LossNet output")
    (pred * R.f64(fx["net%d_g_pred" % D])).sum().backward()
    for k in _keys():
        _close(sd[k].grad, fx["net%d_grad_%s" % (D, k)], 1e-5, "gradient of " + k)
    for i in range(4):
        _close(maps[i].grad, fx["net%d_gfeat%d" % (D, i)], 1e-5, "gradient of map %d" % i)


def _keys():
    from cald_amd.baselines import LOSSNET_KEYS
    return LOSSNET_KEYS


@pytest.mark.parametrize("T", [0, 5])
def test_epoch_loop_restatement_reproduces_the_reference(fx, T):
    """Three iterations of ll_train.train_one_epoch (epoch 0: warm-up of both optimizers; SGD 0.01 / 0.9 / 1e-4): LossNet's parameters
    after every iteration, ll_loss, the logged learning rates, and the feature gradients -- None with task_epochs = 0 (the reference's
    default detaches), present with task_epochs = 5."""
    sd0 = {k: fx["ep_sd0_" + k] for k in _keys()}
    feats = [[fx["ep_feat_%d_%d" % (it, i)] for i in range(4)] for it in range(3)]
    losses = [{k: fx["ep%d_loss_%d_%s" % (T, it, k)] for k in R.LOSS_NAMES} for it in range(3)]
    out = R.train_epoch(sd0, feats, losses, task_epochs=T)
    for it, o in enumerate(out):
        for k in _keys():
            _close(o["sd"][k], fx["ep%d_sd_%d_%s" % (T, it, k)], 1e-5, "iteration %d %s" % (it, k))
        assert abs(o["ll_loss"] - float(fx["ep%d_ll_loss" % T][it])) <= 1e-5 * max(1.0, abs(o["ll_loss"]))
        assert abs(o["lr"] - fx["ep%d_lr" % T][it][1]) <= 1e-12 and abs(o["lr"] - fx["ep%d_lr" % T][it][0]) <= 1e-12
        if T == 0:
            assert o["gfeat"] is None
        else:
            for i in range(4):
                _close(o["gfeat"][i], fx["ep%d_gfeat_%d_%d" % (T, it, i)], 1e-5, "iteration %d map %d gradient" % (it, i))
    assert any(float(np.abs(fx["ep5_gfeat_%d_0" % it]).max()) > 0 for it in range(3)), "the live run carries a gradient into the maps"


def test_per_image_losses_restatement_reproduces_the_reference_copies(golden):
    """detection/frcnn_ll.py's per-image losses as executed (tests/golden/frcnn_losses.npz, single-image cases: read, never modified)."""
    g = golden("frcnn_losses")

    def close(got, key):
        w64 = float(g[key + "_f64"])
        assert abs(float(got) - w64) <= 1e-9 * max(abs(w64), 1e-3), (key, float(got), w64)
    for k in range(int(g["b_n"])):
        logits, deltas, labels, tgt = [torch.from_numpy(g["b%d_%s" % (k, n)]) for n in ("logits", "deltas", "labels", "targets")]
        cls, box = R.fastrcnn_loss_per_image(logits.double(), deltas.double(), labels.long(), tgt.double(), [logits.shape[0]])
        close(cls[0], "b%d_cls" % k); close(box[0], "b%d_box" % k)
    for k in range(int(g["r_n"])):
        obj, deltas, tgt = [torch.from_numpy(g["r%d_%s" % (k, n)]).double() for n in ("obj", "deltas", "targets")]
        pos, neg = torch.from_numpy(g["r%d_pos" % k]).long(), torch.from_numpy(g["r%d_neg" % k]).long()
        o, b = R.rpn_loss_per_image(obj.reshape(-1), deltas, tgt, pos, neg)
        close(o, "r%d_obj" % k); close(b, "r%d_box" % k)
    # two images of unequal row counts: every image is normalised by ITS count
    gen = torch.Generator().manual_seed(3)
    logits, breg = torch.randn(8, 5, generator=gen).double(), torch.randn(8, 20, generator=gen).double()
    labels, tgt = torch.tensor([0, 2, 0, 1, 0, 0, 0, 3]), torch.randn(8, 4, generator=gen).double()
    cls, box = R.fastrcnn_loss_per_image(logits, breg, labels, tgt, [3, 5])
    c0, b0 = R.fastrcnn_loss_per_image(logits[:3], breg[:3], labels[:3], tgt[:3], [3])
    c1, b1 = R.fastrcnn_loss_per_image(logits[3:], breg[3:], labels[3:], tgt[3:], [5])
    assert torch.equal(cls, torch.cat([c0, c1])) and torch.equal(box, torch.cat([b0, b1]))


def test_python_surface_errors_and_keys_need_no_gpu():
    from cald_amd import ll_train, train
    from cald_amd.baselines import LOSSNET_KEYS
    with pytest.raises(ValueError, match="not even"):
        ll_train.LossPredLoss(torch.zeros(3), torch.zeros(3))
    with pytest.raises(NotImplementedError, match="RetinaNet"):
        train.RetinaNetTrainer({}, 21, loss_mode="ll")
    with pytest.raises(ValueError, match="loss_mode"):
        train.FasterRCNNTrainer({}, 21, loss_mode="per_image")
    for D in (128, 1, 100):
        net = ll_train.LossNet(interm_dim=D, device="cpu")
        sd = net.state_dict()
        assert tuple(sd) == tuple(LOSSNET_KEYS)
        assert tuple(sd["FC1.weight"].shape) == (D, 256) and tuple(sd["linear.weight"].shape) == (1, 4 * D) and tuple(sd["linear.bias"].shape) == (1,)
        # parameters() are views of ONE flat buffer, every tensor 16-byte aligned: train.SGD's fused launch covers them
        base = net.flat.data_ptr()
        for k, p in net.named_parameters():
            assert p.data_ptr() == base + 4 * net._off[k] and net._off[k] % 4 == 0
        again = ll_train.LossNet(state_dict=sd, device="cpu")
        assert again.D == D and all(torch.equal(again.state_dict()[k], sd[k]) for k in LOSSNET_KEYS)
    with pytest.raises(ValueError):
        ll_train.LossNet(interm_dim=257, device="cpu")
    with pytest.raises(KeyError):
        ll_train.LossNet(state_dict={"FC1.weight": torch.zeros(4, 256)}, device="cpu")
    with pytest.raises(ValueError, match="pooled"):
        ll_train.LossNet(interm_dim=4, device="cpu")({str(k): torch.zeros(2, 256, 3, 3) for k in range(4)})
