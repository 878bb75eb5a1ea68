"""Training LossNet beside RetinaNet, CPU side: the float64 restatement (tests/_retina_ll_restatement.py) that the GPU tests compare the HIP
path with is pinned here to the EXECUTED reference (tests/golden/retina_ll_train.npz from tools/make_golden_retina_ll.py:
detection/retina_ll.py's per-image head losses, ll_train.py train_one_epoch through its 'retina' branch), and the Python surface that needs
no GPU is checked.  Bounds: those of test_ll_train.py for the Faster R-CNN copies -- 1e-9 relative against float64 recordings, 1e-5 against
float32 ones."""
import numpy as np
import pytest
import torch

import _retina_ll_restatement as R


@pytest.fixture(scope="module")
def fx(golden):
    return golden("retina_ll_train")


def _keys():
    from cald_amd.baselines import LOSSNET_KEYS
    return LOSSNET_KEYS


def _close(got, want, tol, what):
    got = np.asarray(got.detach() if hasattr(got, "detach") else got, np.float64); want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-30, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err <= tol, "%s: max err / max|ref| = %.3g > %.3g" % (what, err, tol)


def _n_cases(fx):
    return len(fx["a_names"])


def test_fixture_covers_the_edge_cases_the_kernels_can_get_wrong(fx):
    unequal = all_bg = ignored = single_gt_ignored = first_last = multi_block = False
    for c in range(_n_cases(fx)):
        m = fx["a%d_matched" % c]
        N, At = m.shape
        assert At == 9 * int(fx["a%d_level_pix" % c].sum()) and N == int(fx["a%d_N" % c]) and N >= 3
        nfg = (m >= 0).sum(1)
        unequal |= len(set(nfg.tolist())) == N
        multi_block |= At > 256
        for n in range(N):
            n_gt = len(fx["a%d_gt%d" % (c, n)])
            assert m[n].max() < n_gt
            all_bg |= bool((m[n] == -1).all())
            ignored |= bool((m[n] == -2).any() and nfg[n] > 0)
            single_gt_ignored |= bool(n_gt == 1 and (m[n] == -2).any() and nfg[n] > 0)
            first_last |= bool(m[n, 0] >= 0 and m[n, -1] >= 0)
        # an image without foreground: regression loss exactly 0, classification loss over max(1, 0) = 1
        for n in np.flatnonzero(nfg == 0):
            assert fx["a%d_reg_f32" % c][n] == 0.0 and fx["a%d_reg_f64" % c][n] == 0.0 and fx["a%d_cls_f64" % c][n] > 0
    assert unequal and all_bg and ignored and single_gt_ignored and first_last and multi_block
    x = fx["a0_cls_logits"]
    assert (x == 0).any() and (np.abs(x) == 30).sum() >= 3 and np.signbit(x[x == 0]).any()
    assert fx["ep0_lr"].shape == (3, 2) and "ep0_gfeat_0_0" not in fx.files and "ep5_gfeat_0_0" in fx.files and "ep5_gfeat_0_4" not in fx.files


def _case(fx, c, dtype):
    N = int(fx["a%d_N" % c])
    gts = [torch.from_numpy(fx["a%d_gt%d" % (c, n)]).to(dtype) for n in range(N)]
    labels = [torch.from_numpy(fx["a%d_labels%d" % (c, n)]) for n in range(N)]
    return (torch.from_numpy(fx["a%d_cls_logits" % c]).to(dtype), torch.from_numpy(fx["a%d_bbox_regression" % c]).to(dtype),
            torch.from_numpy(fx["a%d_anchors" % c]).to(dtype), gts, labels, fx["a%d_matched" % c])


def test_per_image_losses_restatement_reproduces_the_reference(fx):
    for c in range(_n_cases(fx)):
        (cm, cl), (rm, rl) = R.retina_losses_per_image(*_case(fx, c, torch.float64))
        for got, key in ((cl, "cls"), (rl, "reg"), (cm.reshape(1), "cls_mean"), (rm.reshape(1), "reg_mean")):
            got = got.numpy()
            w64 = np.atleast_1d(fx["a%d_%s_f64" % (c, key)]); w32 = np.atleast_1d(fx["a%d_%s_f32" % (c, key)])
            assert np.all(np.abs(got - w64) <= 1e-9 * np.maximum(np.abs(w64), 1e-3)), (c, key, got, w64)
            assert np.all(np.abs(got - w32) <= 1e-5 * np.maximum(np.abs(w32), 1e-3)), (c, key, got, w32)
        # every image is normalised by ITS foreground count, and does not depend on the rest of the batch
        cls, reg, anchors, gts, labels, m = _case(fx, c, torch.float64)
        for n in range(len(gts)):
            (_, c1), (_, r1) = R.retina_losses_per_image(cls[n:n + 1], reg[n:n + 1], anchors, gts[n:n + 1], labels[n:n + 1], m[n:n + 1])
            assert torch.equal(c1[0], cl[n]) and torch.equal(r1[0], rl[n])


@pytest.mark.parametrize("T", [0, 5])
def test_epoch_loop_restatement_reproduces_the_reference(fx, T):
    """Three iterations of ll_train.train_one_epoch with args.model = 'retinanet' (epoch 0: warm-up of both optimizers; SGD 0.01 / 0.9 /
    1e-4): LossNet's parameters after every iteration, ll_loss, the logged learning rates and the feature gradients (None when detached)."""
    sd0 = {k: fx["ep_sd0_" + k] for k in _keys()}
    feats = [[fx["ep_feat_%d_%d" % (it, i)] for i in range(4)] for it in range(3)]
    losses = [{k: fx["ep%d_loss_%d_%s" % (T, it, k)] for k in R.LOSS_NAMES} for it in range(3)]
    out = R.train_epoch_retina(sd0, feats, losses, task_epochs=T)
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
        for k in R.LOSS_NAMES:                              # the mean handed out is the per-image values' float32 sum in image order / N
            per = fx["ep%d_loss_%d_%s" % (T, it, k)]
            s = per[0]
            for v in per[1:]:
                s = np.float32(s + v)
            assert np.float32(s / np.float32(len(per))) == fx["ep%d_mean_%d_%s" % (T, it, k)]
    assert any(float(np.abs(fx["ep5_gfeat_%d_0" % it]).max()) > 0 for it in range(3)), "the live run carries a gradient into the maps"


def test_python_surface_needs_no_gpu():
    from cald_amd import train, train_retina_ll
    assert train.RetinaNetLLTrainer is train_retina_ll.RetinaNetLLTrainer and issubclass(train.RetinaNetLLTrainer, train.RetinaNetTrainer)
    assert train.RetinaNetLLTrainer.loss_mode == "ll" and train.RetinaNetLLTrainer.LOSS_NAMES == train.RetinaNetTrainer.LOSS_NAMES
    with pytest.raises(NotImplementedError, match="RetinaNetLLTrainer"):
        train.RetinaNetTrainer({}, 21, loss_mode="ll")
    for bad in ("per_image", "LL", 1, ""):
        with pytest.raises(ValueError, match="loss_mode"):
            train.RetinaNetTrainer({}, 21, loss_mode=bad)
    with pytest.raises(ValueError):
        train.RetinaNetLLTrainer({}, 21, loss_mode=None)
