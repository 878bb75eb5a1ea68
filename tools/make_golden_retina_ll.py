"""tests/golden/retina_ll_train.npz: the reference's RetinaNet beside LossNet, executed as it is (build container only).

Runs ``RetinaNetClassificationHead.compute_loss`` / ``RetinaNetRegressionHead.compute_loss`` of detection/retina_ll.py and the 'retina'
branch of ``ll_train.train_one_epoch`` of the reference tree on the CPU under oracle/ref_harness.py's stubs and records inputs and results.
Only arrays are written; no reference code is copied.

(a) ``a{c}``  both heads' per-image losses (retina_ll.py:100-132, :183-220) in float32 and float64 on small multi-image cases with the
              matcher's decisions given: unequal #foreground per image, an image whose anchors are all background, images with ignored
              anchors, and a single-GT image with ignored anchors (where the ``clamp(min=0)`` of :200 keeps the index -2 in bounds).
              ``sigmoid_focal_loss`` and ``BoxCoder.encode_single`` are torchvision's and are bound to the restatements
              oracle/make_golden_train_losses.py already uses.  Recorded: the inputs, each per-image list and the two means.
              Logits and anchors are laid out (level, pixel, anchor) over ``a{c}_level_pix`` pixels of 9 anchors.
(b) ``ep{T}`` train_one_epoch with ``args.model = "retinanet"``, LossNet(interm_dim=4), three iterations of four images, epoch 0,
              task_epochs = T in (0, 5).  A stub task model returns a FIVE-element feature list (the loop reads [0..3]) and ``(mean, [per
              image])`` tuples times one trainable scalar.  Recorded as lossnet_train.npz records its ``ep{T}``: maps and losses handed
              out, LossNet's parameters after each iteration, ll_loss, both learning rates, the maps' gradients (absent when detached);
              every hidden pre-activation is at least 1e-4 away from its ReLU's kink.

    python tools/make_golden_retina_ll.py            (from the repository root)
"""
import os
import sys
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden_train_losses as mg  # noqa: E402
from tools.make_golden_lossnet_train import BATCH, CHANNELS, EPOCH_D, EPOCH_HW, ITERS, grid  # noqa: E402

LOSS_NAMES = ("classification", "bbox_regression")        # retina_ll.py's dict order
A = 9
# (name, K, level_pix, per image: (number of GT boxes, #foreground, #ignored))
A_CASES = [
    ("small_k3", 3, [6, 2, 1, 1, 1], [(3, 5, 4), (2, 0, 0), (2, 2, 11), (1, 3, 6)]),
    ("two_blocks_k5", 5, [20, 6, 2, 1, 1], [(1, 1, 30), (4, 17, 0), (2, 0, 9)]),
]


def case_a(rs, torch, heads, K, level_pix, per_image):
    cls_head, reg_head = heads
    N, At = len(per_image), A * sum(level_pix)
    blob = {"K": np.int64(K), "level_pix": np.array(level_pix, np.int64), "N": np.int64(N)}
    logits = grid(rs.randn(N, At, K) * 3.0, 6)
    logits[0, 0, 0], logits[0, 1, 1], logits[0, 2, 0], logits[0, 3, 1], logits[0, 4, 2] = 0.0, -0.0, 30.0, -30.0, 30.0
    reg = grid(rs.randn(N, At, 4) * 0.6, 8)
    x0, y0 = rs.rand(At) * 100, rs.rand(At) * 100
    anchors = grid(np.stack([x0, y0, x0 + 8 + rs.rand(At) * 60, y0 + 8 + rs.rand(At) * 60], 1), 3)
    matched = np.full((N, At), -1, np.int64)
    gts, labels = [], []
    for n, (n_gt, n_fg, n_ign) in enumerate(per_image):
        gx, gy = rs.rand(n_gt) * 100, rs.rand(n_gt) * 100
        gts.append(grid(np.stack([gx, gy, gx + 10 + rs.rand(n_gt) * 50, gy + 10 + rs.rand(n_gt) * 50], 1), 3))
        labels.append(rs.randint(0, K, n_gt).astype(np.int64))
        pick = rs.permutation(At)
        if n == 0:                                             # a foreground anchor at the image's first and last anchor
            pick = np.concatenate([[0, At - 1], pick[(pick != 0) & (pick != At - 1)]])
        matched[n, pick[:n_fg]] = rs.randint(0, n_gt, n_fg)
        matched[n, pick[n_fg:n_fg + n_ign]] = -2
    blob.update(cls_logits=logits, bbox_regression=reg, anchors=anchors, matched=matched)
    for n in range(N):
        blob["gt%d" % n], blob["labels%d" % n] = gts[n], labels[n]
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        targets = [{"boxes": torch.from_numpy(g).to(dt), "labels": torch.from_numpy(l)} for g, l in zip(gts, labels)]
        head = {"cls_logits": torch.from_numpy(logits).to(dt), "bbox_regression": torch.from_numpy(reg).to(dt)}
        m = [torch.from_numpy(matched[n]) for n in range(N)]
        cm, cl = cls_head.compute_loss(targets, head, m)
        rm, rl = reg_head.compute_loss(targets, head, [torch.from_numpy(anchors).to(dt)] * N, m)
        assert len(cl) == N and len(rl) == N and cm.dtype == dt and rm.dtype == dt
        blob["cls_" + tag] = np.array([float(v) for v in cl], np.float64)
        blob["reg_" + tag] = np.array([float(v) for v in rl], np.float64)
        blob["cls_mean_" + tag], blob["reg_mean_" + tag] = np.float64(float(cm)), np.float64(float(rm))
    return blob


def main():
    mg.ref_harness.install_stubs()
    if mg.ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, mg.ref_harness.REF_ROOT)
    import matplotlib
    matplotlib.use("Agg")
    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    import ll_train
    from detection import retina_ll as rl
    from ll4al.models.lossnet import LossNet

    rs = np.random.RandomState(20261019)
    blob = {"epoch_hw": np.array(EPOCH_HW, np.int64)}

    # ---- (a) ----
    rl.sigmoid_focal_loss = mg.sigmoid_focal_loss
    ch = rl.RetinaNetClassificationHead.__new__(rl.RetinaNetClassificationHead); torch.nn.Module.__init__(ch)
    ch.num_anchors, ch.BETWEEN_THRESHOLDS = A, mg.Matcher.BETWEEN_THRESHOLDS
    rh = rl.RetinaNetRegressionHead.__new__(rl.RetinaNetRegressionHead); torch.nn.Module.__init__(rh)
    rh.box_coder = mg.BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
    blob["a_names"] = np.array([c[0] for c in A_CASES])
    for c, (name, K, level_pix, per_image) in enumerate(A_CASES):
        ch.num_classes = K
        for k, v in case_a(rs, torch, (ch, rh), K, level_pix, per_image).items():
            blob["a%d_%s" % (c, k)] = v
        print("case a%d %-16s cls %s reg %s" % (c, name, blob["a%d_cls_f32" % c], blob["a%d_reg_f32" % c]))

    # ---- (b) ----
    def fill(ll, wbits=10):
        with torch.no_grad():
            for name, p in ll.named_parameters():
                if name.endswith("bias"):
                    p.copy_(torch.from_numpy(grid(rs.randn(*p.shape) * 0.2 + 0.05, 8)))
                else:
                    p.copy_(torch.from_numpy(grid(rs.randn(*p.shape) / np.sqrt(p.shape[1]), wbits)))

    def relu_clear(ll, feats):
        worst = np.inf
        for j, f in enumerate(feats[:4]):
            fc = getattr(ll, "FC%d" % (j + 1))
            z = f.detach().double().mean(dim=(2, 3)) @ fc.weight.detach().double().t() + fc.bias.detach().double()
            worst = min(worst, float(z.abs().min()))
        return worst

    hw5 = list(EPOCH_HW) + [(1, 1)]                            # the fifth map (P7) is handed out and never read
    ep_feats = [[grid(rs.randn(BATCH, CHANNELS, h, w) * 0.8 + 0.35, 3) for h, w in hw5] for _ in range(ITERS)]
    ep_base = [{k: grid(np.abs(rs.randn(BATCH)) * 0.6 + 0.05, 6) for k in LOSS_NAMES} for _ in range(ITERS)]
    ll0 = LossNet(interm_dim=EPOCH_D)
    fill(ll0)
    sd0 = {k: v.clone() for k, v in ll0.state_dict().items()}
    for k, v in sd0.items():
        blob["ep_sd0_%s" % k] = v.numpy().copy()
    for it in range(ITERS):
        for i, f in enumerate(ep_feats[it][:4]):
            blob["ep_feat_%d_%d" % (it, i)] = f

    for T in (0, 5):
        ll = LossNet(interm_dim=EPOCH_D)
        ll.load_state_dict(sd0)
        theta = torch.nn.Parameter(torch.ones(1))
        rec = dict(feats=[], losses=[], means=[], lr=[], sd=[])

        class StubTask:
            def __init__(self):
                self.at = 0

            def train(self):
                return self

            def __call__(self, images, targets):
                it = self.at
                self.at += 1
                fs = [torch.from_numpy(f.copy()).requires_grad_(True) for f in ep_feats[it]]
                rec["feats"].append(fs)
                assert relu_clear(ll, fs) >= 1e-4, "a hidden unit of case (b) sits on its ReLU's kink: change the seed"
                out = {}
                for k in LOSS_NAMES:
                    per = list((torch.from_numpy(ep_base[it][k]) * theta).unbind(0))
                    out[k] = (sum(per) / len(per), per)
                rec["losses"].append({k: torch.stack(v[1]).detach().numpy().copy() for k, v in out.items()})
                rec["means"].append({k: v[0].detach().numpy().copy() for k, v in out.items()})
                return fs, out

        class Loader:
            def __len__(self):
                return ITERS

            def __iter__(self):
                for it in range(ITERS):
                    if it:
                        self.snap()
                    yield [torch.zeros(3, 4, 4) for _ in range(BATCH)], [{"boxes": torch.zeros(0, 4)} for _ in range(BATCH)]
                self.snap()

            def snap(self):
                rec["lr"].append((task_opt.param_groups[0]["lr"], ll_opt.param_groups[0]["lr"]))
                rec["sd"].append({k: v.clone() for k, v in ll.state_dict().items()})

        task_opt = torch.optim.SGD([theta], lr=0.01, momentum=0.9, weight_decay=1e-4)
        ll_opt = torch.optim.SGD(ll.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        ll_train.args = Namespace(model="retinanet", task_epochs=T, ll_weight=1.0)
        logger = ll_train.train_one_epoch(StubTask(), task_opt, ll, ll_opt, Loader(), torch.device("cpu"), 0, 0, 1000)
        assert len(rec["sd"]) == ITERS and len(rec["feats"]) == ITERS
        blob["ep%d_ll_loss" % T] = np.array(list(logger.meters["ll_loss"].deque), np.float32)
        blob["ep%d_lr" % T] = np.array(rec["lr"], np.float64)                  # [iteration][task, ll]
        for it in range(ITERS):
            for k in LOSS_NAMES:
                blob["ep%d_loss_%d_%s" % (T, it, k)] = rec["losses"][it][k]
                blob["ep%d_mean_%d_%s" % (T, it, k)] = rec["means"][it][k]
            for k, v in rec["sd"][it].items():
                blob["ep%d_sd_%d_%s" % (T, it, k)] = v.numpy().copy()
            for i, f in enumerate(rec["feats"][it]):
                assert (f.grad is None) == (T == 0 or i == 4)
                if f.grad is not None:
                    blob["ep%d_gfeat_%d_%d" % (T, it, i)] = f.grad.numpy().copy()
    assert not np.array_equal(blob["ep0_sd_2_FC1.weight"], blob["ep_sd0_FC1.weight"])
    path = os.path.join(ROOT, "tests", "golden", "retina_ll_train.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
