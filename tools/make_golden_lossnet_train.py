"""tests/golden/lossnet_train.npz: the reference's training of the loss-prediction module, executed as it is (build container only).

Runs ``ll4al.main.LossPredLoss``, ``ll4al.models.lossnet.LossNet`` under autograd and ``ll_train.train_one_epoch`` of the reference tree on
the CPU under oracle/ref_harness.py's stubs (``torch.Tensor.cuda`` patched to the identity) and records inputs and results.  Only arrays
are written; no reference code is copied.

(a) ``lpl*``   LossPredLoss for B = 2, 4, 6: value and input gradient (reduction='mean'), the pair terms (reduction='none'); a tie in the
               target, a pair exactly at the margin, an inactive pair, a margin other than 1.
(b) ``net{D}`` LossNet(interm_dim=D), D = 128 and 1, on four maps of B = 4 images: output, and the gradients of sum(out * g_pred) with
               respect to the ten tensors and the four maps.
(c) ``ep{T}``  train_one_epoch with LossNet(interm_dim=4), three iterations of four images, epoch 0 (both warm-up schedulers), task_epochs = T in (0, 5): T = 0
               detaches the features (the reference's default), T = 5 lets LossNet's gradient into them.  A stub task model returns
               prepared maps and per-image losses (times one trainable scalar, so that the task optimizer has a parameter).  Recorded per
               iteration: the maps and losses handed out, LossNet's parameters afterwards, ll_loss, both learning rates as the reference
               logs them (after the schedulers' step), and the maps' gradients (absent when detached).

Values sit on a coarse binary grid so that the file stays small.  On such a grid a hidden pre-activation can be exactly zero in exact
arithmetic and fall on either side of the ReLU in float32, taking a whole gradient row with it, so the script asserts that every
pre-activation of cases (b) and (c) is at least 1e-4 away from zero (another seed if not).

    python tools/make_golden_lossnet_train.py            (from the repository root)
"""
import os
import sys
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

NET_HW = [(9, 11), (5, 6), (3, 3), (1, 1)]
EPOCH_HW = [(3, 4), (2, 2), (1, 2), (1, 1)]
CHANNELS = 256
LOSS_NAMES = ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")     # frcnn_ll.py's dict order
ITERS, BATCH = 3, 4
EPOCH_D = 4          # interm_dim of case (c): six parameter snapshots are recorded, the file has to stay small

# (name, input, target, margin)
LPL_CASES = [
    ("b4_tie_margin", [1.0, 0.25, 0.5, 0.0], [2.0, 1.0, 1.0, 1.0], 1.0),          # pair 0 exactly at the margin, pair 1 a tie
    ("b2_active", [0.5, -0.25], [1.0, 3.0], 1.0),
    ("b2_inactive", [3.0, 0.0], [2.0, 1.0], 1.0),
    ("b6_mixed", [0.75, -1.5, 0.125, 0.125, 2.0, -0.5], [0.5, 0.25, 1.0, 1.0, 1.25, 2.0], 1.0),   # active, inactive, tie
    ("b6_margin_half", [0.25, 0.5, -0.375, 0.625, 0.0, 0.75], [3.0, 1.0, 2.0, 1.5, 1.0, 0.5], 0.5),  # pair 0 at the margin 0.5
]


def grid(a, bits):
    """values on a coarse binary grid: exact float32 numbers whose low mantissa bytes are zero, so the compressed file stays small"""
    return (np.round(np.asarray(a) * 2.0 ** bits) / 2.0 ** bits).astype(np.float32)


def main():
    ref_harness.install_stubs()
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    import matplotlib
    matplotlib.use("Agg")
    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    import ll_train
    from ll4al.models.lossnet import LossNet
    from ll4al.main import LossPredLoss

    rs = np.random.RandomState(20260612)
    blob = {"net_hw": np.array(NET_HW, np.int64), "epoch_hw": np.array(EPOCH_HW, np.int64)}

    # ---- (a) ----
    blob["lpl_names"] = np.array([c[0] for c in LPL_CASES])
    for name, inp, tgt, margin in LPL_CASES:
        x = torch.tensor(inp, dtype=torch.float32, requires_grad=True)
        t = torch.tensor(tgt, dtype=torch.float32)
        loss = LossPredLoss(x, t, margin=margin)
        loss.backward()
        blob["lpl_%s_input" % name] = np.array(inp, np.float32)
        blob["lpl_%s_target" % name] = np.array(tgt, np.float32)
        blob["lpl_%s_margin" % name] = np.float32(margin)
        blob["lpl_%s_loss" % name] = loss.detach().numpy().copy()
        blob["lpl_%s_grad" % name] = x.grad.numpy().copy()
        blob["lpl_%s_none" % name] = LossPredLoss(x.detach(), t, margin=margin, reduction='none').numpy().copy()

    def fill(ll, wbits=10):
        with torch.no_grad():
            for name, p in ll.named_parameters():
                if name.endswith("bias"):
                    p.copy_(torch.from_numpy(grid(rs.randn(*p.shape) * 0.2 + 0.05, 8)))
                else:
                    p.copy_(torch.from_numpy(grid(rs.randn(*p.shape) / np.sqrt(p.shape[1]), wbits)))

    def relu_clear(ll, feats):
        """smallest |pre-activation| of the four FC layers in float64: a unit within float32 rounding of zero may take either side of the
        ReLU in another summation order, and its whole gradient row with it -- the recorded cases keep clear of that"""
        worst = np.inf
        for j, f in enumerate(feats):
            fc = getattr(ll, "FC%d" % (j + 1))
            z = f.detach().double().mean(dim=(2, 3)) @ fc.weight.detach().double().t() + fc.bias.detach().double()
            worst = min(worst, float(z.abs().min()))
        return worst

    # ---- (b) ----
    net_feats = [grid(rs.randn(BATCH, CHANNELS, h, w) * 0.8 + 0.35, 3) for h, w in NET_HW]         # the same maps for both widths
    for i, f in enumerate(net_feats):
        blob["net_feat%d" % i] = f
    for D in (128, 1):
        ll = LossNet(interm_dim=D)
        fill(ll, wbits=7)
        if D == 1:                                          # keep the single hidden unit of every branch alive
            with torch.no_grad():
                for j in range(1, 5):
                    getattr(ll, "FC%d" % j).bias.fill_(0.5)
        feats = [torch.from_numpy(f.copy()).requires_grad_(True) for f in net_feats]
        g_pred = torch.from_numpy(grid(rs.randn(BATCH), 4))
        for k, v in ll.state_dict().items():
            blob["net%d_sd_%s" % (D, k)] = v.numpy().copy()
        out = ll({str(i): f for i, f in enumerate(feats)})
        assert tuple(out.shape) == (BATCH, 1)
        assert relu_clear(ll, feats) >= 1e-4, "a hidden unit of case (b) sits on its ReLU's kink: change the seed"
        (out.view(-1) * g_pred).sum().backward()
        blob["net%d_out" % D] = out.detach().view(-1).numpy().copy()
        blob["net%d_g_pred" % D] = g_pred.numpy().copy()
        for i, f in enumerate(feats):
            blob["net%d_gfeat%d" % (D, i)] = f.grad.numpy().copy()
        for k, p in ll.named_parameters():
            blob["net%d_grad_%s" % (D, k)] = p.grad.numpy().copy()

    # ---- (c) ----
    ep_feats = [[grid(rs.randn(BATCH, CHANNELS, h, w) * 0.8 + 0.35, 3) for h, w in EPOCH_HW] for _ in range(ITERS)]
    ep_base = [{k: grid(np.abs(rs.randn(BATCH)) * 0.6 + 0.05, 6) for k in LOSS_NAMES} for _ in range(ITERS)]
    ll0 = LossNet(interm_dim=EPOCH_D)
    fill(ll0)
    sd0 = {k: v.clone() for k, v in ll0.state_dict().items()}
    for k, v in sd0.items():
        blob["ep_sd0_%s" % k] = v.numpy().copy()
    for it in range(ITERS):
        for i, f in enumerate(ep_feats[it]):
            blob["ep_feat_%d_%d" % (it, i)] = f

    for T in (0, 5):
        ll = LossNet(interm_dim=EPOCH_D)
        ll.load_state_dict(sd0)
        theta = torch.nn.Parameter(torch.ones(1))
        rec = dict(feats=[], losses=[], lr=[], sd=[])

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
                assert relu_clear(ll, fs) >= 1e-4, "a hidden unit of case (c) sits on its ReLU's kink: change the seed"
                losses = {k: torch.from_numpy(ep_base[it][k]) * theta for k in LOSS_NAMES}
                rec["losses"].append({k: v.detach().numpy().copy() for k, v in losses.items()})
                return {str(i): f for i, f in enumerate(fs)}, losses

        class Loader:
            """three batches of four; every __next__ after the first sees the state the previous iteration left"""

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
        ll_train.args = Namespace(model="faster_rcnn", task_epochs=T, ll_weight=1.0)
        logger = ll_train.train_one_epoch(StubTask(), task_opt, ll, ll_opt, Loader(), torch.device("cpu"), 0, 0, 1000)
        assert len(rec["sd"]) == ITERS and len(rec["feats"]) == ITERS
        blob["ep%d_ll_loss" % T] = np.array(list(logger.meters["ll_loss"].deque), np.float32)
        blob["ep%d_lr" % T] = np.array(rec["lr"], np.float64)                  # [iteration][task, ll]
        for it in range(ITERS):
            for k in LOSS_NAMES:
                blob["ep%d_loss_%d_%s" % (T, it, k)] = rec["losses"][it][k]
            for k, v in rec["sd"][it].items():
                blob["ep%d_sd_%d_%s" % (T, it, k)] = v.numpy().copy()
            for i, f in enumerate(rec["feats"][it]):
                assert (f.grad is None) == (T == 0)
                if f.grad is not None:
                    blob["ep%d_gfeat_%d_%d" % (T, it, i)] = f.grad.numpy().copy()
    assert not np.array_equal(blob["ep0_sd_2_FC1.weight"], blob["ep_sd0_FC1.weight"])
    path = os.path.join(ROOT, "tests", "golden", "lossnet_train.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
