"""tests/golden/lossnet.npz: the reference's learning-loss scoring, executed as it is (build container only).

Runs ``ll_train.get_uncertainty`` and ``ll4al.models.lossnet.LossNet`` of the reference tree on the CPU under oracle/ref_harness.py's
stubs, with a stub task model that returns prepared feature maps, and records inputs and outputs.  Only arrays are written; no reference
code is copied.

Cases (same features, same LossNet): ``faster_rcnn`` -- loader batches of 2 and 1 images, the feature dict '0'..'3' as frcnn_ll.py returns
it; ``retina`` -- the feature list as retina_ll.py returns it, of which ll_train.py:155-161 feeds element 0 to all four branches.

    python tools/make_golden_lossnet.py            (from the repository root)
"""
import os
import sys
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

LEVEL_HW = [(9, 11), (5, 6), (3, 3), (1, 1)]
BATCHES = [2, 1]
CHANNELS = 256


def main():
    ref_harness.install_stubs()
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    import matplotlib
    matplotlib.use("Agg")
    import torch
    import ll_train
    from ll4al.models.lossnet import LossNet

    rs = np.random.RandomState(20260117)
    n = sum(BATCHES)
    # values on a coarse binary grid (features 2^-6, weights 2^-10, biases 2^-8): exact float32 numbers whose low mantissa bytes are zero, so
    # the compressed file stays small
    grid = lambda a, bits: (np.round(a * 2.0 ** bits) / 2.0 ** bits).astype(np.float32)
    feats = [grid(rs.randn(n, CHANNELS, h, w) * 0.8 + 0.35, 6) for (h, w) in LEVEL_HW]
    torch.manual_seed(7)
    ll = LossNet()
    with torch.no_grad():
        for name, p in ll.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.from_numpy(grid(rs.randn(*p.shape) * 0.2 + 0.05, 8)))      # non-zero biases
            else:
                p.copy_(torch.from_numpy(grid(rs.randn(*p.shape) / np.sqrt(p.shape[1]), 10)))
    blob = {"batches": np.array(BATCHES, np.int64), "level_hw": np.array(LEVEL_HW, np.int64)}
    for i, f in enumerate(feats):
        blob["feat%d" % i] = f                               # [n][256][H][W], as the reference's modules see them
    for k, v in ll.state_dict().items():
        blob["sd_" + k] = v.numpy().copy()

    class StubTask:
        """task_model(images) -> (features, detections): the feature maps of the loader batch that is asked for"""

        def __init__(self, as_list):
            self.as_list, self.at = as_list, 0

        def eval(self):
            return self

        def __call__(self, images):
            lo, hi = self.at, self.at + len(images)
            self.at = hi
            fs = [torch.from_numpy(f[lo:hi]) for f in feats]
            return (fs if self.as_list else {str(i): f for i, f in enumerate(fs)}), None

    loader = []
    for b in BATCHES:
        loader.append(([torch.zeros(3, 4, 4) for _ in range(b)], [None] * b))
    for model, as_list in (("faster_rcnn", False), ("retina", True)):
        ll_train.args = Namespace(model=model)
        out = ll_train.get_uncertainty(StubTask(as_list), ll, loader)
        assert out.dtype == torch.float32 and tuple(out.shape) == (n,)
        blob["out_" + model] = out.numpy().copy()
    assert not np.array_equal(blob["out_faster_rcnn"], blob["out_retina"])
    path = os.path.join(ROOT, "tests", "golden", "lossnet.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
