"""Writes tests/golden/frcnn_audit_margins.npz: the Faster R-CNN decision margins of a fixed 16-image sweep.

    python tools/make_golden_frcnn_audit.py [out.npz]

tests/test_gpu_retina_audit.py compares cald_sweep_audit on the same sweep with it, bit for bit: the RetinaNet audit added a public
margin slot (15) and a per-view record, and must leave every Faster R-CNN margin what it was.  The committed file was written by the
commit BEFORE the RetinaNet audit; regenerate it only when a change of the Faster R-CNN margins is intended.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, AUGS, SIZES, BATCH = 16, ["flip", "cut_out", "smaller_resize"], dict(min_size=300, max_size=500), 8


def sweep_margins(precision="fp32"):
    """(consistency [16], margins [16][N_MARGINS]) of the fixture's sweep on the current build."""
    import torch
    from cald_amd import detector, synth, sweep
    m = detector.fasterrcnn_resnet50_fpn_feature(num_classes=21, precision=precision, **SIZES).to("cuda")
    m.load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0)); m.eval()
    dev = [torch.from_numpy(im).cuda() for im in synth.make_pool(N, "voc", 0, scale=0.5)]
    c, _, mg = sweep.sweep_device_images(m, dev, list(range(N)), AUGS, bp=1.3, base_seed=0, batch_images=BATCH, margins=True)
    return c, mg


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "frcnn_audit_margins.npz")
    c, mg = sweep_margins()
    np.savez_compressed(out, consistency=c, margins=mg[:, :15])
    print("wrote", out, mg.shape, "finite per slot:", np.isfinite(mg).sum(0).tolist())
