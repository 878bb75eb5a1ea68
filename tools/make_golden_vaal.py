"""tests/golden/vaal.npz: the reference's VAAL sampling pass, executed as it is (build container only).

Imports ``vaal.vaal_helper`` of the reference tree on the CPU under oracle/ref_harness.py's stubs (torch.Tensor.cuda an identity) and runs
``sample_for_labeling`` on eight small images with the weights of tests/_vaal_restatement.py's generator -- the VAE in train() mode, the
state the reference's sampler finds it in, and in eval() mode -- in float32 and, the same modules in .double(), in float64.  Only arrays
are written; no reference code is copied.  The weights (200 MB) are not stored: the fixture keeps the generator's seed and the SHA-1 of the
bytes it must reproduce.

    python tools/make_golden_vaal.py            (from the repository root)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402
import _vaal_restatement as R  # noqa: E402

SEED = 20261019
BUDGET = 3
# (H, W): smaller than 256 both ways, larger both ways and portrait, around the 256 boundary, wide, portrait, square, a single pixel
IMAGE_HW = [(40, 56), (300, 280), (257, 333), (255, 256), (120, 400), (333, 200), (64, 64), (1, 1)]


def make_images():
    """Blocky colour patches under a ramp: varied enough for eight distinct predictions, regular enough to compress."""
    rs = np.random.RandomState(SEED + 1)
    out = []
    for H, W in IMAGE_HW:
        blocks = rs.randint(0, 256, ((H + 7) // 8, (W + 7) // 8, 3))
        img = np.kron(blocks, np.ones((8, 8, 1), np.int64))[:H, :W].astype(np.float64)
        ramp = (np.arange(H)[:, None, None] * 2 + np.arange(W)[None, :, None] * 3) % 64
        out.append(np.clip(img * 0.75 + ramp, 0, 255).astype(np.uint8))
    return out


def main():
    ref_harness.install_stubs()
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    import torch
    from vaal import vaal_helper

    sd = R.make_weights(SEED)
    images = make_images()
    blob = {"seed": np.array(SEED, np.int64), "budget": np.array(BUDGET, np.int64), "sha1": np.array(R.weights_sha1(sd)),
            "n_images": np.array(len(images), np.int64)}
    for i, im in enumerate(images):
        blob["image%d" % i] = im
    torch.manual_seed(0)
    keys, shapes = [], []
    for mod in (vaal_helper.VAE(), vaal_helper.Discriminator()):
        for k, v in mod.state_dict().items():
            keys.append(k); shapes.append(list(v.shape) + [0] * (4 - v.dim()))
    blob["sd_keys"] = np.array(keys); blob["sd_shapes"] = np.array(shapes, np.int64)

    def run(train, double):
        torch.manual_seed(0)
        vae, disc = vaal_helper.VAE(), vaal_helper.Discriminator()
        tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
        vae.load_state_dict({k: v for k, v in tsd.items() if not k.startswith("net.")}, strict=False)
        disc.load_state_dict({k: v for k, v in tsd.items() if k.startswith("net.")})
        vae.train(train)
        dt = torch.float64 if double else torch.float32
        if double:
            vae, disc = vae.double(), disc.double()
        mus, preds = [], []
        vae.fc_mu.register_forward_hook(lambda m, i, o: mus.append(o.detach().numpy().copy()[0]))
        disc.register_forward_hook(lambda m, i, o: preds.append(float(o.detach().reshape(-1)[0]) if double else o.detach().numpy().reshape(-1)[0]))
        # to_tensor: uint8 HWC -> CHW / 255, in the run's precision (in float64 (u / 255) * 255 is u to 1e-16, as it is exactly in float32)
        loader = [([torch.from_numpy(im).permute(2, 0, 1).contiguous().to(dt).div(255)], None) for im in images]
        idx = vaal_helper.sample_for_labeling(vae, disc, loader, BUDGET)
        return np.stack(mus), np.array(preds, np.float64 if double else np.float32), np.asarray(idx, np.int64)

    for train in (True, False):
        tag = "train" if train else "eval"
        mu, preds, idx = run(train, False)
        mu64, preds64, idx64 = run(train, True)
        assert mu.dtype == np.float32 and preds.dtype == np.float32 and mu64.dtype == np.float64
        assert len(set(preds.tolist())) == len(preds) and len(set(preds64.tolist())) == len(preds64), "two predictions are equal"
        assert np.array_equal(idx, idx64)
        s = np.sort(preds64)
        gap, noise = s[BUDGET] - s[BUDGET - 1], np.abs(preds.astype(np.float64) - preds64).max()
        assert gap >= 100 * noise, "the selection hinges on rounding: gap %g, float32 noise %g" % (gap, noise)
        print("%s: preds %s\n  idx %s  gap %.3g  float32 noise %.3g  |mu32 - mu64| / max|mu64| = %.3g" %
              (tag, preds, idx, gap, noise, np.abs(mu - mu64).max() / np.abs(mu64).max()))
        blob.update({"mu_" + tag: mu, "preds_" + tag: preds, "idx_" + tag: idx, "mu64_" + tag: mu64, "preds64_" + tag: preds64})
    path = os.path.join(ROOT, "tests", "golden", "vaal.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
