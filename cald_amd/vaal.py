"""The VAAL baseline's pool sweep on the MI355X (vaal/vaal_helper.py:186-222 AdversarySampler.sample / sample_for_labeling, called at
vaal_train.py:265-268): every unlabeled image is resized to 256 x 256 (nearest), encoded by the VAE's five conv + BatchNorm + ReLU stages
and fc_mu, and scored by the discriminator; the `budget` images with the LOWEST prediction are queried.

``sample_for_labeling(vae, discriminator, unlabeled_loader, budget)``  -- the reference's function, same positional signature and return
``AdversarySampler(budget).sample(vae, discriminator, loader)``        -- the reference's class
``vaal_sweep_device_images(vae, discriminator, images)``               -- images already in HBM -> preds (and mu)
``VAE`` / ``Discriminator``                                            -- plain torch modules with the reference's state_dict() keys

The sweep runs on the library's kernels (csrc/vaal.hip) and has no CPU or torch fallback.  What it does not reproduce of the reference's
side effects: the global torch generator is not advanced (the reference draws one randn(1, 256) per image for a latent nobody reads), and
a VAE in train() mode keeps its running statistics and num_batches_tracked (the reference updates them once per image).  VAAL's training
is not part of this module.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _ffi
from .sweep import _to_u8_cuda

Z_DIM = 256
ENC_WIDTHS = (3, 64, 128, 256, 512, 1024)
VAE_KEYS = tuple("encoder.%d.%s" % (3 * l, p) for l in range(5) for p in ("weight", "bias")) \
    + tuple("encoder.%d.%s" % (3 * l + 1, p) for l in range(5) for p in ("weight", "bias", "running_mean", "running_var")) \
    + ("fc_mu.weight", "fc_mu.bias")
DISC_KEYS = tuple("net.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias"))


class _View(nn.Module):
    def __init__(self, size):
        super().__init__()
        self.size = size

    def forward(self, t):
        return t.view(self.size)


def _kaiming(m):
    if isinstance(m, (nn.Linear, nn.Conv2d)):
        nn.init.kaiming_normal_(m.weight)
        if m.bias is not None:
            m.bias.data.fill_(0)
    elif isinstance(m, nn.BatchNorm2d):
        m.weight.data.fill_(1)
        m.bias.data.fill_(0)


class VAE(nn.Module):
    """The VAAL encoder-decoder: encoder = five [Conv2d(k=4, s=2, p=1) -> BatchNorm2d -> ReLU] stages 3 -> 64 -> 128 -> 256 -> 512 -> 1024
    on a 256 x 256 input (maps 128, 64, 32, 16, 8), flattened in NCHW order; fc_mu and fc_logvar 65 536 -> z_dim; decoder = Linear and five
    [ConvTranspose2d(k=4, s=2, p=1) -> BatchNorm2d -> ReLU] stages 1024 -> 512 -> 256 -> 128 -> 64 -> 32 and a 1 x 1 transposed conv to nc.
    forward(imgs) resizes every image to 256 x 256 (nearest), multiplies by 255 and returns (x_recon, z, mu, logvar)."""

    def __init__(self, z_dim=Z_DIM, nc=3):
        super().__init__()
        self.z_dim, self.nc = z_dim, nc
        enc, w = [], (nc,) + ENC_WIDTHS[1:]
        for l in range(5):
            enc += [nn.Conv2d(w[l], w[l + 1], 4, 2, 1, bias=True), nn.BatchNorm2d(w[l + 1]), nn.ReLU(True)]
        self.encoder = nn.Sequential(*enc, _View((-1, 1024 * 8 * 8)))
        self.fc_mu = nn.Linear(1024 * 8 * 8, z_dim)
        self.fc_logvar = nn.Linear(1024 * 8 * 8, z_dim)
        dec, d = [nn.Linear(z_dim, 1024 * 8 * 8), _View((-1, 1024, 8, 8))], (1024, 512, 256, 128, 64, 32)
        for l in range(5):
            dec += [nn.ConvTranspose2d(d[l], d[l + 1], 4, 2, 1, bias=True), nn.BatchNorm2d(d[l + 1]), nn.ReLU(True)]
        self.decoder = nn.Sequential(*dec, nn.ConvTranspose2d(32, nc, 1))
        for seq in (self.encoder, self.decoder):
            for m in seq:
                _kaiming(m)

    def forward(self, imgs):
        x = torch.cat([F.interpolate(img.unsqueeze(0), (256, 256)) * 255 for img in imgs])
        h = self.encoder(x)
        mu, logvar = self.fc_mu(h), self.fc_logvar(h)
        z = torch.randn(*mu.size()).to(mu.device) * (0.5 * logvar).exp() + mu
        return self.decoder(z), z, mu, logvar


class Discriminator(nn.Module):
    """The VAAL adversary: Linear(z, 512) -> ReLU -> Linear(512, 512) -> ReLU -> Linear(512, 1) -> Sigmoid."""

    def __init__(self, z_dim=Z_DIM):
        super().__init__()
        self.z_dim = z_dim
        self.net = nn.Sequential(nn.Linear(z_dim, 512), nn.ReLU(True), nn.Linear(512, 512), nn.ReLU(True), nn.Linear(512, 1), nn.Sigmoid())
        for m in self.net:
            _kaiming(m)

    def forward(self, z):
        return self.net(z)


def _state(module_or_dict, keys):
    """{key: float32 array} of the tensors the sweep reads; whatever else the state holds (decoder, fc_logvar, ...) is left out."""
    sd = module_or_dict.state_dict() if hasattr(module_or_dict, "state_dict") else module_or_dict
    return {k: np.ascontiguousarray(v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, np.float32), dtype=np.float32)
            for k, v in sd.items() if k in keys}


def expected_shapes():
    """{key: shape} of every tensor the sweep reads."""
    out = {}
    for l in range(5):
        out["encoder.%d.weight" % (3 * l)] = (ENC_WIDTHS[l + 1], ENC_WIDTHS[l], 4, 4)
        out["encoder.%d.bias" % (3 * l)] = (ENC_WIDTHS[l + 1],)
        for p in ("weight", "bias", "running_mean", "running_var"):
            out["encoder.%d.%s" % (3 * l + 1, p)] = (ENC_WIDTHS[l + 1],)
    out.update({"fc_mu.weight": (Z_DIM, 65536), "fc_mu.bias": (Z_DIM,), "net.0.weight": (512, Z_DIM), "net.0.bias": (512,),
                "net.2.weight": (512, 512), "net.2.bias": (512,), "net.4.weight": (1, 512), "net.4.bias": (1,)})
    return out


def checked_state(vae, discriminator):
    """The tensors the sweep reads out of the two modules / dicts; KeyError for a missing one, ValueError for a mis-shaped one (the
    library checks the same at cald_vaal_finalize)."""
    state = dict(_state(vae, VAE_KEYS))
    state.update(_state(discriminator, DISC_KEYS))
    for k, shape in expected_shapes().items():
        if k not in state:
            raise KeyError("VAAL state lacks %s" % k)
        if tuple(state[k].shape) != shape:
            raise ValueError("%s is %s, expected %s" % (k, tuple(state[k].shape), shape))
    return state


class VaalModel:
    """The VAE's encoder + fc_mu and the discriminator mirrored on the HIP side (cald_vaal_*); a missing or mis-shaped tensor raises at
    construction.  bn_running: BatchNorm uses the running statistics (a module in eval()); a dict means training mode, as in the reference.
    Build it once to sweep several times with the same weights."""

    def __init__(self, vae, discriminator, ctx=None):
        self.h = None
        state = checked_state(vae, discriminator)
        from .detector import get_ctx
        self.ctx = ctx if ctx is not None else get_ctx()
        self.bn_running = hasattr(vae, "training") and not vae.training
        L = _ffi.lib()
        self.h = C.c_void_p()
        _ffi.check(L.cald_vaal_create(self.ctx, C.byref(self.h)))
        try:
            for k, a in state.items():
                shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
                _ffi.check(L.cald_vaal_load_tensor(self.h, k.encode(), _ffi.ptr(a), shape, a.ndim))
            _ffi.check(L.cald_vaal_finalize(self.h))
        except Exception:
            self.close()
            raise

    def close(self):
        if self.h is not None:
            _ffi.lib().cald_vaal_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vaal_sweep_device_images(vae, discriminator, images, batch_images=0, return_mu=False, bn_running=None):
    """Discriminator predictions float32 [n] of uint8 HWC CUDA tensors already resident in HBM (with return_mu also mu, float32 [n][256]).
    vae: a VaalModel (discriminator is then ignored), or the two modules / dicts.  bn_running overrides the mode taken from vae.training.
    batch_images: images per launch sequence (0 = 64; about 9 MB of scratch each); the results do not depend on it."""
    own = not isinstance(vae, VaalModel)
    model = VaalModel(vae, discriminator) if own else vae
    try:
        n = len(images)
        preds = np.zeros(n, np.float32)
        mu = np.zeros((n, Z_DIM), np.float32) if return_mu else None
        if n:
            for im in images:
                if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_cuda or not im.is_contiguous():
                    raise ValueError("images: contiguous uint8 [H][W][3] CUDA tensors")
            ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in images])
            Hs = np.array([im.shape[0] for im in images], np.int32)
            Ws = np.array([im.shape[1] for im in images], np.int32)
            running = model.bn_running if bn_running is None else bool(bn_running)
            cfg = _ffi.VaalCfg(_ffi.VAAL_BN_RUNNING if running else _ffi.VAAL_BN_BATCH, int(batch_images))
            torch.cuda.current_stream().synchronize()        # the images may still be on their way (non_blocking uploads)
            _ffi.check(_ffi.lib().cald_sweep_vaal(model.ctx, model.h, n, ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i), C.byref(cfg),
                                                  _ffi.ptr(preds), _ffi.ptr(mu) if return_mu else None))
    finally:
        if own:
            model.close()
    return (preds, mu) if return_mu else preds


def select_lowest(preds, budget):
    """Positions of the `budget` lowest predictions, lowest first; equal predictions in increasing position.  budget >= len(preds)
    returns every position."""
    preds = np.asarray(preds)
    order = np.argsort(preds, kind="stable")
    return order[:max(0, min(int(budget), len(preds)))].astype(np.int64)


def sample_for_labeling(vae, discriminator, unlabeled_loader, budget, rank=0, world_size=1, group=None, return_preds=False,
                        batch_images=0):
    """Drop-in for vaal_helper.py:219 (same positional signature): a numpy array of the loader positions of the `budget` images the
    discriminator holds most likely to be unlabeled -- the lowest predictions, lowest first.  Equal predictions are ordered by lower loader
    position; torch.topk, which the reference uses, leaves the order among exact ties unspecified.  vae / discriminator: torch modules with
    the reference's state_dict() keys, or dicts of arrays; BatchNorm follows vae.training (batch statistics of the one image in train(),
    running statistics in eval(); a dict means train(), the state the reference's sampler finds the VAE in).  Loader items are (images, _)
    with ONE image each, as the reference's index bookkeeping needs: PIL, uint8 HWC tensors or float CHW tensors in [0, 1].  world_size > 1:
    rank r scores the positions p % world_size == r and one all-gather (sweep.allgather_scores) returns every prediction on every rank.
    return_preds: also the float32 predictions in loader order."""
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    images, mine, n_pos = [], [], 0
    for pos, (imgs, _) in enumerate(unlabeled_loader):
        n_pos += 1
        if len(imgs) != 1:
            raise ValueError("loader item %d holds %d images: the VAAL sampler indexes loader positions and runs at loader batch 1" % (pos, len(imgs)))
        if pos % world_size != rank:
            continue
        mine.append(pos); images.append(_to_u8_cuda(imgs[0], dev))
    preds = vaal_sweep_device_images(vae, discriminator, images, batch_images)
    if world_size > 1:
        from . import sweep
        full, _ = sweep.allgather_scores(mine, preds.astype(np.float64), np.zeros((len(mine), 1), np.float64), n_pos, group)
        preds = np.asarray(full, np.float64).astype(np.float32)
    idx = select_lowest(preds, budget)
    return (idx, preds) if return_preds else idx


class AdversarySampler:
    """vaal_helper.py:186-216 for callers that use the class."""

    def __init__(self, budget):
        self.budget = budget

    def sample(self, vae, discriminator, dataloader, **kw):
        return sample_for_labeling(vae, discriminator, dataloader, self.budget, **kw)
