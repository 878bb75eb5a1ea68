"""Baseline active-learning sweeps of the same repo on the HIP detector.

``lt_c_get_uncertainty(task_model, unlabeled_loader)``  -- lt_c_train.py:105-121 (localization tightness + classification)
``ls_c_get_uncertainty(task_model, unlabeled_loader)``  -- ls_c_train.py:108-155 (localization stability + classification;
    six GaussianNoise views per image, torch.randn stream re-seeded per pool position like the CALD sweep)
Same positional signatures and return types (list of floats in loader order) as the reference functions.
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from .sweep import _to_u8_cuda


def _collect(unlabeled_loader):
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    images, positions = [], []
    for pos, (imgs, _) in enumerate(unlabeled_loader):
        for image in imgs:
            images.append(_to_u8_cuda(image, dev)); positions.append(pos)
    return images, positions


def _arrays(images):
    n = len(images)
    ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in images])
    Hs = np.array([im.shape[0] for im in images], np.int32)
    Ws = np.array([im.shape[1] for im in images], np.int32)
    return ptrs, Hs, Ws


def lt_c_get_uncertainty(task_model, unlabeled_loader, batch_images=64):
    task_model.eval()
    images, _ = _collect(unlabeled_loader)
    out = np.zeros(len(images), np.float64)
    if len(images):
        ptrs, Hs, Ws = _arrays(images)
        _ffi.check(_ffi.lib().cald_sweep_ltc(task_model.handle(), len(images), ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i),
                                             batch_images, _ffi.ptr(out, _ffi.c_d)))
    return [float(v) for v in out]


def ls_c_get_uncertainty(task_model, unlabeled_loader, aves=None, base_seed=0, batch_images=32):
    task_model.eval()
    images, positions = _collect(unlabeled_loader)
    out = np.zeros(len(images), np.float64)
    if len(images):
        ptrs, Hs, Ws = _arrays(images)
        pos = np.ascontiguousarray(positions, dtype=np.int64)
        _ffi.check(_ffi.lib().cald_sweep_lsc(task_model.handle(), len(images), ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i),
                                             _ffi.ptr(pos, _ffi.c_i64), int(base_seed), batch_images, _ffi.ptr(out, _ffi.c_d)))
    return [float(v) for v in out]


# ---- the learning-loss baseline (ll_train.py:145-166, ll4al/models/lossnet.py:31-65) ----
LOSSNET_KEYS = tuple("FC%d.%s" % (i, p) for i in range(1, 5) for p in ("weight", "bias")) + ("linear.weight", "linear.bias")


def ll_group_padding(sizes, groups, min_size, max_size):
    """[(Hp, Wp)] per image: the padded size of its loader batch, as torchvision's ImageList gives it -- the per-dimension maximum over
    the group's members of the detector transform's resized size (GeneralizedRCNNTransform: scale = min_size / min(H, W), capped so that
    max(H, W) * scale <= max_size; floor), rounded up to a multiple of 32.  sizes: [(H, W)], groups: the loader-batch id of each image."""
    import math

    def padded(H, W):
        scale = float(min_size) / float(min(H, W))
        if float(max(H, W)) * scale > float(max_size):
            scale = float(max_size) / float(max(H, W))
        return tuple((int(math.floor(float(d) * scale)) + 31) // 32 * 32 for d in (H, W))

    own = [padded(int(H), int(W)) for H, W in sizes]
    best = {}
    for g, (hp, wp) in zip(groups, own):
        b = best.get(g, (0, 0))
        best[g] = (max(b[0], hp), max(b[1], wp))
    return [best[g] for g in groups]


def _lossnet_state(ll_model):
    """{key: float32 array} of LossNet's ten tensors, from a module (state_dict()) or a dict."""
    sd = ll_model.state_dict() if hasattr(ll_model, "state_dict") else ll_model
    return {k: np.ascontiguousarray(v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, np.float32), dtype=np.float32)
            for k, v in sd.items() if k in LOSSNET_KEYS}


class _LossNet:
    """LossNet mirrored on the HIP side for the length of one call (cald_lossnet_*); a missing or mis-shaped tensor raises at finalize."""

    def __init__(self, ctx, state):
        L = _ffi.lib()
        self.h = C.c_void_p()
        _ffi.check(L.cald_lossnet_create(ctx, C.byref(self.h)))
        try:
            for k, a in state.items():
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _ffi.check(L.cald_lossnet_load_tensor(self.h, k.encode(), _ffi.ptr(a), shape, a.ndim))
            _ffi.check(L.cald_lossnet_finalize(self.h))
        except Exception:
            self.close()
            raise

    def close(self):
        if self.h is not None:
            _ffi.lib().cald_lossnet_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def lossnet_scores(ll_model, pooled, ctx=None):
    """LossNet on pooled vectors [n][4][256] (cald_op_lossnet): float32 [n]."""
    from .detector import get_ctx
    pooled = np.ascontiguousarray(pooled, np.float32).reshape(-1, 4, 256)
    out = np.zeros(pooled.shape[0], np.float32)
    with _LossNet(ctx if ctx is not None else get_ctx(), _lossnet_state(ll_model)) as ln:
        _ffi.check(_ffi.lib().cald_op_lossnet(ln.h, pooled.shape[0], _ffi.ptr(pooled), _ffi.ptr(out)))
    return out


def ll_sweep_device_images(task_model, ll_model, images, groups, levels=None, batch_views=0, return_pooled=False):
    """Scores uint8 HWC CUDA tensors already resident in HBM; groups[i] = loader-batch id of image i (non-decreasing).  Returns the
    float64 scores [n] (float32 values) and, with return_pooled, the pooled vectors [n][4][256] float32."""
    from .detector import get_ctx
    n = len(images)
    out = np.zeros(n, np.float64)
    pooled = np.zeros((n, 4, 256), np.float32) if return_pooled else None
    if levels is None:
        levels = (0, 0, 0, 0) if task_model.arch == 1 else (0, 1, 2, 3)      # ll_train.py:155-161: features[0] four times for RetinaNet
    if len(levels) != 4:
        raise ValueError("levels: one pyramid index per LossNet branch (4)")
    state = _lossnet_state(ll_model)
    handle = task_model.handle()
    ctx = task_model._ctx if getattr(task_model, "_ctx", None) is not None else get_ctx(task_model._device)
    with _LossNet(ctx, state) as ln:
        if n:
            ptrs, Hs, Ws = _arrays(images)
            grp = np.ascontiguousarray(groups, dtype=np.int32)
            cfg = _ffi.LLCfg(int(batch_views), (C.c_int * 4)(*[int(l) for l in levels]))
            _ffi.check(_ffi.lib().cald_sweep_ll(handle, ln.h, n, ptrs, _ffi.ptr(Hs, _ffi.c_i), _ffi.ptr(Ws, _ffi.c_i), _ffi.ptr(grp, _ffi.c_i),
                                                C.byref(cfg), _ffi.ptr(out, _ffi.c_d), _ffi.ptr(pooled) if return_pooled else None))
    return (out, pooled) if return_pooled else out


def ll_pack_rows(batch_scores, width):
    """One float64 row of `width` columns per loader batch, NaN-padded: the rows the multi-rank sweep sends through
    sweep.allgather_scores (first column as `cons`, the rest as `cls`)."""
    rows = np.full((len(batch_scores), width), np.nan, np.float64)
    for r, s in enumerate(batch_scores):
        rows[r, :len(s)] = s
    return rows


def ll_unpack_rows(first, rest):
    """The scores in loader order out of gathered rows (first column, remaining columns): the NaN padding is dropped."""
    rows = np.concatenate([np.asarray(first, np.float64).reshape(-1, 1), np.asarray(rest, np.float64).reshape(len(first), -1)], axis=1)
    return rows[~np.isnan(rows)]


def ll_get_uncertainty(task_model, ll_model, unlabeled_loader, levels=None, batch_views=0, rank=0, world_size=1, group=None,
                       return_pooled=False):
    """Drop-in for ll_train.py:145 (same positional signature): a float32 CPU tensor in loader order.  Every loader item is one loader
    batch; its images are padded to their common size, so -- as in the reference -- an image's score depends on its batch.  ll_model: a
    torch module whose state_dict() has LossNet's keys, or such a dict.  levels: pyramid index per LossNet branch (default: the reference
    as shipped, (0, 1, 2, 3) for Faster R-CNN and (0, 0, 0, 0) for RetinaNet).  world_size > 1: rank r scores the loader batches
    b % world_size == r, and one all-gather (sweep.allgather_scores) returns the full vector on every rank; the loader's batch size must
    then be the same on every rank.  return_pooled (single rank): also the pooled vectors, float32 [n][4][256]."""
    if not hasattr(task_model, "handle"):          # the reference's torch model: mirror it on the HIP side
        from .detector import from_torch_module
        task_model = from_torch_module(task_model)
    task_model.eval()
    if hasattr(ll_model, "eval"):
        ll_model.eval()
    if return_pooled and world_size > 1:
        raise ValueError("return_pooled is a single-rank option")
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    images, groups, sizes, mine = [], [], [], []
    n_batches = 0
    for b, (imgs, _) in enumerate(unlabeled_loader):
        n_batches += 1
        if b % world_size != rank:
            continue
        mine.append(b); sizes.append(len(imgs))
        for image in imgs:
            images.append(_to_u8_cuda(image, dev)); groups.append(b)
    res = ll_sweep_device_images(task_model, ll_model, images, groups, levels, batch_views, return_pooled)
    scores = res[0] if return_pooled else res
    if world_size > 1:
        from . import sweep
        import torch.distributed as dist
        backend = dist.get_backend(group)
        t = torch.tensor([max(sizes) if sizes else 1], dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        width = max(2, int(t.item()))                  # allgather_scores wants at least one `cls` column
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        rows = ll_pack_rows([scores[off[k]:off[k + 1]] for k in range(len(sizes))], width)
        first, rest = sweep.allgather_scores(mine, rows[:, 0], rows[:, 1:], n_batches, group)
        scores = ll_unpack_rows(first, rest)
    out = torch.from_numpy(np.asarray(scores, np.float64).astype(np.float32))
    return (out, res[1]) if return_pooled else out
