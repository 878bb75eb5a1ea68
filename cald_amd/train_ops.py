"""Thin wrappers of the cald_train_* device operators (include/cald_hip.h, cald_amd/csrc/train_*.hip) on torch CUDA tensors.

torch supplies device memory and the stream only; every arithmetic step is a libcaldhip kernel.  Activations are NHWC
float32 [N, H, W, C].  No fallback: without the library or an MI355X every call raises.
"""
import contextlib
import ctypes as C

import torch

from . import _ffi
from .detector import get_ctx

FLAG_BIAS, FLAG_BN, FLAG_RELU = 1, 2, 4


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_WGRAD_CTX = [None]     # set by train.py while weight gradients / weight packing / target matching are issued on another stream


def _wctx(t):
    return _WGRAD_CTX[0] if _WGRAD_CTX[0] is not None else get_ctx(t.device.index)


def _chk(t, name):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), name


def round_up(x, m):
    return (x + m - 1) // m * m


def packed_floats(Cout, Cin, KH, KW, CinK, mode):
    n = C.c_int64()
    _ffi.check(_ffi.lib().cald_train_packed_floats(Cout, Cin, KH, KW, CinK, mode, C.byref(n)))
    return int(n.value)


def f16x3_scale(max_abs):
    """(S, unscale) of a layer whose largest |weight| is max_abs: the scale policy of an inference model's finalize (cald_train_f16x3_scale)."""
    S, u = C.c_int(), C.c_float()
    _ffi.check(_ffi.lib().cald_train_f16x3_scale(float(max_abs), C.byref(S), C.byref(u)))
    return int(S.value), float(u.value)


def packed16_bytes(Cout, Cin, KH, KW, CinK, mode):
    """Bytes of a forward pack's split twin; 0 for a shape the split-fp16 kernels do not take."""
    n = C.c_int64()
    _ffi.check(_ffi.lib().cald_train_packed16_bytes(Cout, Cin, KH, KW, CinK, mode, C.byref(n)))
    return int(n.value)


def packed_grad16_bytes(Cout, Cin, KH, KW, CinK, mode):
    """Bytes of a data-gradient pack's split twin; 0 where conv_h3 does not take the data gradient's shape."""
    n = C.c_int64()
    _ffi.check(_ffi.lib().cald_train_packed_grad16_bytes(Cout, Cin, KH, KW, CinK, mode, C.byref(n)))
    return int(n.value)


def f16x3_grad_scale(max_abs):
    """(G, in_scale) of a gradient tensor whose largest |entry| is max_abs (cald_train_f16x3_grad_scale): in_scale = 2^(4 + G) places that
    maximum in [2^10, 2^11) before conv_h3 splits it; G is clamped to +-60 and 0 for an all-zero or non-finite tensor."""
    G, s = C.c_int(), C.c_float()
    _ffi.check(_ffi.lib().cald_train_f16x3_grad_scale(float(max_abs), C.byref(G), C.byref(s)))
    return int(G.value), float(s.value)


_KERNEL_LOG = [None]    # a list while record_kernels() is open: (layer, kernel) of every forward conv / linear launch


@contextlib.contextmanager
def record_kernels():
    """Collects (layer shape, kernel that took the launch) of every forward conv / linear issued inside the block."""
    prev, log = _KERNEL_LOG[0], []
    _KERNEL_LOG[0] = log
    try:
        yield log
    finally:
        _KERNEL_LOG[0] = prev


_DGRAD_LOG = [None]     # a list while record_dgrad_kernels() is open: (layer, kernel) of every data-gradient launch


@contextlib.contextmanager
def record_dgrad_kernels():
    """Collects (layer shape, kernel that took the launch) of every data gradient issued through conv / conv_dgrad / conv_group inside the
    block (record_kernels() logs forward launches only)."""
    prev, log = _DGRAD_LOG[0], []
    _DGRAD_LOG[0] = log
    try:
        yield log
    finally:
        _DGRAD_LOG[0] = prev


class PackedConv(object):
    """A torch-layout weight [Cout, Cin, KH, KW] (+ bias / frozen-BN scale, shift) in the layout the MFMA kernels read.  w16_S (forward
    packs): also its split-fp16 twin at weight scale 2^w16_S for conv_h3 / conv_h4 -- self.w16 stays None where those take no such shape.
    grad16_S (data-gradient packs, modes 1 / 3): the twin of the fp32 pack's values (transposed, flipped, `scale` folded in) at weight scale
    2^grad16_S, which conv(..., G=) / conv_dgrad / conv_group read -- None where conv_h3 does not take the data gradient's shape."""

    def __init__(self, weight, bias=None, scale=None, shift=None, CinK=None, mode=0, taps=None, out=None, pack=True, w16_S=None, w16_out=None,
                 grad16_S=None):
        _chk(weight, "weight")
        if mode in (2, 3):                               # linear on [tap][Cin] rows, torch weight [Cout, Cin * taps] (3: its data gradient)
            self.Cout, self.Cin, self.KH, self.KW = weight.shape[0], weight.shape[1] // taps, taps, 1
            CinK = self.Cin if mode == 2 else (CinK if CinK is not None else round_up(self.Cout, 4))
        elif weight.dim() == 2:                          # plain linear layer = 1x1 conv
            self.Cout, self.Cin, self.KH, self.KW = weight.shape[0], weight.shape[1], 1, 1
        else:
            self.Cout, self.Cin, self.KH, self.KW = weight.shape
        self.mode = mode
        self.CinK = CinK if CinK is not None else (round_up(self.Cout, 4) if mode == 1 else self.Cin)
        n = packed_floats(self.Cout, self.Cin, self.KH, self.KW, self.CinK, mode)
        self.buf = out if out is not None else torch.empty(n, dtype=torch.float32, device=weight.device)
        assert self.buf.numel() >= n
        # gradient packs (modes 1, 3) carry no epilogue vectors: a scale given there is folded into the filter rows
        self.flags = ((FLAG_BIAS if bias is not None else 0) | (FLAG_BN if scale is not None else 0)) if mode in (0, 2) else 0
        # what a PackPlan needs to repeat this pack (the tensors are kept alive: the plan holds their device pointers)
        self.src = (weight, bias, scale, shift)
        self.w16, self.w16_S, self.w16_unscale = None, 0, 1.0
        if w16_S is not None and mode in (0, 2):
            nb = packed16_bytes(self.Cout, self.Cin, self.KH, self.KW, self.CinK, mode)
            if nb:
                self.w16 = w16_out if w16_out is not None else torch.empty(nb // 2, dtype=torch.int16, device=weight.device)
                assert self.w16.numel() * 2 >= nb
                self.w16_S, self.w16_unscale = int(w16_S), 2.0 ** -(int(w16_S) + 4)
        if grad16_S is not None and mode in (1, 3):
            nb = packed_grad16_bytes(self.Cout, self.Cin, self.KH, self.KW, self.CinK, mode)
            if nb:
                self.w16 = w16_out if w16_out is not None else torch.empty(nb // 2, dtype=torch.int16, device=weight.device)
                assert self.w16.numel() * 2 >= nb
                self.w16_S = int(grad16_S)          # (the launch's unscale also undoes the gradient's scale: 2^-(S + 4 + G), per launch)
        if pack and self.w16 is not None:
            _ffi.check(_ffi.lib().cald_train_pack_conv16(_wctx(weight), _p(weight), _p(bias), _p(scale), _p(shift), self.Cout, self.Cin, self.KH,
                                                         self.KW, self.CinK, mode, _p(self.buf), _p(self.w16), self.w16_S))
        elif pack:
            _ffi.check(_ffi.lib().cald_train_pack_conv(_wctx(weight), _p(weight), _p(bias), _p(scale), _p(shift), self.Cout,
                                                       self.Cin, self.KH, self.KW, self.CinK, mode, _p(self.buf)))

    def job(self):
        w, b, sc, sh = self.src
        q = _ffi.PackJob()
        q.weight, q.bias, q.bn_scale, q.bn_shift = [t.data_ptr() if t is not None else None for t in (w, b, sc, sh)]
        q.Cout, q.Cin, q.KH, q.KW, q.CinK, q.mode, q.packed = self.Cout, self.Cin, self.KH, self.KW, self.CinK, self.mode, self.buf.data_ptr()
        if self.w16 is not None:
            q.w16, q.w16_S = self.w16.data_ptr(), self.w16_S
        return q


class PackPlan(object):
    """All of a model's PackedConv buffers re-packed in two launches (cald_train_pack_plan_*): after an optimizer step every trainable
    weight has changed, and one cald_train_pack_conv per layer and form is ~220 launches of a few microseconds each."""

    def __init__(self, packs, device):
        self.packs = list(packs)                         # keeps weights and packed buffers alive
        n = len(self.packs)
        self.jobs = (_ffi.PackJob * n)(*[pk.job() for pk in self.packs])
        need = C.c_int64()
        _ffi.check(_ffi.lib().cald_train_pack_plan_scratch_floats(n, self.jobs, C.byref(need)))
        self.scratch = torch.empty(max(int(need.value), 1), dtype=torch.float32, device=device)
        self.handle = C.c_void_p()
        # (the context whose stream run() will use: the scratch is zeroed on that stream)
        _ffi.check(_ffi.lib().cald_train_pack_plan_create(_wctx(self.scratch), n, self.jobs, _p(self.scratch), int(need.value),
                                                          C.byref(self.handle)))

    def run(self):
        _ffi.check(_ffi.lib().cald_train_pack_plan_run(_wctx(self.scratch), self.handle))

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                _ffi.lib().cald_train_pack_plan_destroy(h)
            except Exception:
                pass


def _layer_label(pk, x, stride):
    kind = "linear" if pk.mode == 2 or (pk.KH == 1 and x.shape[0] == 1 and x.shape[1] == 1) else "conv"
    return "%s %dx%d/%d %d->%d on %dx%dx%d" % (kind, pk.KH, pk.KW, stride, pk.Cin, pk.Cout, x.shape[0], x.shape[1], x.shape[2])


def _dgrad_label(pk, x):
    return "dgrad %dx%d %d<-%d on %dx%dx%d" % (pk.KH if pk.mode == 1 else 1, pk.KW if pk.mode == 1 else 1, pk.Cin * (pk.KH if pk.mode == 3 else 1),
                                                pk.Cout, x.shape[0], x.shape[1], x.shape[2])


def conv(x, pk, stride=1, pad=0, relu=False, residual=None, up=None, out=None, out_ld=None, mask=None, x16=None, ex16=None, split_out=False, G=None):
    """Forward conv / linear (pk.mode 0 or 2) or stride-1 data gradient (pk.mode 1) of a dense NHWC batch.  A pack with a split twin
    (pk.w16) runs on the split-fp16 kernels where they take the launch.  Such a launch may use split twins of activations (int32 tensors of
    the fp32 tensor's shape, the layout of an inference model of precision "f16x3"): x16 = the twin of x, ex16 = the twin of residual / up
    -- the sum then takes the 22-bit value that model adds -- and split_out=True makes it write its output's twin: it returns (out, twin).
    G (data-gradient packs with a twin, PackedConv(grad16_S=)): the gradient exponent of x (f16x3_grad_scale) -- the launch runs on conv_h3
    with x staged at 2^(4 + G); None: the exact kernels."""
    _chk(x, "x")
    N, H, W, Cx = x.shape
    n_out = pk.Cin if pk.mode == 1 else (pk.Cin * pk.KH if pk.mode == 3 else pk.Cout)
    if pk.mode == 2:
        assert Cx == pk.Cin * pk.KH
        kh = kw = 1
    elif pk.mode == 3:
        assert Cx == pk.CinK
        kh = kw = 1
    else:
        assert Cx == pk.CinK, (Cx, pk.CinK)
        kh, kw = pk.KH, pk.KW
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    ld = out_ld if out_ld is not None else n_out
    if out is None:
        out = (torch.zeros if ld != n_out else torch.empty)((N, Ho, Wo, ld), dtype=torch.float32, device=x.device)
    Hup, Wup = (up.shape[1], up.shape[2]) if up is not None else (0, 0)
    flags = pk.flags | (FLAG_RELU if relu else 0)
    if (x16 is not None or ex16 is not None or split_out) and pk.w16 is None:
        raise ValueError("split activations need a pack with a split twin")
    log = _KERNEL_LOG[0] if pk.mode in (0, 2) else None
    if pk.mode in (1, 3):
        dlog = _DGRAD_LOG[0]
        name = C.c_char_p()
        if pk.w16 is not None and G is not None:
            assert stride == 1 and up is None
            _ffi.check(_ffi.lib().cald_train_conv_dgrad_f16x3(_wctx(x), N, H, W, _p(x), pk.CinK, _p(pk.buf), pk.Cout, pk.Cin, pk.KH, pk.KW, pad, pk.mode,
                                                              _p(residual), _p(mask), _p(out), ld, _p(pk.w16), 2.0 ** -(pk.w16_S + 4 + int(G)),
                                                              2.0 ** (4 + int(G)), C.byref(name)))
        elif dlog is not None:                           # the exact kernels, with the name of the one that took the launch
            _ffi.check(_ffi.lib().cald_train_conv_f16x3(_wctx(x), N, H, W, _p(x), pk.CinK, _p(pk.buf), pk.Cout, pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode,
                                                        flags, _p(residual), _p(up), Hup, Wup, _p(mask), _p(out), ld, None, 1.0, None, 0, None, C.byref(name)))
        else:
            _ffi.check(_ffi.lib().cald_train_conv(_wctx(x), N, H, W, _p(x), pk.CinK, _p(pk.buf), pk.Cout,
                                                  pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode, flags, _p(residual), _p(up), Hup, Wup, _p(mask), _p(out), ld))
        if dlog is not None:
            dlog.append((_dgrad_label(pk, x), name.value.decode()))
        return out
    if pk.w16 is None and log is None:
        _ffi.check(_ffi.lib().cald_train_conv(_wctx(x), N, H, W, _p(x), pk.CinK, _p(pk.buf), pk.Cout,
                                              pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode, flags, _p(residual), _p(up), Hup, Wup, _p(mask), _p(out), ld))
        return out
    ex = residual if residual is not None else up
    if ex16 is not None and (ex is None or (residual is not None and up is not None) or ex16.shape != ex.shape):
        raise ValueError("ex16 is the twin of ONE addend, residual or up, of that addend's shape")
    if x16 is not None and x16.shape != x.shape:
        raise ValueError("x16 must have the shape of x")
    out16 = torch.empty(out.shape, dtype=torch.int32, device=out.device) if split_out else None
    # (the epilogue reads ONE tensor: with ex16 the residual / up pointer is the twin's)
    res_p, up_p = (_p(ex16) if residual is not None else None, _p(ex16) if up is not None else None) if ex16 is not None else (_p(residual), _p(up))
    name = C.c_char_p()
    _ffi.check(_ffi.lib().cald_train_conv_f16x3(_wctx(x), N, H, W, _p(x), pk.CinK, _p(pk.buf), pk.Cout, pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode,
                                                flags, res_p, up_p, Hup, Wup, _p(mask), _p(out), ld, _p(pk.w16), pk.w16_unscale, _p(x16),
                                                int(ex16 is not None), _p(out16), C.byref(name)))
    if log is not None:
        log.append((_layer_label(pk, x, stride), name.value.decode()))
    return (out, out16) if split_out else out


def conv_group(xs, pks, stride=1, pad=0, relu=False, outs=None, out_ld=None, masks=None, xs16=None, Gs=None):
    """The same layer shape on several NHWC tensors in one launch; pks: one PackedConv per tensor (all of one shape) or a single one.
    xs16 (packs with split twins only): the split twins of xs, one per tensor (see conv).  Gs (data-gradient packs with twins): one gradient
    exponent per tensor (see conv); None: the exact kernels."""
    if not isinstance(pks, (list, tuple)):
        pks = [pks] * len(xs)
    pk = pks[0]
    n_out = pk.Cin if pk.mode == 1 else pk.Cout
    ld = out_ld if out_ld is not None else n_out
    res = []
    for i, x in enumerate(xs):
        _chk(x, "x")
        assert x.shape[3] == pk.CinK and x.shape[0] == xs[0].shape[0]
        Ho, Wo = (x.shape[1] + 2 * pad - pk.KH) // stride + 1, (x.shape[2] + 2 * pad - pk.KW) // stride + 1
        o = outs[i] if outs is not None else (torch.zeros if ld != n_out else torch.empty)((x.shape[0], Ho, Wo, ld), dtype=torch.float32, device=x.device)
        res.append(o)
    hw = [v for x in xs for v in (x.shape[1], x.shape[2])]
    flags = pk.flags | (FLAG_RELU if relu else 0)
    log = _KERNEL_LOG[0] if pk.mode in (0, 2) else None
    split = all(p.w16 is not None for p in pks)
    if pk.mode in (1, 3):
        dlog = _DGRAD_LOG[0]
        names = (C.c_char_p * len(xs))()
        mk = _ptr_array(masks) if masks is not None else None
        if split and Gs is not None:
            assert stride == 1 and len(Gs) == len(xs)
            uns = (C.c_float * len(xs))(*[2.0 ** -(p.w16_S + 4 + int(G)) for p, G in zip(pks, Gs)])
            ins = (C.c_float * len(xs))(*[2.0 ** (4 + int(G)) for G in Gs])
            _ffi.check(_ffi.lib().cald_train_conv_dgrad_group_f16x3(_wctx(xs[0]), len(xs), xs[0].shape[0], _int_array(hw), _ptr_array(xs), pk.CinK,
                                                                    _ptr_array([p.buf for p in pks]), pk.Cout, pk.Cin, pk.KH, pk.KW, pad, pk.mode, mk,
                                                                    _ptr_array(res), ld, _ptr_array([p.w16 for p in pks]), uns, ins, names))
        elif dlog is not None:
            _ffi.check(_ffi.lib().cald_train_conv_group_f16x3(_wctx(xs[0]), len(xs), xs[0].shape[0], _int_array(hw), _ptr_array(xs), pk.CinK,
                                                              _ptr_array([p.buf for p in pks]), pk.Cout, pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode, flags,
                                                              mk, _ptr_array(res), ld, None, None, None, names))
        else:
            _ffi.check(_ffi.lib().cald_train_conv_group(_wctx(xs[0]), len(xs), xs[0].shape[0], _int_array(hw), _ptr_array(xs), pk.CinK,
                                                        _ptr_array([p.buf for p in pks]), pk.Cout, pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode, flags,
                                                        mk, _ptr_array(res), ld))
        if dlog is not None:
            dlog.extend((_dgrad_label(p, x), nm.decode()) for p, x, nm in zip(pks, xs, names))
        return res
    if not split and log is None:
        _ffi.check(_ffi.lib().cald_train_conv_group(_wctx(xs[0]), len(xs), xs[0].shape[0], _int_array(hw), _ptr_array(xs), pk.CinK,
                                                    _ptr_array([p.buf for p in pks]), pk.Cout, pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode, flags,
                                                    _ptr_array(masks) if masks is not None else None, _ptr_array(res), ld))
        return res
    if xs16 is not None and (not split or len(xs16) != len(xs) or any(t.shape != x.shape for t, x in zip(xs16, xs))):
        raise ValueError("xs16: one twin of its tensor's shape per tensor, and packs with split twins")
    w16 = uns = in16 = None
    if split:
        w16, uns = _ptr_array([p.w16 for p in pks]), (C.c_float * len(pks))(*[p.w16_unscale for p in pks])
        in16 = _ptr_array(xs16) if xs16 is not None else None
    names = (C.c_char_p * len(xs))()
    _ffi.check(_ffi.lib().cald_train_conv_group_f16x3(_wctx(xs[0]), len(xs), xs[0].shape[0], _int_array(hw), _ptr_array(xs), pk.CinK,
                                                      _ptr_array([p.buf for p in pks]), pk.Cout, pk.Cin, pk.KH, pk.KW, stride, pad, pk.mode, flags,
                                                      _ptr_array(masks) if masks is not None else None, _ptr_array(res), ld, w16, uns, in16, names))
    if log is not None:
        log.extend((_layer_label(p, x, stride), nm.decode()) for p, x, nm in zip(pks, xs, names))
    return res


def dilate(g, s, Hd, Wd):
    N, Ho, Wo, Cc = g.shape
    out = torch.empty((N, Hd, Wd, Cc), dtype=torch.float32, device=g.device)
    _ffi.check(_ffi.lib().cald_train_dilate(_wctx(g), N, Ho, Wo, Cc, s, Hd, Wd, _p(g), _p(out)))
    return out


def conv_dgrad(g, pk_d, H, W, stride, pad, residual=None, mask=None, G=None):
    """dX [N, H, W, Cin] of a conv whose forward had (stride, pad); g [N, Ho, Wo, CinK(pk_d)], pk_d packed with mode 1.  G: see conv."""
    K = pk_d.KH
    if stride > 1 and K == 1 and pk_d.KW == 1 and pad == 0 and residual is None and mask is None:
        # strided 1x1 (the bottleneck's downsample path): only every stride-th input pixel receives a gradient -- multiply on the
        # coarse grid and scatter the result, instead of scattering dY first and multiplying 3/4 zeros
        return dilate(conv(g, pk_d, G=G), stride, H, W)
    if stride > 1:
        g = dilate(g, stride, H + 2 * pad - K + 1, W + 2 * pad - pk_d.KW + 1)
    out = conv(g, pk_d, stride=1, pad=K - 1 - pad, residual=residual, mask=mask, G=G)
    assert out.shape[1] == H and out.shape[2] == W, (out.shape, H, W)
    return out


def conv_wgrad(x, g, Cin, Cout, KH, KW, stride, pad, dw, db=None, accumulate=False, row_scale=None):
    _chk(x, "x"); _chk(g, "g")
    N, H, W, ldx = x.shape
    _ffi.check(_ffi.lib().cald_train_conv_wgrad(_wctx(x), N, H, W, _p(x), Cin, ldx, _p(g), Cout, g.shape[-1], KH, KW, stride,
                                                pad, _p(row_scale), _p(dw), _p(db), int(accumulate)))
    return dw


def linear_wgrad(x, g, Cout, dw, db=None, taps=1, accumulate=False):
    _chk(x, "x"); _chk(g, "g")
    R, K = x.shape[0], x[0].numel()
    _ffi.check(_ffi.lib().cald_train_linear_wgrad(_wctx(x), R, _p(x), K, _p(g), Cout, g.shape[-1], taps, _p(dw), _p(db),
                                                  int(accumulate)))
    return dw


def conv_wgrad_plan(N, H, W, Cin, ldx, Cout, ldg, KH, KW, stride, pad):
    """The launch plan conv_wgrad takes for this shape (kernel variant, splits, reduction): a host query, nothing runs."""
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    pl = _ffi.WgradPlan()
    _ffi.check(_ffi.lib().cald_train_wgrad_plan(N * Ho * Wo, N, H, W, Cin, ldx, Cout, ldg, KH, KW, stride, pad, KH * KW, C.byref(pl)))
    return pl


def linear_wgrad_plan(R, K, Cout, ldg, taps=1):
    """The launch plan linear_wgrad takes for this shape."""
    pl = _ffi.WgradPlan()
    _ffi.check(_ffi.lib().cald_train_wgrad_plan(R, 1, 1, R, K, K, Cout, ldg, 1, 1, 1, 0, taps, C.byref(pl)))
    return pl


def relu_bwd_(g, act=None, scale=None):
    Cc = g.shape[-1]
    _ffi.check(_ffi.lib().cald_train_relu_bwd(_wctx(g), g.numel() // Cc, Cc, _p(g), _p(act), _p(scale)))
    return g


def add(a, b=None, out=None):
    out = out if out is not None else torch.empty_like(a)
    _ffi.check(_ffi.lib().cald_train_add(_wctx(a), a.numel(), _p(out), _p(a), _p(b)))
    return out


def upsample_bwd_(fine, coarse):
    N, Hf, Wf, Cc = fine.shape
    _ffi.check(_ffi.lib().cald_train_upsample_bwd(_wctx(fine), N, Hf, Wf, coarse.shape[1], coarse.shape[2], Cc, _p(fine), _p(coarse)))
    return coarse


def sgd_(param, grad, buf, lr, momentum, weight_decay, first_step):
    _ffi.check(_ffi.lib().cald_train_sgd(_wctx(param), param.numel(), _p(param), _p(grad), _p(buf), lr, momentum, weight_decay,
                                         int(first_step)))


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _int_array(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


def rpn_proposals(heads, Hp, Wp, image_sizes, pre_n=2000, post_n=2000, nms_thr=0.7, min_size=1e-3):
    """heads: five [N, Hl, Wl, 16] tensors (3 logits + 12 deltas + 1 pad).  Returns (proposals [N, post_n, 4], counts [N] int32)."""
    N = heads[0].shape[0]
    dev = heads[0].device
    props = torch.zeros((N, post_n, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(N, dtype=torch.int32, device=dev)
    hw = [v for h in heads for v in (h.shape[1], h.shape[2])]
    _ffi.check(_ffi.lib().cald_train_rpn_proposals(get_ctx(dev.index), N, Hp, Wp, _int_array([v for s in image_sizes for v in s]), _ptr_array(heads),
                                                   _int_array(hw), heads[0].shape[3], pre_n, post_n, nms_thr, min_size, _p(props), _p(counts)))
    return props, counts


def anchors(Hp, Wp, level_hw, device, kind=0):
    """kind 0: Faster R-CNN (3 per location), 1: RetinaNet (9 per location)."""
    n = sum(h * w * (9 if kind else 3) for h, w in level_hw)
    out = torch.empty((n, 4), dtype=torch.float32, device=device)
    _ffi.check(_ffi.lib().cald_train_anchors(get_ctx(device.index), kind, Hp, Wp, _int_array([v for s in level_hw for v in s]), _p(out)))
    return out


def match(boxes, gt, hi, lo, allow_low_quality, out=None):
    if out is None:
        out = torch.empty(boxes.shape[0], dtype=torch.int32, device=boxes.device)
    assert boxes.is_contiguous() and out.is_contiguous()
    _ffi.check(_ffi.lib().cald_train_match(_wctx(boxes), boxes.shape[0], _p(boxes), gt.shape[0], _p(gt), hi, lo, int(allow_low_quality),
                                           _p(out), None))
    return out


def roi_sample_host(slots, n_gt, counts, matched, gt_labels_cat, keys, batch, pos_fraction, pred_ld, num_classes, out=None):
    """cald_train_roi_sample_host: RoI labels + balanced sampling + loss index lists of a whole batch on the host, one call.
    slots / n_gt: sequences or ctypes int arrays; counts: None, a sequence, or an int32 numpy view (the device's counts as copied back).
    out: int64 numpy array of 6 * N * batch elements (e.g. pinned memory) that receives the six lists with stride cap = N * batch:
    table rows | ground-truth rows | labels | pred_idx | pos_rows | image index (float32 in the first 4 R bytes).
    Returns (out, cap, R, n_pos, RoIs per image)."""
    import numpy as np
    N = len(slots)
    cap = N * int(batch)
    assert matched.dtype == np.int32 and matched.flags.c_contiguous and keys.dtype == np.float64 and gt_labels_cat.dtype == np.int64
    if out is None:
        out = np.empty(6 * cap, np.int64)
    assert out.dtype == np.int64 and out.size >= 6 * cap and out.flags.c_contiguous
    R, n_pos, per = C.c_int(), C.c_int(), (C.c_int * N)()
    base = out.ctypes.data
    if counts is None:
        cp = None
    elif isinstance(counts, np.ndarray):
        assert counts.dtype == np.int32 and counts.size >= N
        cp = C.cast(C.c_void_p(counts.ctypes.data), C.POINTER(C.c_int))
    else:
        cp = _int_array(counts)
    ia = lambda v: v if isinstance(v, C.Array) else _int_array(v)
    _ffi.check(_ffi.lib().cald_train_roi_sample_host(N, ia(slots), ia(n_gt), cp, C.c_void_p(matched.ctypes.data), C.c_void_p(gt_labels_cat.ctypes.data),
                                                     C.c_void_p(keys.ctypes.data), int(batch), float(pos_fraction), int(pred_ld), int(num_classes),
                                                     C.c_void_p(base), C.c_void_p(base + 8 * cap), C.c_void_p(base + 16 * cap), C.c_void_p(base + 40 * cap),
                                                     C.c_void_p(base + 32 * cap), C.c_void_p(base + 24 * cap), C.byref(R), C.byref(n_pos), per))
    return out, cap, int(R.value), int(n_pos.value), list(per)


def roi_gather(table, gts_all, idx_dev, cap, R, n_pos, weights):
    """cald_train_roi_gather: RoIAlign rows [R, 5] and the foreground rows' regression targets [n_pos, 4] from the uploaded sampler block."""
    rois = torch.empty((R, 5), dtype=torch.float32, device=table.device)
    box_tgt = torch.empty((n_pos, 4), dtype=torch.float32, device=table.device)
    _ffi.check(_ffi.lib().cald_train_roi_gather(_wctx(table), _p(table), _p(gts_all), _p(idx_dev), int(cap), int(R), int(n_pos),
                                                *[float(w) for w in weights], _p(rois), _p(box_tgt)))
    return rois, box_tgt


def box_encode(reference, proposals, weights):
    out = torch.empty_like(proposals)
    _ffi.check(_ffi.lib().cald_train_box_encode(_wctx(proposals), proposals.shape[0], _p(reference), _p(proposals), *[float(w) for w in weights],
                                                _p(out)))
    return out


def roi_align(feats, rois):
    """feats: four [N, Hl, Wl, C]; rois [R, 5] (image index, box).  Returns [R, 49, C]."""
    R, Cc = rois.shape[0], feats[0].shape[3]
    out = torch.empty((R, 49, Cc), dtype=torch.float32, device=rois.device)
    hw = [v for f in feats for v in (f.shape[1], f.shape[2])]
    _ffi.check(_ffi.lib().cald_train_roi_align(_wctx(rois), _ptr_array(feats), _int_array(hw), Cc, R, _p(rois), _p(out)))
    return out


def roi_align_bwd_(gfeats, rois, gout):
    hw = [v for f in gfeats for v in (f.shape[1], f.shape[2])]
    _ffi.check(_ffi.lib().cald_train_roi_align_bwd(_wctx(rois), gfeats[0].shape[0], _ptr_array(gfeats), _int_array(hw), gfeats[0].shape[3],
                                                   rois.shape[0], _p(rois), _p(gout)))
    return gfeats


def softmax_ce(logits, labels, Ccls, grad=None, gscale=1.0):
    """logits [R, ld] (first Ccls columns are the class logits), labels int64 [R].  Returns the loss as a 1-element tensor."""
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    _ffi.check(_ffi.lib().cald_train_softmax_ce(_wctx(logits), logits.shape[0], Ccls, logits.shape[1], _p(logits), _p(labels), gscale,
                                                _p(loss), _p(grad)))
    return loss


def smooth_l1(pred, idx, target, beta, denom, grad=None, gscale=1.0, weights=None):
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    _ffi.check(_ffi.lib().cald_train_smooth_l1(_wctx(pred), idx.numel(), _p(pred), _p(idx), _p(target), beta, float(denom), _p(weights),
                                               gscale, _p(loss), _p(grad)))
    return loss


def focal_loss(logits_flat, level_pix, N, A, K, ld, matched, gt_labels, gt_off, img_weight, grad=None, gscale=1.0, alpha=0.25):
    loss = torch.empty(1, dtype=torch.float32, device=logits_flat.device)
    _ffi.check(_ffi.lib().cald_train_focal_loss(_wctx(logits_flat), N, _int_array(level_pix), A, K, ld, _p(logits_flat), _p(matched),
                                                _p(gt_labels), _p(gt_off), _p(img_weight), alpha, gscale, _p(loss), _p(grad)))
    return loss


def bce_logits(logits, idx, labels, grad=None, gscale=1.0):
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    _ffi.check(_ffi.lib().cald_train_bce_logits(_wctx(logits), idx.numel(), _p(logits), _p(idx), _p(labels), gscale, _p(loss), _p(grad)))
    return loss


def _seg_off(counts):
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


def softmax_ce_seg(logits, labels, Ccls, counts, grad=None, gscale=None):
    """softmax_ce per image: image i owns the next counts[i] rows.  gscale: None or a float32 device tensor [N].  Returns the losses [N]."""
    N = len(counts)
    loss = torch.empty(N, dtype=torch.float32, device=logits.device)
    _ffi.check(_ffi.lib().cald_train_softmax_ce_seg(_wctx(logits), N, _int_array(_seg_off(counts)), Ccls, logits.shape[1], _p(logits), _p(labels),
                                                    _p(gscale), _p(loss), _p(grad)))
    return loss


def smooth_l1_seg(pred, idx, target, beta, counts, denoms, grad=None, gscale=None, mean_out=None):
    """smooth_l1 per image: image i owns the next counts[i] gathered 4-vectors and divides its sum by denoms[i].  Returns the losses [N].
    mean_out (optional, 1 float32): receives seg_mean of the losses."""
    N = len(counts)
    loss = torch.empty(N, dtype=torch.float32, device=pred.device)
    den = (C.c_float * N)(*[float(d) for d in denoms])
    _ffi.check(_ffi.lib().cald_train_smooth_l1_seg(_wctx(pred), N, _int_array(_seg_off(counts)), _p(pred), _p(idx), _p(target), beta, den,
                                                   _p(gscale), _p(loss), _p(grad)))
    if mean_out is not None:
        seg_mean(loss, out=mean_out)
    return loss


def seg_mean(losses, out=None):
    """(((l_0 + l_1) + ...) + l_{N-1}) / N in float32, image order: ``_sum(losses) / len(targets)`` of retina_ll.py:132.  Returns [1]."""
    _chk(losses, "losses")
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=losses.device)
    _ffi.check(_ffi.lib().cald_train_seg_mean(_wctx(losses), losses.numel(), _p(losses), _p(out)))
    return out


def focal_loss_seg(logits_flat, level_pix, N, A, K, ld, matched, gt_labels, gt_off, denoms, grad=None, gscale=None, alpha=0.25, mean_out=None):
    """focal_loss per image: loss[n] = (sum of image n's terms) / denoms[n] (host floats > 0); image n's gradient is scaled by gscale[n]
    / denoms[n] (gscale: None or a float32 device tensor [N]).  mean_out (optional, 1 float32) receives seg_mean of the losses.
    Returns the losses [N]; nothing is launched or written when N exceeds the 64 images the call takes."""
    if len(denoms) != N or (gscale is not None and (gscale.numel() != N or gscale.dtype != torch.float32 or not gscale.is_contiguous())):
        raise ValueError("focal_loss_seg takes one denominator and one float32 gradient scale per image")
    loss = torch.empty(N, dtype=torch.float32, device=logits_flat.device)
    den = (C.c_float * N)(*[float(d) for d in denoms])
    _ffi.check(_ffi.lib().cald_train_focal_loss_seg(_wctx(logits_flat), N, _int_array(level_pix), A, K, ld, _p(logits_flat), _p(matched),
                                                    _p(gt_labels), _p(gt_off), den, alpha, _p(gscale), _p(loss), _p(mean_out), _p(grad)))
    return loss


def bce_logits_seg(logits, idx, labels, counts, grad=None, gscale=None):
    """bce_logits per image: image i owns the next counts[i] gathered logits.  Returns the losses [N]."""
    N = len(counts)
    loss = torch.empty(N, dtype=torch.float32, device=logits.device)
    _ffi.check(_ffi.lib().cald_train_bce_logits_seg(_wctx(logits), N, _int_array(_seg_off(counts)), _p(logits), _p(idx), _p(labels), _p(gscale),
                                                    _p(loss), _p(grad)))
    return loss


def add_bcast(a, b, g, out=None):
    """(a + b) + g[n][c] / (H W) on [N, H, W, C] maps; g: [N, C] float32 view whose rows may be strided (a level of pooled [N, 4, C])."""
    _chk(a, "a"); _chk(b, "b")
    N, H, W, Cc = a.shape
    assert g.dtype == torch.float32 and g.shape == (N, Cc) and g.stride(1) == 1 and b.shape == a.shape
    out = out if out is not None else torch.empty_like(a)
    _ffi.check(_ffi.lib().cald_train_add_bcast(_wctx(a), N, H * W, Cc, _p(out), _p(a), _p(b), _p(g), g.stride(0) if N > 1 else Cc))
    return out


def train_gap(maps, out=None):
    """Global average pooling of four dense NHWC maps [N, H_l, W_l, 256] in the learning-loss sweep's summation order -> [N, 4, 256]."""
    N = maps[0].shape[0]
    for m in maps:
        _chk(m, "map"); assert m.shape[0] == N and m.shape[3] == 256
    out = out if out is not None else torch.empty((N, 4, 256), dtype=torch.float32, device=maps[0].device)
    hw = [v for m in maps for v in (m.shape[1], m.shape[2])]
    _ffi.check(_ffi.lib().cald_train_gap(_wctx(maps[0]), N, _ptr_array(maps), _int_array(hw), _p(out)))
    return out


def _lossnet_tensors(ts):
    """ts: the ten tensors in LossNet.state_dict() order (FC1.weight, FC1.bias, ..., linear.weight, linear.bias)."""
    t = _ffi.LossNetTensors()
    for j in range(4):
        t.fc_w[j], t.fc_b[j] = ts[2 * j].data_ptr(), ts[2 * j + 1].data_ptr()
    t.lin_w, t.lin_b = ts[8].data_ptr(), ts[9].data_ptr()
    return t


def lossnet_fwd(params, pooled, D):
    """pooled [B, 4, 256] -> (pred [B], hidden [B, 4, D])."""
    _chk(pooled, "pooled")
    B = pooled.shape[0]
    hidden = torch.empty((B, 4, D), dtype=torch.float32, device=pooled.device)
    pred = torch.empty(B, dtype=torch.float32, device=pooled.device)
    t = _lossnet_tensors(params)
    _ffi.check(_ffi.lib().cald_lossnet_train_fwd(_wctx(pooled), B, D, C.byref(t), _p(pooled), _p(hidden), _p(pred)))
    return pred, hidden


def lossnet_bwd(params, grads, pooled, hidden, g_pred, accumulate=False, need_g_pooled=False):
    """Gradients of LossNet's ten tensors into `grads`; returns g_pooled [B, 4, 256] or None."""
    _chk(pooled, "pooled"); _chk(hidden, "hidden"); _chk(g_pred, "g_pred")
    B, D = pooled.shape[0], hidden.shape[2]
    gh = torch.empty((B, 4 * D), dtype=torch.float32, device=pooled.device)
    g_pooled = torch.empty_like(pooled) if need_g_pooled else None
    tp, tg = _lossnet_tensors(params), _lossnet_tensors(grads)
    _ffi.check(_ffi.lib().cald_lossnet_train_bwd(_wctx(pooled), B, D, C.byref(tp), _p(pooled), _p(hidden), _p(g_pred), _p(gh), C.byref(tg),
                                                 int(accumulate), _p(g_pooled)))
    return g_pooled


def loss_pred_loss(inp, target, margin, g_up=None, want_terms=False, want_grad=True, per_pair=False):
    """LossPredLoss value [1] (+ the pair terms [B/2]) and d loss / d input [B] scaled by the device scalar g_up (None: 1); per_pair: the
    gradient of the pair terms (reduction='none') under the upstream gradients g_up [B/2]."""
    _chk(inp, "input"); _chk(target, "target")
    B = inp.numel()
    loss = torch.empty(1, dtype=torch.float32, device=inp.device)
    terms = torch.empty(B // 2, dtype=torch.float32, device=inp.device) if want_terms else None
    grad = torch.empty(B, dtype=torch.float32, device=inp.device) if want_grad else None
    _ffi.check(_ffi.lib().cald_loss_pred_loss(_wctx(inp), B, _p(inp), _p(target), float(margin), int(per_pair), _p(g_up), _p(loss), _p(terms), _p(grad)))
    return loss, terms, grad


def preprocess(images_u8, sizes, Hp, Wp, remainders=None):
    """images_u8: list of uint8 [H, W, 3] cuda tensors; sizes: list of (Hr, Wr).  Returns [N, Hp, Wp, 4] float32."""
    N = len(images_u8)
    dev = images_u8[0].device
    out = torch.empty((N, Hp, Wp, 4), dtype=torch.float32, device=dev)
    hw = [v for im, (hr, wr) in zip(images_u8, sizes) for v in (im.shape[0], im.shape[1], hr, wr)]
    rem = None
    if remainders is not None and any(r is not None for r in remainders):
        rem = (C.c_void_p * N)(*[(r.data_ptr() if r is not None else None) for r in remainders])
    _ffi.check(_ffi.lib().cald_train_preprocess(get_ctx(dev.index), N, _ptr_array(images_u8), rem, _int_array(hw), Hp, Wp, _p(out)))
    return out


def maxpool(x):
    N, H, W, Cc = x.shape
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), dtype=torch.float32, device=x.device)
    _ffi.check(_ffi.lib().cald_train_maxpool(_wctx(x), N, H, W, Cc, _p(x), _p(out)))
    return out


def subsample2(x):
    N, H, W, Cc = x.shape
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), dtype=torch.float32, device=x.device)
    _ffi.check(_ffi.lib().cald_train_subsample2(_wctx(x), N, H, W, Cc, _p(x), _p(out)))
    return out


def transform_size(H, W, min_size, max_size):
    hr, wr, hp, wp = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _ffi.check(_ffi.lib().cald_op_transform_size(H, W, min_size, max_size, C.byref(hr), C.byref(wr), C.byref(hp), C.byref(wp)))
    return hr.value, wr.value, hp.value, wp.value
