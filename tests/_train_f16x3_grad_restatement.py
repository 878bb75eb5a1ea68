"""numpy restatement of a data gradient of a backward_precision "f16x3" trainer (cald_amd/csrc/train_pack.hip, train_conv.hip,
conv_h3.hip), on top of tests/_train_f16x3_restatement.py and the oracle's bit-for-bit statement of conv_h3:

    filter   the data gradient of a conv with torch weight w [Cout, Cin, KH, KW] (+ FrozenBatchNorm scale) is the stride-1 convolution of
             dY (channel stride CinK >= Cout) with  wd [Cin, CinK, KH, KW],  wd[ci, co, kh, kw] = fp32(w[co, ci, KH-1-kh, KW-1-kw] * scale[co]);
             of a tap-major linear layer [Cout, Cin * taps] the 1 x 1 filter  wd [taps * Cin, CinK],  wd[t * Cin + ci, co] = w[co, ci * taps + t] * scale[co]
    S_d      finalize's scale policy (R.f16x3_scale) on max |wd|;  the twin is R.pack_w16(R.kmajor(wd), S_d)
    G        max |g| = f * 2^e, f in [0.5, 1)  ->  G = 7 - e, clamped to +-60; 0 for an all-zero or non-finite tensor;  in_scale = 2^(4 + G)
    launch   oracle.conv2d_f16x3 on g * 2^G (the oracle stages at 2^4) with the prepared weights' unscale replaced by 2^-(S_d + 4 + G), the
             fp32 residual passed through, then  out = mask > 0 ? out : 0
"""
import math

import numpy as np

import _train_f16x3_restatement as R


def grad_scale(max_abs):
    """(G, in_scale) from the largest |entry| of a gradient tensor."""
    max_abs = float(np.float32(max_abs))
    G = 0
    if max_abs > 0.0 and math.isfinite(max_abs):
        G = 7 - math.frexp(max_abs)[1]
    G = max(-60, min(60, G))
    return G, float(np.ldexp(np.float32(1.0), 4 + G))


def grad_filter(w, scale=None, cin_k=None, taps=None):
    """The data gradient's filter as a forward torch weight: [Cin, CinK, KH, KW] (conv; a 2-D w is a 1 x 1 conv) or, with `taps`, the 1 x 1
    filter [taps * Cin, CinK] of a tap-major linear layer.  Rows co >= Cout (channel padding of dY) are zero."""
    w = np.asarray(w, np.float32)
    cout = w.shape[0]
    cin_k = R.round_up(cout, 4) if cin_k is None else cin_k
    sc = np.ones(cout, np.float32) if scale is None else np.asarray(scale, np.float32)
    if taps is not None:
        cin = w.shape[1] // taps
        ws = (w * sc[:, None]).astype(np.float32).reshape(cout, cin, taps)
        wd = np.zeros((taps * cin, cin_k), np.float32)
        wd[:, :cout] = ws.transpose(2, 1, 0).reshape(taps * cin, cout)
        return wd
    if w.ndim == 2:
        w = w[:, :, None, None]
    _, cin, kh, kw = w.shape
    ws = (w * sc[:, None, None, None]).astype(np.float32)
    wd = np.zeros((cin, cin_k, kh, kw), np.float32)
    wd[:, :cout] = ws[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)
    return wd


def grad_twin(wd):
    """(S_d, uint16 words [Kpad / 16][2][NPad][16]) of the device twin of the data-gradient pack of filter wd."""
    S = R.f16x3_scale(np.abs(wd).max() if wd.size else 0.0)[0]
    return S, R.pack_w16(R.kmajor(wd), S)


def dilate(g, stride, hd, wd_):
    """dY [H, W, C] of a strided layer scattered onto the stride-1 grid [hd, wd_, C]."""
    out = np.zeros((hd, wd_, g.shape[2]), np.float32)
    out[::stride, ::stride][:g.shape[0], :g.shape[1]] = g
    return out


def dgrad(oracle, g, wd, pad, G, residual=None, mask=None, prepared=None):
    """One image's data gradient, bit for bit what conv_h3 computes: g [H, W, CinK] (already dilated for a strided layer), wd from
    grad_filter, pad = K - 1 - forward pad.  prepared: oracle.f16x3_weights of wd, to share among launches."""
    g = np.ascontiguousarray(g, np.float32)
    kh, kw = (wd.shape[2], wd.shape[3]) if wd.ndim == 4 else (1, 1)
    wp = prepared if prepared is not None else prepare(oracle, wd)
    wp = dict(wp, unscale=float(np.ldexp(np.float32(1.0), -(wp["S"] + 4 + G))))
    with np.errstate(over="ignore", invalid="ignore"):
        out = oracle.conv2d_f16x3(np.ldexp(g, G).astype(np.float32), wp, kh, kw, 1, pad, residual=residual)
    if mask is not None:
        out = np.where(np.asarray(mask, np.float32) > 0, out, np.float32(0.0)).astype(np.float32)
    return out


def prepare(oracle, wd):
    kh, kw = (wd.shape[2], wd.shape[3]) if wd.ndim == 4 else (1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        wp = oracle.f16x3_weights(R.hwc_rows(wd), kh, kw, wd.shape[1])
    assert wp["S"] == R.f16x3_scale(np.abs(wd).max())[0]
    return wp
