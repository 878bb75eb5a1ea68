"""numpy restatement of the split-fp16 weight pack a forward_precision "f16x3" trainer makes on the device (cald_amd/csrc/train_pack.hip;
model.hip pack_w16 at an inference model's finalize): the scale policy, the K-major index formula and the hi / lo split.

    S        max |w| = f * 2^e, f in [0.5, 1)  ->  S = 14 - e, clamped to +-40; 0 for an all-zero or non-finite tensor
    unscale  2^-(S + 4)
    k        Cin_k % 16 == 0 and at most 32 taps: ((ci >> 4) * taps + tap) * 16 + (ci & 15); else tap * Cin_k + ci;
             a tap-major linear layer (fc6: torch weight [Cout][Cin * taps], rows [tap][Cin]): tap * Cin + ci
    w16      [Kpad / 16][2 (hi, lo)][CoutPad][16] fp16:  hi = fp16(w * 2^S),  lo = fp16(w * 2^S - hi)   (round to nearest even)
"""
import math

import numpy as np


def round_up(x, m):
    return (x + m - 1) // m * m


def cout_pad(cout):
    return round_up(cout, 128) if cout >= 128 else (round_up(cout, 64) if cout >= 64 else round_up(cout, 32))


def f16x3_scale(max_abs):
    """(S, unscale) from the largest |weight| of a layer."""
    max_abs = float(np.float32(max_abs))
    S = 0
    if max_abs > 0.0 and math.isfinite(max_abs):
        S = 14 - math.frexp(max_abs)[1]
    S = max(-40, min(40, S))
    return S, float(np.ldexp(np.float32(1.0), -(S + 4)))


def kmajor(w, cin_k=None, taps=None):
    """torch weight -> K-major [Kpad][CoutPad] float32 in the kernels' chain order.  w: [Cout, Cin, KH, KW], or [Cout, Cin] (1 x 1), or --
    with `taps` -- the tap-major linear form [Cout, Cin * taps].  cin_k: channel stride of the input (>= Cin, default Cin)."""
    w = np.asarray(w, np.float32)
    if taps is not None:                                     # mode 2: k = tap * Cin + ci of torch column ci * taps + tap
        cout, cin = w.shape[0], w.shape[1] // taps
        wk = np.zeros((round_up(taps * cin, 16), cout_pad(cout)), np.float32)
        wk[:taps * cin, :cout] = w.reshape(cout, cin, taps).transpose(2, 1, 0).reshape(taps * cin, cout)
        return wk
    if w.ndim == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    cin_k = cin if cin_k is None else cin_k
    t = kh * kw
    wk = np.zeros((round_up(t * cin_k, 16), cout_pad(cout)), np.float32)
    tap, ci = np.meshgrid(np.arange(t), np.arange(cin), indexing="ij")
    k = ((ci >> 4) * t + tap) * 16 + (ci & 15) if (cin_k % 16 == 0 and t <= 32) else tap * cin_k + ci
    wk[k.reshape(-1), :cout] = w.reshape(cout, cin, t).transpose(2, 1, 0).reshape(t * cin, cout)
    return wk


def hwc_rows(w, cin_k=None):
    """The same weight as the oracle takes it: rows in (kh, kw, cin) order, [KH * KW * Cin_k][Cout], no padding of K or Cout."""
    w = np.asarray(w, np.float32)
    if w.ndim == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    cin_k = cin if cin_k is None else cin_k
    out = np.zeros((kh * kw, cin_k, cout), np.float32)
    out[:, :cin, :] = w.reshape(cout, cin, kh * kw).transpose(2, 1, 0)
    return out.reshape(kh * kw * cin_k, cout)


def split(wk, S):
    """(hi, lo) fp16 arrays of wk * 2^S."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.ldexp(np.asarray(wk, np.float32), S).astype(np.float32)
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def pack_w16(wk, S):
    """K-major [Kpad][CoutPad] -> the device buffer's words: uint16 [Kpad / 16][2][CoutPad][16]."""
    kpad, npad = wk.shape
    hi, lo = split(wk, S)
    out = np.empty((kpad // 16, 2, npad, 16), np.uint16)
    out[:, 0] = hi.view(np.uint16).reshape(kpad // 16, 16, npad).transpose(0, 2, 1)
    out[:, 1] = lo.view(np.uint16).reshape(kpad // 16, 16, npad).transpose(0, 2, 1)
    return out


def weight_cases(shape, seed=0):
    """{name: weight of `shape`}: the value ranges that exercise the scale policy and the split."""
    rng = np.random.RandomState(seed)
    base = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    base.reshape(-1)[0] = 1.0                                # max |w| of `base` is exactly 1
    cases = {"pow2": base * np.float32(0.25),
             "pow2_minus_ulp": base * np.nextafter(np.float32(0.25), np.float32(0)),
             "zero": np.zeros(shape, np.float32),
             "tiny_1e-6": base * np.float32(1e-6),
             "clamp_hi": base * np.float32(2.0 ** -60),      # S would be 74
             "clamp_lo": base * np.float32(2.0 ** 70)}       # S would be -57: the packed halves overflow to inf
    small = np.float32(1e-7) * (np.float32(1.0) + np.float32(0.25) * base)        # 0.75e-7 .. 1.25e-7: not one value with one residual
    mix = np.where(rng.rand(*shape) < 0.5, np.float32(1.0), small).astype(np.float32) * np.sign(base + np.float32(1e-3))
    mix.reshape(-1)[0] = 1.0
    cases["mixed_1_and_1e-7"] = mix.astype(np.float32)       # the lo halves of the small weights are fp16 subnormals
    return cases
