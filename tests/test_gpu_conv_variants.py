"""Every conv kernel instantiation the launchers can launch, pinned one at a time through cald_op_conv_probe and compared with a plain
reference at the shapes and feature combinations where kernels go wrong (M / K / Cout tails, ragged views, empty views, dynamic and
gathered rows, border taps).

  exact mode:  bit for bit against oracle.conv2d, per view (in_relu applied to the input first, mask after everything else; dyn_rows,
               row_map and gather select rows of the full output -- every output is an independent k-chain, so those bits are exact too)
  f16x3 mode:  bit for bit against oracle.conv2d_f16x3 (split-form residuals through oracle.f16x3_requantize); split-form outputs
               (out16) word for word against the split of the reference value (h16.h), which is what f16x3_requantize decodes
  energy4:     each of the four 64-channel partial sums of squares within the relative error the pruning's bound pays for (the 1.0001 of
               rpn_prune.hip: 2304 u, u = 2^-24, for a sum of 9 x 256 squares) of the float64 sum over the reference output
Every output buffer is the caller's, filled with a sentinel and returned whole: words outside what the launch may write (guard rows
after the last one, channels Cout .. out_ld, rows a view's dyn_rows / row_map / gather count excludes) must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FP32, F16X3 = 0, 1
AUTO, P4, P4_GROUP, P4_FUSED, GENERIC, STEM, H3, H3_GROUP, H4, H4_GROUP = range(10)
TAUTO, NARROW, WIDE = 0, 1, 2
SENT = np.uint32(0xFFC0DEAD)          # a NaN no kernel produces from finite operands
GUARD = 128                           # guard rows after the last output row (one whole M tile)


def _p4(epi, c4, tn, taps):
    return "conv_p4_kernel<%d,%s,%d,%d>" % (epi, "true" if c4 else "false", tn, taps)


def _mf(cfg, epi, fast):
    return "conv_mfma_f32_kernel<%s,%d,16,%s>" % (cfg, epi, "true" if fast else "false")


# Every instantiation the launchers of conv_p4.hip, conv_mfma.hip, conv_stem.hip, conv_h3.hip and conv_h4.hip can launch.
ALL_KERNELS = set(
    # launch_conv_p4: plain / residual / top-down, masked (training backward) with and without residual -- both tiles, taps 0 / 1 / 9
    [_p4(e, False, tn, t) for e in (0, 1, 2, 4, 5) for tn in (1, 2) for t in (0, 1, 9)]
    # gathered rows (16) with residual (17): 1 x 1 and 3 x 3 only
    + [_p4(e, False, tn, t) for e in (16, 17) for tn in (1, 2) for t in (1, 9)]
    # Cin == 4: the unrolled 7 x 7 stem (13 k-tiles) and the generic loop
    + [_p4(0, True, tn, t) for tn in (1, 2) for t in (0, 13)]
    # launch_conv_p4_group: plain or masked
    + ["conv_p4_group_kernel<%d,false,%d,%d>" % (e, tn, t) for e in (0, 4) for tn in (1, 2) for t in (0, 1, 9)]
    + ["conv_p4_fused_kernel"]
    # launch_conv_generic: three tile configurations x plain / residual / top-down x fast / general k-loop
    + [_mf(cfg, e, f) for cfg in ("2,2,2,2", "2,2,2,1", "4,1,1,1") for e in (0, 1, 2) for f in (True, False)]
    + ["conv_stem_kernel"]
    + ["conv_h3_kernel<0,%d,true>" % tn for tn in (1, 2)]
    + ["conv_h3_kernel<%d,%d,false>" % (e, tn) for e in (0, 1, 2) for tn in (1, 2)]
    + ["conv_h3_group_kernel<0,%d,false>" % tn for tn in (1, 2)]
    + ["conv_h4_kernel<%d>" % e for e in (0, 1, 2)]
    + ["conv_h4_group_kernel"])

OBSERVED = set()


@pytest.fixture(scope="module")
def hip():
    import torch
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0))


# ------------------------------------------------------------------------------------------------------------------- problem set-up
def split_words(x, C):
    """h16.h split form of x [pixels][C] (C % 16 == 0): per 16-channel chunk [16 fp16 hi | 16 fp16 lo] of 16 x, as uint32 [pixels][C]."""
    s = (np.asarray(x, np.float32) * np.float32(16)).astype(np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    P = s.shape[0]
    h = np.empty((P, C // 16, 2, 16), np.float16)
    h[:, :, 0, :] = hi.reshape(P, C // 16, 16)
    h[:, :, 1, :] = lo.reshape(P, C // 16, 16)
    return np.ascontiguousarray(h).view(np.uint32).reshape(P, C)


def out_hw(H, W, K, s, p):
    if H == 0 or W == 0:
        return 0, 0
    return (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1


class Prob:
    """One conv problem of the probe: data, the reference, the expected buffers."""

    def __init__(self, seed, views=((9, 11),), Cin=16, Cout=64, K=3, stride=1, pad=None, bias=True, bn=True, relu=True, in_relu=False,
                 out_ld=None, res=False, up=False, mask=False, dyn=None, row_map=False, gather=None, energy=False, out16=False,
                 in16=False, ex16=False, out32=True, cin_true=None):
        rs = np.random.RandomState(seed)
        self.__dict__.update(views=list(views), Cin=Cin, Cout=Cout, K=K, stride=stride, pad=K // 2 if pad is None else pad, relu=relu,
                             in_relu=in_relu, out_ld=out_ld or Cout, dyn=dyn, gather=gather, ex16=ex16, energy=energy, out16=out16,
                             out32=out32)
        self.V = len(self.views)
        self.ohw = [out_hw(H, W, K, stride, self.pad) for H, W in self.views]
        self.pin = np.cumsum([0] + [H * W for H, W in self.views])
        self.pout = np.cumsum([0] + [h * w for h, w in self.ohw])
        R, L = int(self.pout[-1]), self.out_ld
        self.x = rs.randn(int(self.pin[-1]), Cin).astype(np.float32)
        self.x[rs.rand(*self.x.shape) < 0.3] = 0.0
        self.cin_true = cin_true or Cin              # the stem: 3 channels of weights, the input's fourth channel is zero padding
        self.x[:, self.cin_true:] = 0.0
        self.w = (rs.randn(Cout, self.cin_true, K, K) * np.sqrt(2.0 / (Cin * K * K))).astype(np.float32)
        wf = np.zeros((Cout, Cin, K, K), np.float32)
        wf[:, :self.cin_true] = self.w
        self.wk = np.ascontiguousarray(wf.transpose(2, 3, 1, 0).reshape(-1, Cout))
        self.b = rs.randn(Cout).astype(np.float32) if bias else None
        self.sc = (0.5 + rs.rand(Cout)).astype(np.float32) if bn else None
        self.sh = rs.randn(Cout).astype(np.float32) if bn else None
        self.r = rs.randn(R, L).astype(np.float32) if res else None
        self.uhw = [((h + 1) // 2, (w + 1) // 2) for h, w in self.ohw]
        self.pup = np.cumsum([0] + [h * w for h, w in self.uhw])
        self.u = rs.randn(int(self.pup[-1]), L).astype(np.float32) if up else None
        self.m = rs.randn(R, L).astype(np.float32) if mask else None
        self.x16 = split_words(self.x, Cin) if in16 else None
        self.rmap = None
        if row_map:        # a random subset of each view's pixels, in random order, dyn[v] of them
            self.rmap = np.zeros(max(R, 1), np.int32)
            for v in range(self.V):
                n = self.ohw[v][0] * self.ohw[v][1]
                self.rmap[self.pout[v]:self.pout[v] + n] = rs.permutation(n).astype(np.int32)

    # reference output of view v, [Ho][Wo][Cout]
    def ref_view(self, v, precision):
        from oracle import oracle as orc
        H, W = self.views[v]
        Ho, Wo = self.ohw[v]
        x = self.x[self.pin[v]:self.pin[v + 1]].reshape(H, W, self.Cin)
        res = up = None
        if self.r is not None:
            res = self.r[self.pout[v]:self.pout[v + 1], :self.Cout].reshape(Ho, Wo, self.Cout)
        if self.u is not None:
            up = self.u[self.pup[v]:self.pup[v + 1], :self.Cout].reshape(self.uhw[v][0], self.uhw[v][1], self.Cout)
        if self.ex16:
            res = orc.f16x3_requantize(res) if res is not None else None
            up = orc.f16x3_requantize(up) if up is not None else None
        bn = (self.sc, self.sh) if self.sc is not None else None
        if precision == F16X3:
            y = orc.conv2d_f16x3(x, self.wk, self.K, self.K, self.stride, self.pad, bias=self.b, bn=bn, residual=res, up=up, relu=self.relu,
                                 in_relu=self.in_relu)
        else:
            xr = np.maximum(x, np.float32(0)) if self.in_relu else x
            y = orc.conv2d(xr, self.wk, self.K, self.K, self.stride, self.pad, bias=self.b, bn=bn, residual=res, up=up, relu=self.relu)
        if self.m is not None:
            y = np.where(self.m[self.pout[v]:self.pout[v + 1], :self.Cout].reshape(Ho, Wo, self.Cout) > 0, y, np.float32(0))
        return y.reshape(Ho * Wo, self.Cout)

    # the rows a launch writes: (buffer row, reference pixel) pairs of view v
    def rows(self, v):
        n = self.ohw[v][0] * self.ohw[v][1]
        if self.gather is not None:
            Wo = self.ohw[v][1]
            pix = [(y0 + j) * Wo + x0 + i for (x0, y0, w, h) in self.gather[v] for j in range(h) for i in range(w)]
            return np.array(pix, np.int64), np.array(pix, np.int64)
        d = n if self.dyn is None else min(self.dyn[v], n)
        m = np.arange(d)
        return m, (self.rmap[self.pout[v]:self.pout[v] + d].astype(np.int64) if self.rmap is not None else m)

    def expected(self, precision):
        R, L, C = int(self.pout[-1]), self.out_ld, self.Cout
        out = np.full((R + GUARD, L), SENT, np.uint32)
        o16 = np.full((R + GUARD, L), SENT, np.uint32)
        e64 = np.full((R + GUARD, 4), np.nan)
        written = np.zeros(R + GUARD, bool)
        for v in range(self.V):
            if self.ohw[v][0] * self.ohw[v][1] == 0:
                continue
            y = self.ref_view(v, precision)
            m, pix = self.rows(v)
            if m.size == 0:
                continue
            rows = self.pout[v] + m
            vals = y[pix]
            out[rows, :C] = vals.view(np.uint32)
            if self.out16:
                w = split_words(np.pad(vals, ((0, 0), (0, L - C))), L)
                o16[rows, :C] = w[:, :C]
            v64 = vals.astype(np.float64) ** 2
            for q in range(4):
                if 64 * q < C:
                    e64[rows, q] = v64[:, 64 * q:64 * q + 64].sum(1)
            written[rows] = True
        return out, o16, e64, written

    def struct(self, ffi):
        from cald_amd._ffi import ConvProbe
        p = ConvProbe()
        p.V = self.V
        for v, (H, W) in enumerate(self.views):
            p.in_hw[v][0], p.in_hw[v][1] = H, W
            p.up_hw[v][0], p.up_hw[v][1] = self.uhw[v]
            if self.dyn is not None:
                p.dyn_rows[v] = self.dyn[v]
            if self.gather is not None:
                p.nrect[v] = len(self.gather[v])
                for k, rc in enumerate(self.gather[v]):
                    for j in range(4):
                        p.rect[v][k][j] = rc[j]
        p.has_dyn = int(self.dyn is not None)
        p.gather = int(self.gather is not None)
        p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad = self.Cin, self.Cout, self.K, self.K, self.stride, self.pad
        p.relu, p.in_relu, p.out_ld, p.cin_true = int(self.relu), int(self.in_relu), self.out_ld, self.cin_true
        u32 = C.POINTER(C.c_uint32)
        p.weight, p.bias, p.bn_scale, p.bn_shift = ffi.ptr(self.w), ffi.ptr(self.b), ffi.ptr(self.sc), ffi.ptr(self.sh)
        p.in_ = ffi.ptr(self.x)
        p.in16 = ffi.ptr(self.x16, u32)
        self._rw = split_words(self.r, self.out_ld).view(np.float32) if (self.ex16 and self.r is not None) else self.r
        self._uw = split_words(self.u, self.out_ld).view(np.float32) if (self.ex16 and self.u is not None) else self.u
        p.residual, p.up, p.ex16 = ffi.ptr(self._rw), ffi.ptr(self._uw), int(self.ex16)
        p.mask = ffi.ptr(self.m)
        p.row_map = ffi.ptr(self.rmap, C.POINTER(C.c_int))
        R = int(self.pout[-1]) + GUARD
        self.got = np.full((R, self.out_ld), SENT, np.uint32) if self.out32 else None
        self.got16 = np.full((R, self.out_ld), SENT, np.uint32) if self.out16 else None
        self.gote = np.full((R, 4), SENT, np.uint32) if self.energy else None
        p.out, p.out_n = ffi.ptr(self.got.view(np.float32) if self.got is not None else None), 0 if self.got is None else self.got.size
        p.out16, p.out16_n = ffi.ptr(self.got16, u32), 0 if self.got16 is None else self.got16.size
        p.energy4, p.energy4_n = ffi.ptr(self.gote.view(np.float32) if self.gote is not None else None), 0 if self.gote is None else self.gote.size
        return p


def probe(hip, probs, path=AUTO, tile=TAUTO, precision=FP32):
    """Runs the launch; returns the kernel name(s).  Refusal raises NotImplementedError (CALD_ERR_UNSUPPORTED)."""
    ffi = hip["ffi"]
    arr = (ffi.ConvProbe * len(probs))(*[p.struct(ffi) for p in probs])
    name = C.create_string_buffer(256)
    ffi.check(hip["L"].cald_op_conv_probe(hip["ctx"], precision, arr, len(probs), path, tile, name, 256))
    return name.value.decode()


def check(probs, precision):
    for i, p in enumerate(probs):
        out, o16, e64, written = p.expected(precision)
        if p.got is not None:
            bad = np.nonzero(p.got != out)
            assert bad[0].size == 0, "problem %d: %d words differ, first (row, channel) %r: got %08x want %08x" % (
                i, bad[0].size, (int(bad[0][0]), int(bad[1][0])), int(p.got[bad][0]), int(out[bad][0]))
        if p.got16 is not None:
            bad = np.nonzero(p.got16 != o16)
            assert bad[0].size == 0, "problem %d: %d split words differ, first (row, channel) %r" % (i, bad[0].size, (int(bad[0][0]), int(bad[1][0])))
        if p.gote is not None:
            g = p.gote.view(np.float32).astype(np.float64)
            assert np.all(p.gote[~written] == SENT), "problem %d: energy4 written outside the launch's rows" % i
            E = e64[written]
            got = g[written]
            # the four slots cover channels [64 q, 64 q + 64): together all 256; each within 2304 u of the float64 sum (rpn_prune.hip 1.0001)
            assert np.all(np.isfinite(got)), "problem %d: energy4 slots not written (%d rows)" % (i, int((~np.isfinite(got)).any(1).sum()))
            assert np.all(np.abs(got - E) <= 2304 * 2.0 ** -24 * E), "problem %d: energy4 max rel err %g" % (
                i, float((np.abs(got - E) / np.maximum(E, 1e-30)).max()))


# ----------------------------------------------------------------------------------------------------------------- the matrix
def _cases():
    """(id, [Prob kwargs ...], path, tile, precision, expected kernel name or None)."""
    cs = []
    tails = [(16, 8), (1, 129), (127, 1)]           # rows per view = 0, 1, 127 (mod 128), a 1-pixel-wide view
    ragged = [(9, 11), (3, 5), (16, 8), (1, 1), (12, 13)]
    shapes = {9: dict(K=3), 1: dict(K=1), 0: dict(K=5)}
    for tn, tile in ((1, NARROW), (2, WIDE)):
        for taps, kw in shapes.items():
            Cout = (80 if tn == 2 else 64)
            cs.append(("p4_plain_tn%d_t%d" % (tn, taps), [dict(views=tails, Cout=Cout, **kw)], P4, tile, FP32, _p4(0, False, tn, taps)))
            cs.append(("p4_res_tn%d_t%d" % (tn, taps), [dict(views=ragged, Cout=Cout, res=True, out_ld=Cout + 16, **kw)], P4, tile, FP32, _p4(1, False, tn, taps)))
            cs.append(("p4_up_tn%d_t%d" % (tn, taps), [dict(views=ragged[:3], Cout=Cout, up=True, in_relu=True, **kw)], P4, tile, FP32, _p4(2, False, tn, taps)))
            cs.append(("p4_mask_tn%d_t%d" % (tn, taps), [dict(views=ragged[:2], Cout=Cout, mask=True, dyn=[50, 0], **kw)], P4, tile, FP32, _p4(4, False, tn, taps)))
            cs.append(("p4_maskres_tn%d_t%d" % (tn, taps), [dict(views=tails[:2], Cout=Cout, mask=True, res=True, **kw)], P4, tile, FP32, _p4(5, False, tn, taps)))
            cs.append(("p4_group_tn%d_t%d" % (tn, taps), [dict(views=ragged, Cout=Cout, **kw), dict(views=[(0, 0)], Cout=Cout, **kw),
                                                          dict(views=tails, Cout=Cout, dyn=[100, 0, 127], **kw)], P4_GROUP, tile, FP32,
                       "conv_p4_group_kernel<0,false,%d,%d>" % (tn, taps)))
            cs.append(("p4_groupmask_tn%d_t%d" % (tn, taps), [dict(views=ragged[:2], Cout=Cout, mask=True, **kw),
                                                              dict(views=[(5, 7)], Cout=Cout, mask=True, **kw)], P4_GROUP, tile, FP32,
                       "conv_p4_group_kernel<4,false,%d,%d>" % (tn, taps)))
        # gathered rows: 1 .. 8 rectangles touching the borders, stride 1 and 2, with and without residual
        for taps, K in ((9, 3), (1, 1)):
            for res, st in ((False, 1), (True, 2)):
                H, W = (13, 17) if st == 1 else (25, 33)          # output 13 x 17 either way
                g = [[(0, 0, 3, 2)], [], [(0, 0, 17, 1), (0, 12, 17, 1), (0, 1, 1, 11), (16, 1, 1, 11), (5, 5, 2, 2), (8, 3, 4, 1), (2, 8, 3, 3),
                                          (12, 9, 3, 2)]]
                cs.append(("p4_gather_tn%d_t%d_s%d_res%d" % (tn, taps, st, res),
                           [dict(views=[(H, W)] * 3, Cout=256 if tn == 2 else 64, K=K, stride=st, res=res, gather=g)], P4, tile, FP32,
                           _p4(17 if res else 16, False, tn, taps)))
        # Cin == 4: the 7 x 7 / 2 stem (Kpad 208 > K 196) on the unrolled and a 3 x 3 on the generic loop
        c4out = 64 if tn == 1 else 128
        cs.append(("p4_c4_stem_tn%d" % tn, [dict(views=[(37, 53), (8, 9)], Cin=4, cin_true=3, Cout=c4out, K=7, stride=2, bias=False)], P4, tile, FP32,
                   _p4(0, True, tn, 13)))
        cs.append(("p4_c4_3x3_tn%d" % tn, [dict(views=[(9, 11), (1, 1)], Cin=4, Cout=c4out, K=3, bias=False)], P4, tile, FP32, _p4(0, True, tn, 0)))
    # energy4 + out16 of the FPN output conv under the pruning: wide single launch, grouped launch, auto (which must pick wide)
    e = dict(Cin=32, Cout=256, K=3, relu=False, bn=False, energy=True, out16=True)
    cs.append(("p4_energy_wide", [dict(views=ragged, **e)], P4, WIDE, FP32, _p4(0, False, 2, 9)))
    cs.append(("p4_energy_auto", [dict(views=[(9, 11)], **e)], AUTO, TAUTO, FP32, _p4(0, False, 2, 9)))
    cs.append(("p4_energy_group", [dict(views=ragged[:3], **e), dict(views=[(5, 7)], dyn=[20], **e)], P4_GROUP, TAUTO, FP32,
               "conv_p4_group_kernel<0,false,2,9>"))
    cs.append(("p4_out16_narrow", [dict(views=tails, Cin=32, Cout=256, K=3, out16=True)], P4, NARROW, FP32, _p4(0, False, 1, 9)))
    cs.append(("p4_rowmap", [dict(views=ragged[:3], Cin=32, Cout=256, K=3, dyn=[40, 0, 128], row_map=True, energy=True, out16=True)],
               P4, TAUTO, FP32, _p4(0, False, 2, 9)))
    # the fused layer-1 pair: conv2 (3 x 3, 64 -> 64) + conv3 (1 x 1, 64 -> 256, + residual)
    cs.append(("p4_fused", [dict(views=ragged, Cin=64, Cout=64, K=3, bias=False),
                            dict(views=ragged, Cin=64, Cout=256, K=1, bias=False, res=True)], P4_FUSED, TAUTO, FP32, "conv_p4_fused_kernel"))
    # generic kernel: Cout tails 105 / 64 / 15 (tiles 128 / 64 / 32), fast and general k-loops (Cin 20: Kpad > K; 7 x 7 Cin 16: 49 taps)
    for cfg, Cout in (("2,2,2,2", 105), ("2,2,2,1", 64), ("4,1,1,1", 15)):
        for fast, kw in ((True, dict(Cin=16, K=3)), (False, dict(Cin=20, K=3)), (False, dict(Cin=16, K=7, views=[(8, 9)]))):
            v = kw.pop("views", tails)
            tag = "fast" if fast else "slow_k%d" % kw["K"]
            cs.append(("generic_%s_%s_plain" % (cfg, tag), [dict(views=v, Cout=Cout, in_relu=True, **kw)], GENERIC, TAUTO, FP32, _mf(cfg, 0, fast)))
            cs.append(("generic_%s_%s_res" % (cfg, tag), [dict(views=ragged[:3] if v is tails else v, Cout=Cout, res=True, dyn=[30, 0, 5][:len(v)] if v is tails else None,
                                                                out_ld=Cout + 3, **kw)], GENERIC, TAUTO, FP32, _mf(cfg, 1, fast)))
            cs.append(("generic_%s_%s_up" % (cfg, tag), [dict(views=v, Cout=Cout, up=True, stride=2, **kw)], GENERIC, TAUTO, FP32, _mf(cfg, 2, fast)))
    # K chain of 12 544 (fc6)
    cs.append(("p4_fc6_chain", [dict(views=[(1, 130)], Cin=12544, Cout=128, K=1)], P4, WIDE, FP32, _p4(0, False, 2, 1)))
    # the stem kernel: every view an exact grid of 8 x 16 output blocks
    cs.append(("stem", [dict(views=[(32, 64), (16, 32)], Cin=4, cin_true=3, Cout=64, K=7, stride=2, pad=3, bias=False)], STEM, TAUTO, FP32, "conv_stem_kernel"))
    # f16x3: conv_h3 (fp32 or split input, split residual), its group, conv_h4 (split input only), its group
    for tn, Cout in ((1, 64), (2, 256)):
        cs.append(("h3_c4_tn%d" % tn, [dict(views=[(9, 11), (16, 8)], Cin=4, Cout=Cout, K=7, stride=2, bias=False)], H3, TAUTO, F16X3, "conv_h3_kernel<0,%d,true>" % tn))
        cs.append(("h3_plain_tn%d" % tn, [dict(views=tails, Cout=Cout, in_relu=True, out16=True)], H3, TAUTO, F16X3, "conv_h3_kernel<0,%d,false>" % tn))
        cs.append(("h3_res_tn%d" % tn, [dict(views=ragged, Cout=Cout, res=True, ex16=True, in16=True, K=1, dyn=[99, 3, 128, 0, 7])], H3, TAUTO, F16X3,
                   "conv_h3_kernel<1,%d,false>" % tn))
        cs.append(("h3_up_tn%d" % tn, [dict(views=ragged[:3], Cout=Cout, up=True, stride=2, out_ld=Cout + 16)], H3, TAUTO, F16X3, "conv_h3_kernel<2,%d,false>" % tn))
        cs.append(("h3_group_tn%d" % tn, [dict(views=ragged, Cout=Cout), dict(views=[(0, 0)], Cout=Cout), dict(views=tails, Cout=Cout, in16=True, out16=True)],
                   H3_GROUP, TAUTO, F16X3, "conv_h3_group_kernel<0,%d,false>" % tn))
    cs.append(("h4_plain", [dict(views=tails, Cin=32, Cout=256, in16=True, out16=True, out32=False)], H4, TAUTO, F16X3, "conv_h4_kernel<0>"))
    cs.append(("h4_res", [dict(views=ragged, Cin=16, Cout=256, K=1, in16=True, res=True, ex16=True, dyn=[99, 3, 128, 0, 7])], H4, TAUTO, F16X3, "conv_h4_kernel<1>"))
    cs.append(("h4_up", [dict(views=ragged[:3], Cin=16, Cout=256, in16=True, up=True)], H4, TAUTO, F16X3, "conv_h4_kernel<2>"))
    cs.append(("h4_group", [dict(views=ragged, Cin=16, Cout=256, in16=True), dict(views=[(0, 0)], Cin=16, Cout=256, in16=True),
                            dict(views=tails, Cin=16, Cout=512, in16=True, out16=True)], H4_GROUP, TAUTO, F16X3, "conv_h4_group_kernel"))
    return cs


CASES = _cases()


def _run_case(hip, case):
    cid, specs, path, tile, precision, want = case
    probs = [Prob(1000 * k + sum(map(ord, cid)), **s) for k, s in enumerate(specs)]
    if path == P4_FUSED:       # conv3 reads conv2's output, which the fused kernel keeps on chip: conv2's buffer stays untouched
        probs[1].x = np.concatenate([probs[0].ref_view(v, FP32) for v in range(probs[0].V)]).astype(np.float32)
    name = probe(hip, probs, path, tile, precision)
    OBSERVED.update(name.split(";"))
    if path == P4_FUSED:
        assert np.all(probs[0].got == SENT), "the fused kernel wrote conv2's output"
    check(probs[1:] if path == P4_FUSED else probs, precision)
    assert name == want, "%s launched %s, expected %s" % (cid, name, want)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_variant_matches_reference(hip, case):
    _run_case(hip, case)


def test_every_instantiation_is_exercised(hip):
    """The kernels the matrix launched are exactly the instantiations the launchers can launch (cases deselected in this run are
    run here)."""
    for case in CASES:
        if case[5] not in OBSERVED:
            _run_case(hip, case)
    assert OBSERVED == ALL_KERNELS, ("never launched: %s; not in the list: %s" % (sorted(ALL_KERNELS - OBSERVED), sorted(OBSERVED - ALL_KERNELS)))


# --------------------------------------------------------------------------------------------------------------------- refusals
def _refusals():
    g = [[(0, 0, 3, 2)]]
    rs = []
    for path, prec, base in ((H3, F16X3, dict(Cout=64)), (H4, F16X3, dict(Cout=256, in16=True)), (GENERIC, FP32, dict(Cout=64))):
        feats = [("mask", dict(mask=True))]
        if path != GENERIC:
            feats += [("gather", dict(gather=g)), ("row_map", dict(dyn=[20], row_map=True)), ("energy4", dict(Cout=256, energy=True))]
        else:
            feats += [("gather", dict(gather=g)), ("row_map", dict(dyn=[20], row_map=True)), ("energy4", dict(Cout=256, energy=True)),
                      ("out16", dict(out16=True))]
        for fname, f in feats:
            kw = dict(base); kw.update(f)
            rs.append(("%d_%s" % (path, fname), [kw], path, TAUTO, prec))
    rs.append(("p4_narrow_energy4", [dict(Cin=32, Cout=256, energy=True, relu=False)], P4, NARROW, FP32))
    rs.append(("p4_group_narrow_energy4", [dict(Cin=32, Cout=256, energy=True, relu=False)], P4_GROUP, NARROW, FP32))
    rs.append(("p4_energy4_res", [dict(Cin=32, Cout=256, energy=True, res=True)], P4, WIDE, FP32))
    rs.append(("p4_mask_up", [dict(mask=True, up=True)], P4, TAUTO, FP32))
    rs.append(("p4_c4_mask", [dict(Cin=4, K=3, mask=True)], P4, TAUTO, FP32))
    rs.append(("p4_res_and_up", [dict(res=True, up=True)], P4, TAUTO, FP32))
    rs.append(("generic_res_and_up", [dict(res=True, up=True)], GENERIC, TAUTO, FP32))
    rs.append(("auto_mask_no_kernel", [dict(Cin=20, mask=True)], AUTO, TAUTO, FP32))       # conv_p4 refuses Cin 20; the generic kernel has no mask
    rs.append(("p4_wide_cout64", [dict(Cout=64)], P4, WIDE, FP32))
    rs.append(("stem_not_exact_grid", [dict(views=[(30, 64)], Cin=4, cin_true=3, Cout=64, K=7, stride=2, pad=3, bias=False)], STEM, TAUTO, FP32))
    rs.append(("h3_in_fp32_mode", [dict()], H3, TAUTO, FP32))
    rs.append(("h4_without_split_input", [dict(Cout=256)], H4, TAUTO, F16X3))
    rs.append(("fused_wrong_shape", [dict(Cin=64, Cout=64, K=3, bias=False), dict(Cin=64, Cout=256, K=1, bias=False)], P4_FUSED, TAUTO, FP32))
    return rs


def test_pinned_launchers_refuse_what_they_do_not_implement(hip):
    """A pinned launcher refuses (CALD_ERR_UNSUPPORTED) every feature it does not implement -- it never launches with one ignored and never
    hands the problem to another kernel; the output buffer stays untouched."""
    accepted = []
    for rid, specs, path, tile, prec in _refusals():
        probs = [Prob(7, **s) for s in specs]
        try:
            name = probe(hip, probs, path, tile, prec)
            accepted.append("%s -> %s" % (rid, name))
        except NotImplementedError:
            for p in probs:
                assert p.got is None or np.all(p.got == SENT), rid
    assert not accepted, "launched instead of refused: %s" % accepted


# ---------------------------------------------------------------------------------------------------------------- auto selection
def test_auto_selection_boundaries(hip):
    """What the product's selection picks, so that a change of a heuristic is a visible decision: the narrow tile up to 384 M tiles of a
    128-channel 1 x 1 layer (2 x 384 narrow workgroups fill one round of 768 slots), the wide one from 385 on; energy4 always wide; the stem
    kernel only where every view is an exact grid of 8 x 16 output blocks."""
    def name(views, **kw):
        kw.setdefault("Cin", 16); kw.setdefault("K", 1)
        return probe(hip, [Prob(3, views=views, **kw)], AUTO, TAUTO, FP32)
    assert name([(384 * 128, 1)], Cout=128) == _p4(0, False, 1, 1)
    assert name([(385 * 128, 1)], Cout=128) == _p4(0, False, 2, 1)
    assert name([(128, 1)], Cout=128, dyn=[128]) == _p4(0, False, 2, 1)               # dynamic rows: wide
    assert name([(128, 1)], Cout=256, energy=True, relu=False) == _p4(0, False, 2, 1)  # energy4: wide (narrow would leave it unwritten)
    assert name([(128, 1)], Cout=256, relu=False) == _p4(0, False, 1, 1)
    stem = dict(Cin=4, cin_true=3, Cout=64, K=7, stride=2, pad=3, bias=False)
    assert name([(32, 64), (16, 32)], **stem) == "conv_stem_kernel"
    assert name([(30, 64)], **stem) == _p4(0, True, 1, 13)                              # 15 output rows: not a grid of 8 x 16
    assert name([(9, 11)], Cin=20, Cout=64, K=3) == _mf("2,2,2,1", 0, False)             # Cin % 16 != 0: the generic kernel
    assert name([(9, 11)], Cout=15, K=3) == _mf("4,1,1,1", 0, True)                      # Cout 15: the 32-wide generic tile
