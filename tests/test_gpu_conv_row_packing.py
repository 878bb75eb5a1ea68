"""Packed row tiles of conv_p4.hip (ConvArgs::packed_rows): a launch tiles the output level's flat row space, so a 128-row tile may
cover the end of one view and the start of the next ones.  Every case runs through cald_op_conv_probe twice on the same operands, with
per-view tiles and with packed tiles: the two output buffers must be the same bytes -- guard rows and channels Cout .. out_ld included
-- and both equal oracle.conv2d per view (test_gpu_conv_variants.check).  Inputs are random and mostly non-zero, so a tap that reads a
neighbouring view's pixel instead of the zero outside the image shows.

Shapes (output H x W per view; stride-2 cases feed the odd input size 2 o - 1):
  issue3   5x7, 0x0, 9x13, 11x12      284 rows: both tile boundaries fall inside a view, an empty view lies inside tile 0
  many     5x7, 0x0, 6x9, 4x5, 11x12  tile 0 touches four views and the empty one
  edge     8x16, 3x5                  the first view ends exactly on the tile boundary
  small    5x7, 3x4                   47 rows in all: one tile, partly filled
  eight    8 views of 2x3             48 rows, eight views in one tile
The generic k-loop (TAPS 0) runs a 5 x 5 filter on 16 channels: conv_p4 takes no Cin that is not a multiple of 16 (Cin 20 goes to
conv_mfma, which is not packed)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_conv_variants import FP32, NARROW, P4, P4_GROUP, WIDE, Prob, check, hip      # noqa: F401  (hip: the module fixture)

pytestmark = pytest.mark.gpu

PACK_OFF, PACK_ON = 1, 2

VIEWS = {
    "issue3": [(5, 7), (0, 0), (9, 13), (11, 12)],
    "many": [(5, 7), (0, 0), (6, 9), (4, 5), (11, 12)],
    "edge": [(8, 16), (3, 5)],
    "small": [(5, 7), (3, 4)],
    "eight": [(2, 3)] * 8,
}


def in_views(out_views, stride):
    return [(0, 0) if h == 0 else (stride * (h - 1) + 1, stride * (w - 1) + 1) for h, w in out_views]


def run(hip, kws, path, tile, pack):
    """One launch of fresh problems built from kws (same seeds: same operands every time) under the given row tiling."""
    ffi = hip["ffi"]
    probs = [Prob(seed=11 + i, **kw) for i, kw in enumerate(kws)]
    structs = [p.struct(ffi) for p in probs]
    for s in structs:
        s.row_packing = pack
    arr = (ffi.ConvProbe * len(probs))(*structs)
    name = C.create_string_buffer(256)
    ffi.check(hip["L"].cald_op_conv_probe(hip["ctx"], FP32, arr, len(probs), path, tile, name, 256))
    return probs, name.value.decode()


def both_ways(hip, kws, path, tile, kernel=None):
    per_view, k0 = run(hip, kws, path, tile, PACK_OFF)
    packed, k1 = run(hip, kws, path, tile, PACK_ON)
    assert k0 == k1 and (kernel is None or k1 == kernel), (k0, k1, kernel)
    for i, (a, b) in enumerate(zip(per_view, packed)):
        for name in ("got", "got16", "gote"):
            x, y = getattr(a, name), getattr(b, name)
            assert (x is None) == (y is None)
            if x is not None:
                assert x.tobytes() == y.tobytes(), "problem %d: %s differs between per-view and packed tiles (%d words)" % (i, name, int((x != y).sum()))
    check(per_view, FP32)
    check(packed, FP32)


# filter / epilogue variants: (id, kwargs, taps, epi)
VARIANTS = [
    ("3x3", dict(K=3, relu=True), 9, 0),
    ("3x3_s2_inrelu", dict(K=3, stride=2, in_relu=True, relu=False), 9, 0),
    ("3x3_cin48", dict(K=3, Cin=48, bias=False), 9, 0),              # three 16-channel chunks: the loader's channel cursor moves
    ("1x1", dict(K=1, relu=True), 1, 0),
    ("1x1_s2", dict(K=1, stride=2, bn=False), 1, 0),
    ("5x5_generic", dict(K=5, relu=False), 0, 0),
    ("3x3_res", dict(K=3, res=True), 9, 1),
    ("1x1_res_s2", dict(K=1, stride=2, res=True, in_relu=True), 1, 1),
    ("1x1_up", dict(K=1, up=True, bn=False, relu=False), 1, 2),       # the FPN lateral: per-view up_hw (Prob.uhw)
    ("3x3_up", dict(K=3, up=True, in_relu=True), 9, 2),
    ("5x5_up", dict(K=5, up=True), 0, 2),
]


@pytest.mark.parametrize("tn,tile", [(1, NARROW), (2, WIDE)], ids=["narrow", "wide"])
@pytest.mark.parametrize("var", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("views", sorted(VIEWS))
def test_packed_equals_per_view_and_oracle(hip, views, var, tn, tile):
    _, kw, taps, epi = var
    Cout = 56 if tn == 1 else 120              # channels Cout .. out_ld are guard words; CoutPad 64 / 128
    kw = dict(kw, views=in_views(VIEWS[views], kw.get("stride", 1)), Cout=Cout, out_ld=Cout + 8)
    kw.setdefault("Cin", 16)
    both_ways(hip, [kw], P4, tile, "conv_p4_kernel<%d,false,%d,%d>" % (epi, tn, taps))


@pytest.mark.parametrize("views", sorted(VIEWS))
def test_packed_out16_and_energy4(hip, views):
    """The FPN output conv under the pruning: 256 channels, split-fp16 copy and per-pixel energy out of the packed launch's epilogue."""
    kw = dict(views=VIEWS[views], Cin=32, Cout=256, K=3, relu=False, bn=False, energy=True, out16=True)
    both_ways(hip, [kw], P4, WIDE, "conv_p4_kernel<0,false,2,9>")


@pytest.mark.parametrize("tn,tile", [(1, NARROW), (2, WIDE)], ids=["narrow", "wide"])
@pytest.mark.parametrize("K", [3, 1])
def test_packed_group_of_four_levels(hip, K, tn, tile):
    """Four problems of different levels in one grouped launch, one of them with fewer than 128 rows in all."""
    Cout = 64 if tn == 1 else 128
    levels = [[(19, 25), (0, 0), (17, 29)], VIEWS["issue3"], VIEWS["small"], VIEWS["eight"]]
    kws = [dict(views=v, Cin=32, Cout=Cout, K=K, out_ld=Cout + 4) for v in levels]
    both_ways(hip, kws, P4_GROUP, tile, "conv_p4_group_kernel<0,false,%d,%d>" % (tn, 9 if K == 3 else 1))


def test_unpackable_problem_is_refused(hip):
    """row_packing = 2 on a launch whose row counts live on the device is an error, not a silent per-view launch."""
    with pytest.raises(Exception):
        run(hip, [dict(views=VIEWS["small"], dyn=[10, 3])], P4, NARROW, PACK_ON)
