"""The packed row tiles' row -> (view, row inside the view) lookup (common.h seg_find_row, run on the CPU through cald_op_row_pack_lookup)
against its restatement in numpy -- the largest v with pix_off[v] <= row -- on random plans that include empty views (leading, trailing,
several in a row), and the admission rule conv_pack_rows at its 32-bit limit.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from cald_amd import _ffi
    return _ffi


def lookup(ffi, out_hw, rows, in_hw=None, Cin=16, out_ld=64):
    out_hw = np.ascontiguousarray(out_hw, np.int32)
    in_hw = out_hw if in_hw is None else np.ascontiguousarray(in_hw, np.int32)
    rows = np.ascontiguousarray(rows, np.int64)
    view = np.full(rows.size, -1, np.int32)
    local = np.full(rows.size, -1, np.int64)
    packed = C.c_int64(-1)
    ffi.check(ffi.lib().cald_op_row_pack_lookup(len(out_hw), ffi.ptr(in_hw, ffi.c_i), ffi.ptr(out_hw, ffi.c_i), Cin, out_ld, rows.size,
                                               ffi.ptr(rows, ffi.c_i64), ffi.ptr(view, ffi.c_i), ffi.ptr(local, ffi.c_i64), C.byref(packed)))
    return view, local, packed.value


def test_lookup_matches_numpy_on_random_plans_with_empty_views(lib):
    rs = np.random.RandomState(7)
    for trial in range(200):
        V = int(rs.randint(1, 129))
        hw = rs.randint(1, 40, (V, 2)).astype(np.int32)
        hw[rs.rand(V) < 0.3] = 0                       # empty views anywhere, runs of them included
        if trial % 3 == 0:
            hw[0] = 0                                  # a leading empty view
        if trial % 5 == 0:
            hw[-1] = 0                                 # a trailing one
        if not hw.prod(1).any():
            hw[int(rs.randint(V))] = (3, 5)
        pix_off = np.concatenate([[0], np.cumsum(hw.prod(1, dtype=np.int64))])
        total = int(pix_off[-1])
        rows = np.unique(np.concatenate([np.arange(0, total, 128), pix_off[:-1][pix_off[:-1] < total], np.maximum(pix_off[1:] - 1, 0),
                                         rs.randint(0, total, 64), [total - 1]])).astype(np.int64)
        view, local, packed = lookup(lib, hw, rows)
        want = np.searchsorted(pix_off[:V], rows, side="right") - 1         # the largest v with pix_off[v] <= row
        np.testing.assert_array_equal(view, want)
        np.testing.assert_array_equal(local, rows - pix_off[want])
        assert np.all(hw[view].prod(1) > local), "a row was given to a view that does not hold it (an empty view, or past its end)"
        assert packed == total


def test_admission_rule_refuses_what_a_32_bit_offset_cannot_reach(lib):
    """A tile that straddles two views addresses both from the first one's start: input span, and output rows to the tile's end."""
    rows = np.array([0], np.int64)
    ok = [(1000, 1000), (100, 100)]                                   # 1 000 000 rows: the boundary falls inside a tile
    assert lookup(lib, ok, rows, Cin=64)[2] == 1010000
    assert lookup(lib, ok, rows, Cin=512)[2] == 1010000               # 1 010 000 x 512 x 4 B = 2.07e9 < 0x7FFE0000 - 64 KB
    assert lookup(lib, ok, rows, Cin=1024)[2] == 0                    # the input span of the straddling tile passes 2 GB
    assert lookup(lib, ok, rows, Cin=16, out_ld=1024)[2] == 0         # so does the first view's output plus one tile
    aligned = [(1024, 1000), (100, 100)]                              # the boundary on a tile edge: no tile straddles, nothing to refuse
    assert lookup(lib, aligned, rows, Cin=512, out_ld=256)[2] == 1034000
    assert lookup(lib, [(0, 0), (0, 0)], np.zeros(0, np.int64))[2] == 0   # an empty level has nothing to pack
