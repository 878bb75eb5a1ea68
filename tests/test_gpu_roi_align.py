"""roi.hip's three inference RoIAlign kernels (roi_order_kernel, roi_align_kernel, roi_align_rows_kernel with the three instantiations of
roi_rows_walk) through cald_op_roi_align_views, on the constructed cases of tests/_roi_cases.py: no model, no forward.  Every comparison
is byte for byte, against the oracle -- which test_roi_align.py pins to the numpy restatement, to a float64 evaluation and to the census
of the row walk's branches on the same cases without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import _roi_cases as K
import _roi_restatement as R

pytestmark = pytest.mark.gpu
F32 = np.float32
ERR_INVALID = -1
CAP = K.ROI_CAP
FILL = 0xA5A5A5A5           # guard word of every output row before the launch
NAMES = ("a", "b")


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


def _views(hip, feats, rois, C_, out16=0, kernel=0, rows_back=None, want_order=False, **over):
    """cald_op_roi_align_views on views given as lists (feats[v] = the four level maps, rois[v] = [n][4]) -> (rc, out words
    [V][rows_back][49][C] pre-filled with FILL, order [V][1024] or None)"""
    ffi = hip["ffi"]
    V = len(feats)
    counts = np.array([len(r) for r in rois], np.int32)
    rows_back = rows_back or max(1, int(counts.max()))
    flat = [np.ascontiguousarray(f, F32) for fv in feats for f in fv]
    fp = (ffi.c_f * len(flat))(*[ffi.ptr(f) for f in flat])
    hw = np.array([f.shape[:2] for f in flat], np.int32)
    allr = np.ascontiguousarray(np.concatenate([np.asarray(r, F32).reshape(-1, 4) for r in rois] + [np.zeros((1, 4), F32)]))
    out = np.full((V, rows_back, 49, C_), FILL, np.uint32)
    order = np.full((V, 1024), -7, np.int32) if want_order else None
    a = dict(V=V, feats=fp, level_hw=ffi.ptr(hw, ffi.c_i), counts=ffi.ptr(counts, ffi.c_i), rois=ffi.ptr(allr), C=C_, out16=out16, kernel=kernel,
             rows_back=rows_back, out=out.ctypes.data_as(C.POINTER(C.c_uint32)), order=ffi.ptr(order, ffi.c_i))
    keep = []                                   # overrides: integer arrays as lists, pointers and scalars as they are
    for k, v in over.items():
        if k in ("level_hw", "counts") and v is not None:
            keep.append(np.array(v, np.int32))
            v = ffi.ptr(keep[-1], ffi.c_i)
        a[{"rows_arg": "rows_back", "feats_arg": "feats", "rois_arg": "rois"}.get(k, k)] = v
    rc = hip["L"].cald_op_roi_align_views(a.pop("ctx", hip["ctx"]), a["V"], a["feats"], a["level_hw"], a["counts"], a["rois"], a["C"], a["out16"], a["kernel"],
                                          a["rows_back"], a["out"], a["order"])
    return rc, out, order


def _same_words(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def _want(name):
    """the oracle's rows of a case at 260 channels; C = 256 / C = 8 are their first channels (a channel's value does not depend on C)"""
    from oracle import oracle as o
    c = K.case(name)
    w = o.roi_align(c["feats"], c["rois"])
    w.setflags(write=False)
    return w


def _run_case(hip, name, C_, **kw):
    c = K.case(name)
    rc, out, _ = _views(hip, [K.feats_at(c, C_)], [c["rois"]], C_, **kw)
    hip["ffi"].check(rc)
    return out[0]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("C_,kernel", [(256, 0), (256, 1), (8, 0), (260, 0)], ids=["rows256", "gather256", "gather8", "gather260"])
def test_kernels_equal_the_oracle_on_the_constructed_cases(hip, orc, name, C_, kernel):
    """the row walk (C = 256 as the forward runs it) and the gather kernel (forced at 256; 8 and 260 channels) on every reachable branch of
    the walk, every row pattern, the sample edges and the level boundaries"""
    _same_words(_run_case(hip, name, C_, kernel=kernel), np.ascontiguousarray(_want(name)[:, :, :C_]), (name, C_, kernel))


@pytest.mark.parametrize("name", NAMES)
def test_row_walk_equals_the_gather_kernel_in_process(hip, orc, name):
    for out16 in (0, 1):
        _same_words(_run_case(hip, name, 256, kernel=0, out16=out16), _run_case(hip, name, 256, kernel=1, out16=out16), (name, out16))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kernel", [0, 1])
def test_split_form_rows_equal_split_words_of_the_oracle(hip, orc, name, kernel):
    """h16_store4 from both kernels: 16 hi halves, then 16 lo halves per 16 channels; rows with 16 x in fp16's subnormal range included"""
    want = R.split_words(np.ascontiguousarray(_want(name)[:, :, :256]))
    got = _run_case(hip, name, 256, kernel=kernel, out16=1)
    _same_words(got, want, (name, kernel))
    _same_words(R.join(got), orc.f16x3_requantize(np.ascontiguousarray(_want(name)[:, :, :256])), (name, kernel, "joined"))


@pytest.mark.parametrize("out16", [0, 1])
def test_views_case(hip, orc, out16):
    """nine views of different map sizes, 0 to 1000 RoIs: view 8 shares XCD column 0 with view 0, view 1 is empty between two full ones,
    every RoI of view 6 ties on the order key.  Rows below a view's count equal the oracle run on that view alone, every word from the
    count on is the guard word that went up, order[v][:n] is roi_order's permutation."""
    vc = K.views_case()
    rc, out, order = _views(hip, vc["feats"], vc["rois"], 256, out16=out16, rows_back=CAP, want_order=True)
    hip["ffi"].check(rc)
    for v in range(vc["V"]):
        n = int(vc["counts"][v])
        assert (out[v, n:] == FILL).all(), (v, "rows beyond the count were written")
        if n:
            want = orc.roi_align(vc["feats"][v], vc["rois"][v])
            _same_words(out[v, :n], R.split_words(want) if out16 else want, (v, out16))
        assert order[v, :n].tolist() == R.roi_order(vc["rois"][v]).tolist(), v
        assert sorted(order[v, :n].tolist()) == list(range(n)), v
        assert (order[v] != -7).all()           # the kernel writes all 1024 entries of a view


def test_one_view_through_the_new_hook_equals_cald_op_roi_align(hip, orc):
    c = K.case("b")
    ffi = hip["ffi"]
    for C_ in (256, 8):
        feats = K.feats_at(c, C_)
        fp = (ffi.c_f * 4)(*[ffi.ptr(f) for f in feats])
        hw = np.array([f.shape[:2] for f in feats], np.int32)
        old = np.empty((len(c["rois"]), 49, C_), F32)
        ffi.check(hip["L"].cald_op_roi_align(hip["ctx"], fp, ffi.ptr(hw, ffi.c_i), C_, len(c["rois"]), ffi.ptr(np.ascontiguousarray(c["rois"])), ffi.ptr(old)))
        _same_words(_run_case(hip, "b", C_), old, C_)


def test_rejected_arguments_leave_out_untouched(hip, orc):
    c = K.case("a")
    feats, rois = [K.feats_at(c, 16)], [c["rois"][:5]]
    def bad(C_=16, **over):
        rc, out, order = _views(hip, feats, rois, C_, want_order=True, **over)
        assert rc == ERR_INVALID, over
        assert (out == FILL).all() and (order == -7).all(), over
    bad(V=0); bad(V=129); bad(C_=0); bad(C_=6); bad(C_=1028); bad(C_=8, out16=1); bad(out16=2); bad(kernel=2); bad(kernel=-1)
    bad(rows_arg=CAP + 1); bad(rows_arg=0); bad(rows_arg=-1)
    bad(counts=[-1]); bad(counts=[CAP + 1])
    bad(level_hw=[[0, 3], [2, 2], [1, 2], [1, 1]]); bad(level_hw=[[3, 3], [2, 2], [1, -2], [1, 1]])
    bad(feats_arg=None); bad(level_hw=None); bad(counts=None); bad(rois_arg=None); bad(ctx=None)
    ffi = hip["ffi"]
    nul = (ffi.c_f * 4)(*([ffi.ptr(f) for f in feats[0][:3]] + [None]))
    bad(feats_arg=nul)
    for v in (np.nan, np.inf, -np.inf):
        r = np.array(rois[0], F32); r[3, 2] = v
        bad(rois_arg=ffi.ptr(r))
    assert hip["L"].cald_op_roi_align_views(hip["ctx"], 1, None, None, None, None, 16, 0, 0, 1, None, None) == ERR_INVALID
    rc, out, _ = _views(hip, feats, rois, 16)                  # and the next valid call works
    ffi.check(rc)
    _same_words(out[0], np.ascontiguousarray(_want("a")[:5, :, :16]), "after the rejected calls")
