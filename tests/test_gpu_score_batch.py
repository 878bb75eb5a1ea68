"""score.hip's five kernels on whole batches in the sweep's layout, through cald_op_score_batch: the constructed cases of
tests/_score_cases.py against the numpy restatement (tests/_score_restatement.py), which test_score_batch.py pins to the oracle on the
same cases without a GPU.  No model, no forward.  Every output is compared byte for byte (a NaN equals any NaN); 0xA5 guard bytes
around every output array must survive."""
import ctypes as C
import functools

import numpy as np
import pytest

import _score_cases as K
import _score_restatement as R

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 256
ERR_INVALID = -1


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    assert _ffi.lib().cald_op_pair_params(9, 1, 1, 0.0, None) == ERR_INVALID
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


@functools.lru_cache(maxsize=None)
def _case(Cn):
    return K.batch_case(Cn)


class Guarded:
    """a float32 output array between two runs of 0xA5 bytes, itself pre-filled with 0xA5"""

    def __init__(self, shape):
        n = int(np.prod(shape)) * 4
        self.raw = np.full(n + 2 * GUARD, 0xA5, np.uint8)
        self.a = self.raw[GUARD:GUARD + n].view(F32).reshape(shape)

    def intact(self):
        return (self.raw[:GUARD] == 0xA5).all() and (self.raw[-GUARD:] == 0xA5).all()

    def untouched(self):
        return (self.raw == 0xA5).all()


def _probe(hip, case, **over):
    ffi = hip["ffi"]
    V, P, Cn = case["V"], case["P"], case["C"]
    out = dict(cons=Guarded((max(P, 1),)), cls_corr=Guarded((V, Cn - 1)), pair_audit=Guarded((max(P, 1), 2)), max_iou=Guarded((max(P, 1), 50)), lt=Guarded((V,)))
    arrs = {k: np.ascontiguousarray(case[k]) for k in ("boxes", "props", "scores", "labels", "scores_cls", "prob_max", "count", "view_img", "view_isref",
                                                       "ref_sel", "ref_n", "ref_view", "aug_view", "pair_img", "aug_kind", "aug_param")}
    for k, v in over.items():
        if k in arrs:
            arrs[k] = None if v is None else np.ascontiguousarray(v, arrs[k].dtype)
    q = ffi.ScoreProbe()
    q.V, q.cap, q.C, q.n_img, q.P, q.bp = V, case["cap"], over.get("C", Cn), case["n_img"], P, case["bp"]
    for k, a in arrs.items():
        setattr(q, k, ffi.ptr(a, dict(ffi.ScoreProbe._fields_)[k]))
    for k, g in out.items():
        setattr(q, k, None if over.get(k, 0) is None else ffi.ptr(g.a))
    rc = hip["L"].cald_op_score_batch(hip["ctx"], C.byref(q))
    return rc, out


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero((np.where(nan, 0, got).view(np.uint32) != np.where(nan, 0, want).view(np.uint32)).ravel())
    assert not len(bad), (what, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


@pytest.mark.parametrize("Cn", [21, 91])
def test_score_batch_equals_restatement(hip, oracle, Cn):
    """consistency, class-max vectors, the pair audit, max-IoU rows and lt_c of one batch: three images (50, 3 and 0 scored boxes), thirteen
    views of 0 / 1 / 63 / 64 / 65 / 100 / 2049 detections, every box transform with the parameters cald_op_pair_params gives"""
    case = _case(Cn)
    ffi, L = hip["ffi"], hip["L"]
    par = np.zeros((case["P"], 12), F32)
    for p, (img, _, kind, prm) in enumerate(case["pairs"]):
        ffi.check(L.cald_op_pair_params(kind, K.IMG_HW[img][0], K.IMG_HW[img][1], prm, ffi.ptr(par[p])))
    _same(par, case["aug_param"], "pair parameters")
    rc, out = _probe(hip, case, aug_param=par)
    ffi.check(rc)
    fill = np.full((case["P"], 50), 0xA5A5A5A5, np.uint32).view(F32)
    want = R.score_batch(case, oracle.js_divergence, max_iou_fill=fill)
    for k, g in out.items():
        assert g.intact(), k
        _same(g.a, want[k], k)
    for p in range(case["P"]):                  # the oracle directly, where it has the function
        img, av = int(case["pair_img"][p]), int(case["aug_view"][p])
        sel, M = R.selection(case, img), int(case["count"][av])
        if len(sel) and M:
            ab = R.aug_box(case["boxes"][img][sel], int(case["aug_kind"][p]), par[p])
            cons = oracle.consistency_view(ab, case["scores_cls"][img][sel], case["prob_max"][img][sel], case["boxes"][av][:M],
                                           case["scores_cls"][av][:M], case["prob_max"][av][:M], case["bp"])
            _same(out["cons"].a[p], F32(cons), ("oracle consistency", p))
    assert (out["cons"].a[case["count"][case["aug_view"]] == 0] == 0).all()


@pytest.mark.parametrize("turn", K.LT_TURNS)
def test_lt_uncertainty_kernel_edges(hip, oracle, turn):
    """views of 0, 1, 255, 256, 257 and 600 detections; the minimum at detection 0, 255, 256 or the last one"""
    case = K.lt_case(turn)
    rc, out = _probe(hip, case)
    hip["ffi"].check(rc)
    assert all(g.intact() for g in out.values())
    got = out["lt"].a
    _same(got, R.score_batch(case, None)["lt"], "lt")
    assert got[0] == 1.0
    for v, n in enumerate(K.LT_COUNTS):
        _same(got[v], F32(oracle.lt_uncertainty(dict(boxes=case["boxes"][v][:n], props=case["props"][v][:n], prob_max=case["prob_max"][v][:n]))), v)
    assert out["cons"].untouched() and out["pair_audit"].untouched() and out["max_iou"].untouched()      # no pair: nothing written


def test_score_batch_rejects_bad_arguments(hip, oracle):
    case = K.lt_case(0)
    case = dict(case, P=1)
    def bad(**over):
        rc, out = _probe(hip, case, **over)
        assert rc == ERR_INVALID, over
        assert all(g.untouched() for g in out.values()), over
    bad(C=1); bad(C=257)
    bad(ref_n=[51]); bad(ref_n=[-1])
    bad(ref_n=[2], ref_sel=np.r_[0, case["cap"], np.zeros(48, int)][None])
    bad(view_img=[0, 0, 1, 0, 0, 0]); bad(view_img=[0, -1, 0, 0, 0, 0])
    bad(ref_view=[6]); bad(aug_view=[-1]); bad(pair_img=[1]); bad(aug_kind=[4])
    bad(count=[0, 1, 255, 256, 257, 601])
    for k in ("boxes", "props", "scores", "labels", "scores_cls", "prob_max", "count", "view_img", "view_isref", "ref_sel", "ref_n", "ref_view",
              "aug_view", "pair_img", "aug_kind", "aug_param", "cons", "cls_corr", "pair_audit", "max_iou", "lt"):
        bad(**{k: None})
    assert hip["L"].cald_op_score_batch(hip["ctx"], None) == ERR_INVALID and hip["L"].cald_op_score_batch(None, None) == ERR_INVALID
    rc, out = _probe(hip, case)                 # and the next valid call works
    hip["ffi"].check(rc)
    _same(out["lt"].a, R.score_batch(case, None)["lt"], "lt after the rejected calls")


def test_sweep_ltc_refuses_retinanet(hip):
    """lt_c reads the proposals behind the detections; RetinaNet has none"""
    from cald_amd import synth
    torch, ffi = hip["torch"], hip["ffi"]
    model = hip["det"].retinanet_resnet50_fpn_cal(num_classes=21, min_size=64, max_size=96)
    model.to("cuda").load_state_dict(synth.pseudo_trained_retinanet(21, 50, seed=0))
    model.eval()
    img = torch.zeros((40, 56, 3), dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * 1)(img.data_ptr())
    out = np.full(1, -7.0, np.float64)
    rc = hip["L"].cald_sweep_ltc(model.handle(), 1, ptrs, ffi.ptr(np.array([40], np.int32), ffi.c_i), ffi.ptr(np.array([56], np.int32), ffi.c_i), 1,
                                 ffi.ptr(out, ffi.c_d))
    assert rc == ERR_INVALID and b"Faster R-CNN" in hip["L"].cald_last_error() and out[0] == -7.0
