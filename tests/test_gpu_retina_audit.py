"""GPU tests of the RetinaNet decision-margin audit (audit.hip audit_retina_kernel / audit_retina_suborder_kernel, through
cald_op_retina_audit and cald_sweep_audit).

  * The hook equals tests/_retina_audit_restatement.py bit for bit on the constructed cases (tests/test_retina_audit.py shows what each was
    built for): both sides compute float32 expressions in a stated order from the same float32 scores and boxes -- the restatement's come
    from the oracle's exponential, the library's bits.
  * On a small RetinaNet the audit changes no score, fills the slots a RetinaNet has, and sees a near-tie in every image whose f16x3
    consistency differs from the exact one; the Faster R-CNN margins are what they were before the RetinaNet audit existed.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _retina_audit_restatement as A

F32 = np.float32
pytestmark = pytest.mark.gpu
SIZES = dict(min_size=300, max_size=500)
AUGS = ["flip", "cut_out", "smaller_resize"]


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


def gpu_audit(hip, case):
    ffi, L = hip["ffi"], hip["L"]
    cls, reg = case.heads()
    hw = np.array([v for hw_ in case.level_hw for v in hw_], np.int32)
    base = np.ascontiguousarray(case.base, F32)
    cp = (ffi.c_f * 5)(*[ffi.ptr(c) for c in cls]); rp = (ffi.c_f * 5)(*[ffi.ptr(r) for r in reg])
    Hp, Wp, Hr, Wr = case.sizes
    m = np.full(ffi.N_MARGINS, np.nan, F32); n = C.c_int(-1)
    ffi.check(L.cald_op_retina_audit(hip["ctx"], cp, rp, ffi.ptr(hw, ffi.c_i), case.A, case.K, ffi.ptr(base), Hp, Wp, Hr, Wr, 2 * Hr, 2 * Wr,
                                     case.score_thr, case.nms_thr, case.per_class, C.byref(n), ffi.ptr(m)))
    return m, n.value


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_hook_equals_the_restatement_bit_for_bit(hip, oracle, name):
    case = A.CASES[name]()
    want = case.restate(oracle.exp_array)
    got, n = gpu_audit(hip, case)
    print(name, "n", n, "margins", {hip["ffi"].MARGIN_NAMES[q]: float(got[q]) for q in range(16) if np.isfinite(got[q])})
    assert n == want["n"], (name, n, want["n"])
    assert got.tobytes() == want["margins"].tobytes(), (name, got, want["margins"])
    if name == "many":                                   # the regime the case is for: the class's candidates do not fit the tail's LDS sort
        s, _ = case.inputs(oracle.exp_array)
        assert (s[:, 0] > F32(0.05)).sum() > 8192 and np.isfinite(got[[A.THR, A.IOU, A.ORDER, A.CAP, A.SMALL, A.TOP2, A.SUB]]).all()


def test_hook_refuses_more_than_512_per_class(hip):
    case = A.CASES["nothing"]()
    case.per_class = 513
    with pytest.raises(NotImplementedError, match="AUDIT_MAX_DET"):
        gpu_audit(hip, case)


# ---------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def retina_runs(hip):
    """64 images of pool seed 0 (the noise row was calibrated on seed 1) through a small RetinaNet: per precision the plain sweep and the audited
    one at two batch sizes."""
    torch = hip["torch"]
    from cald_amd import synth, sweep
    sd = synth.pseudo_trained_retinanet(21, 50, seed=0)
    dev = [torch.from_numpy(im).cuda() for im in synth.make_pool(64, "voc", 0, scale=0.5)]
    pos = list(range(len(dev)))
    out = {}
    for prec in ("fp32", "f16x3"):
        m = hip["det"].retinanet_resnet50_fpn_cal(num_classes=21, precision=prec, **SIZES).to("cuda")
        m.load_state_dict(sd); m.eval()
        plain = sweep.sweep_device_images(m, dev, pos, AUGS, bp=1.3, base_seed=0, batch_images=16)
        audited = [sweep.sweep_device_images(m, dev, pos, AUGS, bp=1.3, base_seed=0, batch_images=b, margins=True) for b in (16, 24)]
        out[prec] = dict(plain=plain, audited=audited)
        del m
        torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_the_audit_changes_no_score(retina_runs, prec):
    """(i) margins=True returns the plain sweep's consistency and cls_corr bit for bit, at two batch sizes; the margins do not depend on
    the batch size either."""
    r = retina_runs[prec]
    plain = r["plain"]
    for audited in r["audited"]:
        assert plain[0].tobytes() == audited[0].tobytes() and plain[1].tobytes() == audited[1].tobytes()
    assert r["audited"][0][2].tobytes() == r["audited"][1][2].tobytes()
    assert (plain[0] > 0).sum() >= 32


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_margins_fill_the_slots_a_retinanet_has(hip, retina_runs, prec):
    """(ii) RPN and RoI slots +inf, no NaN, nothing negative; the NMS and small-box margins finite on every image with a detection."""
    cons, _, mg = retina_runs[prec]["audited"][0]
    assert mg.shape == (64, hip["ffi"].N_MARGINS) and mg.dtype == F32
    assert np.isinf(mg[:, :7]).all() and not np.isnan(mg).any() and (mg >= 0).all()
    has = cons > 0
    assert has.sum() >= 32 and np.isfinite(mg[has][:, [8, 15]]).all()
    # the argmax record compares a reference box's best detection with the best one of ANOTHER box (an anchor's detections share one): a
    # gap between two IoUs, well below the best IoU itself on views that hold hundreds of overlapping detections
    assert np.isfinite(mg[has][:, 12]).all() and np.median(mg[has][:, 12]) < 0.1


def test_every_image_f16x3_scores_differently_carries_a_near_tie(hip, retina_runs):
    """(iii) every image whose f16x3 consistency differs from the exact one by more than 1e-5 has a margin below 4 x the measured f16x3
    noise (MARGIN_NOISE_F16X3_RETINA, profiles/retina_f16x3_noise.json)."""
    ce = retina_runs["fp32"]["audited"][0][0]
    ch, _, mh = retina_runs["f16x3"]["audited"][0]
    noise = np.array(hip["ffi"].MARGIN_NOISE_F16X3_RETINA, F32)
    assert noise.shape == (16,) and (noise[:7] == 0).all() and (noise[7:] > 0).all()
    changed = np.abs(ce - ch) > 1e-5
    near = (mh < 4.0 * noise[None, :]).any(axis=1)
    print("retina audit: %d of %d images changed beyond 1e-5; %d have a decision within 4 x noise" % (int(changed.sum()), len(ce), int(near.sum())))
    for i in np.where(changed & ~near)[0]:
        print("  image %d: |delta| %.3g, margins / noise %s" % (i, abs(ce[i] - ch[i]), np.round(mh[i, 7:] / noise[7:], 1).tolist()))
    assert near[changed].all(), np.where(changed & ~near)[0]


def test_frcnn_margins_are_what_they_were(hip, golden):
    """(iv) the Faster R-CNN margins of a fixed 16-image sweep equal the fixture written before the RetinaNet audit
    (tools/make_golden_frcnn_audit.py); the new slot 15 stays +inf."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_frcnn_audit", os.path.join(os.path.dirname(__file__), "..", "tools", "make_golden_frcnn_audit.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    want = golden("frcnn_audit_margins")
    c, mg = tool.sweep_margins()
    assert c.tobytes() == want["consistency"].tobytes()
    assert mg[:, :15].tobytes() == want["margins"].tobytes()
    assert np.isinf(mg[:, 15]).all() and np.isfinite(want["margins"][:, [0, 1, 8]]).all()


def test_more_than_512_per_class_is_not_implemented(hip):
    """(v)"""
    torch = hip["torch"]
    from cald_amd import synth, sweep
    m = hip["det"].retinanet_resnet50_fpn_cal(num_classes=21, detections_per_img=513, **SIZES).to("cuda")
    m.load_state_dict(synth.pseudo_trained_retinanet(21, 50, seed=0)); m.eval()
    dev = [torch.from_numpy(im).cuda() for im in synth.make_pool(2, "voc", 0, scale=0.5)]
    with pytest.raises(NotImplementedError, match="AUDIT_MAX_DET"):
        sweep.sweep_device_images(m, dev, [0, 1], AUGS, margins=True)
    c, k = sweep.sweep_device_images(m, dev, [0, 1], AUGS)              # the plain sweep takes the model
    assert c.shape == (2,)


def test_an_image_without_detections_still_gets_its_threshold_margin(hip):
    """A threshold 5e-4 above an image's best score: no detection, consistency 0.0 as in the plain sweep -- and the margins say how close
    that was: post_thr is the distance of that best score, the kinds that need a candidate stay +inf."""
    torch = hip["torch"]
    from cald_amd import synth, sweep
    sd = synth.pseudo_trained_retinanet(21, 50, seed=0)
    dev = [torch.from_numpy(im).cuda() for im in synth.make_pool(2, "voc", 0, scale=0.5)][1:]
    m = hip["det"].retinanet_resnet50_fpn_cal(num_classes=21, **SIZES).to("cuda")
    m.load_state_dict(sd); m.eval()
    best = F32(m(dev)[0]["scores"].max().item())
    thr = F32(best + F32(5e-4))
    strict = hip["det"].retinanet_resnet50_fpn_cal(num_classes=21, score_thresh=float(thr), **SIZES).to("cuda")
    strict.load_state_dict(sd); strict.eval()
    assert F32(strict.cfg.box_score_thresh) == thr and len(strict(dev)[0]["scores"]) == 0
    c, k, mg = sweep.sweep_device_images(strict, dev, [0], AUGS, margins=True)
    assert c[0] == 0.0 and (k == 0).all()
    assert mg[0, A.THR] == F32(thr - best) and np.isinf(mg[0, [A.IOU, A.ORDER, A.CAP, A.SMALL, A.SUB, A.TOP2, 12]]).all()
