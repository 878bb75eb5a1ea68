"""Packed row tiles in the detector forward (cald_model_set_row_packing): a ragged batch of three image sizes, small enough that P5 / P6
hold a few dozen rows per view -- one 128-row tile then spans all three views, and most tiles of the coarse levels straddle a view end.
Every stage tensor cald_debug_tensor exposes is the same bytes with the switch off and on, and equal to the oracle's (as
test_gpu_parity.test_forward_stagewise_bit_exact compares them); a sweep's consistency / cls_corr are the same bytes either way."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIN_SIZE, MAX_SIZE = 160, 256
STAGES = ["input", "conv1", "pool1", "C2", "C3", "C4", "C5", "P2", "P3", "P4", "P5", "P6", "rpn0", "rpn1", "rpn2", "rpn3", "rpn4",
          "proposals", "roi", "fc6", "fc7", "pred"]


@pytest.fixture(scope="module")
def hip():
    import torch
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, det=detector, torch=torch)


@pytest.fixture(scope="module")
def tiny_model(hip, oracle):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    model = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=MIN_SIZE, max_size=MAX_SIZE).to("cuda")
    model.load_state_dict(sd)
    model.eval()
    return model, oracle.prepare_frcnn(sd, 21, 50)


def set_packing(hip, model, mode):
    was = C.c_int()
    hip["ffi"].check(hip["L"].cald_model_set_row_packing(model.handle(), mode, C.byref(was)))
    return was.value


def three_sizes():
    """Three pool images with three different padded sizes."""
    from cald_amd import synth
    pool = synth.make_pool(12, "voc", 0, scale=0.5)
    picked, seen = [], set()
    for im in pool:
        if im.shape[:2] not in seen:
            seen.add(im.shape[:2]); picked.append(im)
        if len(picked) == 3:
            break
    assert len(picked) == 3, "the synthetic pool should hold three image sizes"
    return picked


def test_forward_stages_identical_packed_and_per_view_and_oracle(hip, oracle, tiny_model):
    torch = hip["torch"]
    model, P = tiny_model
    imgs = three_sizes()
    views = [(torch.from_numpy(im).cuda(), v == 1, None) for v, im in enumerate(imgs)]
    got = {}
    was = set_packing(hip, model, 0)
    try:
        for mode in (0, 1):
            set_packing(hip, model, mode)
            out = model.forward_views(views)
            got[mode] = ({(s, v): model.debug_tensor(s, v) for s in STAGES for v in range(3)},
                         [{k: t.cpu().numpy() for k, t in o.items()} for o in out])
    finally:
        set_packing(hip, model, was)
    for key, t in got[0][0].items():
        assert t.tobytes() == got[1][0][key].tobytes(), "stage %s of view %d differs between per-view and packed row tiles" % key
    for v in range(3):
        for k, t in got[0][1][v].items():
            assert t.tobytes() == got[1][1][v][k].tobytes(), "output %s of view %d differs" % (k, v)
    p5 = [got[1][0][("P5", v)].shape[:2] for v in range(3)]
    assert len(set(p5)) >= 2 and sum(h * w for h, w in p5) < 3 * 128, p5        # ragged, and a handful of rows per view
    for v, im in enumerate(imgs):
        keep = {}
        want = oracle.frcnn_forward(P, im, MIN_SIZE, MAX_SIZE, flip=(v == 1), rects=None, keep=keep)
        stages = [("input", keep["input"]), ("conv1", keep["conv1"]), ("pool1", keep["pool1"])]
        stages += [("C%d" % (i + 2), keep["C"][i]) for i in range(4)]
        stages += [("P%d" % (i + 2), keep["fpn"][i]) for i in range(5)]
        stages += [("rpn%d" % i, keep["rpn_head"][i]) for i in range(5)]
        for name, w in stages:
            g = got[1][0][(name, v)]
            assert g.shape == w.shape, (name, v, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), "view %d stage %s differs from the oracle: max abs %g" % (v, name, float(np.abs(g - w).max()))
        n = keep["proposals"].shape[0]
        assert got[1][0][("proposals", v)].reshape(-1, 4)[:n].tobytes() == keep["proposals"].tobytes(), "view %d: proposals differ" % v
        for name in ("roi", "fc7", "pred"):
            g = got[1][0][(name, v)].reshape(1000, -1)[:n]
            assert g.tobytes() == keep[name].reshape(n, -1).tobytes(), "view %d stage %s differs from the oracle" % (v, name)
        for k in ("boxes", "scores", "labels", "props", "prob_max", "scores_cls"):
            assert got[1][1][v][k].tobytes() == want[k].tobytes(), "view %d output %s differs from the oracle" % (v, k)


def test_sweep_identical_packed_and_per_view(hip, tiny_model):
    from cald_amd import synth, sweep
    torch = hip["torch"]
    model, _ = tiny_model
    pool = synth.make_pool(6, "voc", 0, scale=0.5)
    dev = [torch.from_numpy(im).cuda() for im in pool]
    res = {}
    was = set_packing(hip, model, 0)
    try:
        for mode in (0, 1):
            set_packing(hip, model, mode)
            res[mode] = sweep.sweep_device_images(model, dev, list(range(len(pool))), ["flip", "cut_out", "smaller_resize"], bp=1.3, base_seed=3,
                                                  batch_images=4)
    finally:
        set_packing(hip, model, was)
    assert np.asarray(res[0][0]).tobytes() == np.asarray(res[1][0]).tobytes(), "consistency differs between per-view and packed row tiles"
    assert np.asarray(res[0][1]).tobytes() == np.asarray(res[1][1]).tobytes(), "cls_corr differs between per-view and packed row tiles"
    assert np.all(np.isfinite(np.asarray(res[1][0])))
