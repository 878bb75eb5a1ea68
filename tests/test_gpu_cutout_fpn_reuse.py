"""cut_out reuse through the FPN output convs (cutout_reuse.hip retain / cut_plan, forward.hip fpn, conv_p4.hip's grouped gathered launch with the
pruning's extras): the cut_out forward patches the reference forward's retained P2..P5 -- and, under the certified pruning, P2 / P3's split
copy and energy -- on the output dirty sets.  Nothing may change by a bit: sweeps with the reuse off, on, and on with every stage dense;
single cut_out forwards tensor by tensor; pruning on and off; the extended retention slot refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYER1, LAYER4, LATERAL, OUTPUT = 0, 3, 4, 5
KEPT_FPN, KEPT_STAGES, KEPT_NONE = 0, 1, 2


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


@pytest.fixture(scope="module")
def model(hip):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    m = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=300, max_size=500).to("cuda")
    m.load_state_dict(sd)
    m.eval()
    return m


def set_reuse(hip, model, mode):
    was = C.c_int()
    hip["ffi"].check(hip["L"].cald_model_set_cutout_reuse(model.handle(), mode, C.byref(was)))
    return was.value


def set_cap(hip, model, nbytes):
    was = C.c_int64()
    hip["ffi"].check(hip["L"].cald_model_set_cutout_retention_cap(model.handle(), nbytes, C.byref(was)))
    return was.value


def stages(hip):
    """(rows[6], dense rows[6], tiles[6], dense tiles[6], kept[3]) of the context so far"""
    ffi = hip["ffi"]
    a = [np.zeros(6) for _ in range(4)]
    kept = np.zeros(3, np.int64)
    ffi.check(hip["L"].cald_profile_cutout_stages(hip["ctx"], *[ffi.ptr(x, ffi.c_d) for x in a], ffi.ptr(kept, ffi.c_i64)))
    return a + [kept]


def delta(after, before):
    return [x - y for x, y in zip(after, before)]


def sweep_modes(hip, model, pool, augs, **kw):
    """(consistency, cls_corr) with the reuse off; asserts the same bytes with it on and forced dense; the stage counters of the `on` run"""
    from cald_amd import sweep
    dev = [hip["torch"].from_numpy(im).cuda() for im in pool]
    res = {}
    for mode in (0, 1, 2):
        was = set_reuse(hip, model, mode)
        try:
            before = stages(hip)
            res[mode] = sweep.sweep_device_images(model, dev, list(range(len(pool))), augs, **kw)
            if mode == 1:
                d = delta(stages(hip), before)
        finally:
            set_reuse(hip, model, was)
    for mode in (1, 2):
        np.testing.assert_array_equal(res[mode][0], res[0][0])
        np.testing.assert_array_equal(res[mode][1], res[0][1])
    return res[0], d


def wide_pool(n):
    """300 x 500 images (scale 1 at min / max 300 / 500, padded to 320 x 512), the widest view of this model: a rectangle near a short side
    leaves part of the pyramid clean, which smaller views never do (a rectangle's dirty set grows by about 240 input pixels to each side)"""
    from cald_amd import synth
    return [synth.synth_image(40 + i, 300, 500) for i in range(n)]


@pytest.mark.parametrize("prune", [True, False])
def test_sweep_modes_are_bit_identical_and_the_fpn_computes_fewer_rows(hip, model, prune):
    """one image per batch, so the gate decides image by image; multi_cut_out's first view (one rectangle) is the reused one"""
    was_p = model.set_rpn_prune(prune)
    try:
        (cons, cls), (rows, dense, tiles, dtiles, kept) = sweep_modes(hip, model, wide_pool(12), ["flip", "multi_cut_out", "smaller_resize"], bp=1.3,
                                                                      base_seed=3, batch_images=1)
    finally:
        model.set_rpn_prune(was_p)
    print("rows", rows, "dense", dense, "tiles", tiles, "dense tiles", dtiles, "kept", kept, "consistency", cons)
    assert list(kept) == [12, 0, 0]                                  # every batch took the extended slot: no fallback
    assert rows[OUTPUT] < dense[OUTPUT] and tiles[OUTPUT] < dtiles[OUTPUT]
    assert np.all(rows <= dense) and np.all(tiles <= dtiles)
    assert rows[LAYER4] == dense[LAYER4] and rows[LATERAL] == dense[LATERAL]      # these two stages run dense
    assert (cons > 0).sum() >= 6


# single cut_out forwards: 300 x 500 images (scale 1, padded to 320 x 512: P2 is 80 x 128, P5 10 x 16)
FORWARD_VIEWS = [
    ("corner", [[0, 0, 25, 15]]),                                   # touches two borders; the FPN sets leave the far side clean
    ("two", [[10, 20, 40, 50], [300, 200, 360, 250]]),              # their sets overlap from P3 up
    ("large", [[150, 60, 250, 120]]),                               # 20 % x 20 %: C5 is all dirty
    ("none", []),                                                   # empty sets
    # two bars across two bars: eight disjoint runs in layer1, all a GatherSet holds (CALD_GATHER_RECTS) -- and the most four rectangles were
    # found to give (200 000 random draws): the whole-view path behind a ninth run is not reachable through cutout rectangles
    ("hash", [[0, 80, 500, 100], [0, 200, 500, 220], [120, 0, 140, 300], [340, 0, 360, 300]]),
    ("none", []),
    ("none", []),
]
NAMES = ["C2", "C3", "C4", "C5", "inner2", "inner3", "inner4", "inner5", "P2", "P3", "P4", "P5", "P6"]


def forward_tensors(hip, model, mode, prune, views):
    """the cut_out forward of `views` under reuse mode `mode`: named tensors of every view, the detections, the look-ahead's selected fractions"""
    ffi, L = hip["ffi"], hip["L"]
    was = set_reuse(hip, model, mode)
    ffi.check(L.cald_profile_enable(hip["ctx"], 1))
    try:
        before = stages(hip)
        dets = model.debug_cutout_forward(views, prune=prune)
        d = delta(stages(hip), before)
        sel = np.zeros(2)
        ffi.check(L.cald_profile_prune(hip["ctx"], None, None, ffi.ptr(sel, ffi.c_d), None, None))
        t = {(n, v): model.debug_tensor(n, v) for n in NAMES for v in range(len(views))}
        t.update({("proposals", v): model.debug_tensor("proposals", v) for v in range(len(views))})
    finally:
        ffi.check(L.cald_profile_enable(hip["ctx"], 0))
        set_reuse(hip, model, was)
    dets = [{k: x.cpu().numpy() for k, x in dd.items()} for dd in dets]
    return t, dets, sel, d


@pytest.mark.parametrize("prune", [True, False])
def test_cut_out_forward_tensors_are_bit_identical(hip, model, prune):
    from cald_amd import synth
    torch = hip["torch"]
    views = [(torch.from_numpy(synth.synth_image(20 + i, 300, 500)).cuda(), False, np.array(r, np.int32) if r else None)
             for i, (_, r) in enumerate(FORWARD_VIEWS)]
    was_p = model.set_rpn_prune(prune)
    try:
        ref = forward_tensors(hip, model, 0, prune, views)
        for mode in (1, 2):
            got = forward_tensors(hip, model, mode, prune, views)
            for key in ref[0]:
                assert np.array_equal(got[0][key].view(np.uint32), ref[0][key].view(np.uint32)), (mode, key)
            for v in range(len(views)):
                assert sorted(got[1][v]) == sorted(ref[1][v])
                for k in ref[1][v]:
                    np.testing.assert_array_equal(got[1][v][k], ref[1][v][k], err_msg="mode %d view %d %s" % (mode, v, k))
            np.testing.assert_array_equal(got[2], ref[2])            # the look-ahead selected the same fractions of P2 / P3
            rows, dense, tiles, dtiles, kept = got[3]
            print("mode", mode, "rows", rows, "dense", dense, "tiles", tiles, "dense tiles", dtiles, "kept", kept, "selected", got[2])
            assert list(kept) == [1, 0, 0]
            if mode == 1:
                assert rows[OUTPUT] < dense[OUTPUT] and rows[LAYER1] < dense[LAYER1]       # the FPN outputs and layer1 ran gathered
            else:
                assert rows[OUTPUT] == dense[OUTPUT]
        assert prune == bool(ref[2].max() > 0)
        assert sum(len(d["scores"]) for d in ref[1]) > 0
    finally:
        model.set_rpn_prune(was_p)


def test_view_without_rectangles_launches_nothing_in_the_fpn(hip, model):
    """every set empty: the cut_out forward computes no FPN output row and returns the reference forward's tensors"""
    from cald_amd import synth
    torch = hip["torch"]
    views = [(torch.from_numpy(synth.synth_image(31, 300, 500)).cuda(), False, None)]
    ref = forward_tensors(hip, model, 0, True, views)
    got = forward_tensors(hip, model, 1, True, views)
    for key in ref[0]:
        assert np.array_equal(got[0][key].view(np.uint32), ref[0][key].view(np.uint32)), key
    rows, dense, tiles, dtiles, kept = got[3]
    assert rows[OUTPUT] == 0 and tiles[OUTPUT] == 0 and dense[OUTPUT] > 0 and rows[LAYER1] == 0


def test_pipelined_batches_and_the_refused_extended_slot(hip, model):
    """7 batches of 3 images over two retention slots; then the same with the extended slot refused by the test cap: the three-stage retention
    takes over, the counter says so, the bytes stay"""
    from cald_amd import synth
    pool = synth.make_pool(20, "voc", 1, scale=0.5)
    augs = ["flip", "cut_out", "smaller_resize"]
    base, (rows, dense, tiles, dtiles, kept) = sweep_modes(hip, model, pool, augs, base_seed=7, batch_images=3)
    assert list(kept) == [7, 0, 0]
    was = set_cap(hip, model, 1 << 20)                               # 1 MB: every extended slot is above it
    try:
        capped, (rows, dense, tiles, dtiles, kept) = sweep_modes(hip, model, pool, augs, base_seed=7, batch_images=3)
    finally:
        set_cap(hip, model, was)
    assert list(kept) == [0, 7, 0]
    assert rows[OUTPUT] == dense[OUTPUT] and rows[LAYER1] < dense[LAYER1]         # the FPN ran dense, the three stages still reuse
    np.testing.assert_array_equal(capped[0], base[0])
    np.testing.assert_array_equal(capped[1], base[1])
