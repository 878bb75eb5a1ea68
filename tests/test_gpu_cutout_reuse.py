"""cut_out reuse (cutout_reuse.hip CutPlanner + conv_p4.hip's gathered rows): the batch's cut_out views recompute only the pixels of their first
three stages that the filled rectangles reach, over the reference forward's retained block outputs.  The results must not change by a
bit: reuse on, off, and on with every stage forced dense give identical consistency and cls_corr."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


def make_model(hip, min_size, max_size):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    model = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=min_size, max_size=max_size).to("cuda")
    model.load_state_dict(sd)
    model.eval()
    return model, sd


def set_reuse(hip, model, mode):
    was = C.c_int()
    hip["ffi"].check(hip["L"].cald_model_set_cutout_reuse(model.handle(), mode, C.byref(was)))
    return was.value


def counters(hip):
    rows = np.zeros(3); dense = np.zeros(3); nb = C.c_int64(); nf = C.c_int64()
    ffi = hip["ffi"]
    ffi.check(hip["L"].cald_profile_cutout(hip["ctx"], ffi.ptr(rows, ffi.c_d), ffi.ptr(dense, ffi.c_d), C.byref(nb), C.byref(nf)))
    return rows, dense, nb.value, nf.value


def sweep_modes(hip, model, pool, augs, pos=None, **kw):
    """(consistency, cls_corr) with reuse off, on, and on with every stage dense; the counters' change over the `on` run."""
    from cald_amd import sweep
    torch = hip["torch"]
    dev = [torch.from_numpy(im).cuda() for im in pool]
    pos = list(range(len(pool))) if pos is None else pos
    res = {}
    for mode in (0, 1, 2):
        was = set_reuse(hip, model, mode)
        try:
            before = counters(hip)
            res[mode] = sweep.sweep_device_images(model, dev, pos, augs, **kw)
            after = counters(hip)
        finally:
            set_reuse(hip, model, was)
        if mode == 1:
            delta = [a - b for a, b in zip(after, before)]
    for mode in (1, 2):
        np.testing.assert_array_equal(res[mode][0], res[0][0])
        np.testing.assert_array_equal(res[mode][1], res[0][1])
    return res[0], delta


def test_small_config1_reuse_is_bit_identical(hip):
    from cald_amd import synth
    model, _ = make_model(hip, 300, 500)
    pool = synth.make_pool(10, "voc", 0, scale=0.5)
    augs = ["flip", "cut_out", "smaller_resize"]
    for bi in (4, 64):
        (cons, cls), (rows, dense, nb, nf) = sweep_modes(hip, model, pool, augs, bp=1.3, base_seed=3, batch_images=bi)
        assert nb == (10 + bi - 1) // bi and nf == 0
        assert rows[0] < 0.5 * dense[0], (rows, dense)           # layer1 recomputed a small part of its rows
        assert np.all(rows <= dense)
        assert (cons > 0).sum() >= 5


def test_full_size_config1_reuse_is_bit_identical(hip):
    from cald_amd import synth
    model, _ = make_model(hip, 600, 1000)
    pool = synth.make_pool(6, "voc", 0)
    (cons, cls), (rows, dense, nb, nf) = sweep_modes(hip, model, pool, ["flip", "cut_out", "smaller_resize"], base_seed=2, batch_images=6)
    assert nb == 1 and nf == 0 and rows[0] < 0.5 * dense[0]
    assert len(np.unique(np.round(cons, 6))) > 3


def test_every_augmentation_with_multi_cut_out_is_bit_identical(hip):
    """cut_out and multi_cut_out together: the first cut_out augmentation reuses, the others run dense."""
    from cald_amd import synth
    model, _ = make_model(hip, 300, 500)
    pool = [np.ascontiguousarray(im[:120, :150]) for im in synth.make_pool(3, "voc", 3, scale=0.5)]
    augs = ["rotation", "flip", "ga", "multi_ga", "color_adjust", "color_swap", "sp", "multi_sp", "cut_out", "multi_cut_out",
            "multi_resize", "larger_resize", "smaller_resize"]
    sweep_modes(hip, model, pool, augs, pos=[4, 9, 11], bp=1.3, base_seed=3, batch_images=3)


def test_batch_with_images_without_detections_matches_the_oracle(hip, oracle):
    """Images without reference detections have no augmented views: the cut_out forward gives them a stand-in view whose results are
    dropped.  The mixed batch scores as the oracle does."""
    from cald_amd import synth
    model, sd = make_model(hip, 300, 500)
    black = np.zeros((150, 200, 3), np.uint8)
    gray = np.full((180, 160, 3), 128, np.uint8)
    imgs = synth.make_pool(3, "voc", 0, scale=0.5)
    pool = [imgs[0], black, imgs[1], gray, imgs[2]]
    augs = ["flip", "cut_out", "smaller_resize"]
    (cons, cls), (rows, dense, nb, nf) = sweep_modes(hip, model, pool, augs, bp=1.3, base_seed=5, batch_images=5)
    assert nb == 1
    P = oracle.prepare_frcnn(sd, 21, 50)
    wc, wcls = oracle.get_uncertainty(P, pool, augs, 21, bp=1.3, min_size=300, max_size=500, base_seed=5)
    np.testing.assert_array_equal(cons, np.array(wc))
    np.testing.assert_array_equal(cls, np.stack(wcls))


def test_pipelined_batches_share_two_retention_slots(hip):
    """Several batches in flight (batch k + 1's reference forward runs before batch k's cut_out forward): 7 batches of 3 images."""
    from cald_amd import synth
    model, _ = make_model(hip, 300, 500)
    pool = synth.make_pool(20, "voc", 1, scale=0.5)
    (cons, cls), (rows, dense, nb, nf) = sweep_modes(hip, model, pool, ["flip", "cut_out", "smaller_resize"], base_seed=7, batch_images=3)
    assert nb == 7 and nf == 0
