"""CPU tests of the flat COCO evaluator (cald_amd.coco_eval.FlatCOCOeval: numpy segment table, flat match arrays, vectorised accumulate)
against COCOeval, and of the ``matching`` keyword of both evaluators' entry points.  The device side is tests/test_gpu_eval_match.py."""
import inspect

import numpy as np
import pytest

import _eval_scenes as S
from cald_amd import coco_eval as ce, engine, voc_eval as ve


@pytest.fixture(scope="module")
def scene():
    images, anns, cats, dets = S.random_scene(0)
    want = S.run(ce.COCOeval(ce.CocoGT(images, anns, cats)), images, dets)
    return images, anns, cats, dets, want


def test_scene_has_the_cases_it_is_meant_to_have(scene):
    images, anns, cats, dets, want = scene
    assert len(images) == 30 and len(cats) == 5
    assert any(a["iscrowd"] for a in anns) and any(a["area"] != a["bbox"][2] * a["bbox"][3] for a in anns) and anns[0]["id"] == 0
    assert sum(d["image_id"] == images[3]["id"] and d["category_id"] == cats[0]["id"] for d in dets) > 100
    scores = [d["score"] for d in dets]
    assert len(set(scores)) < len(scores)                     # tied scores
    assert (want.eval["precision"] > 0).any() and (want.eval["precision"] == 0).any() and len(set(np.round(want.stats, 9))) >= 8


def test_flat_host_equals_cocoeval_on_the_random_scene(scene):
    images, anns, cats, dets, want = scene
    got = S.run(ce.FlatCOCOeval(ce.CocoGT(images, anns, cats), matching="host"), images, dets)
    S.assert_same_eval(got, want)
    assert got.host_segments == len(got._chunks[0].seg_cat) > 50


def test_flat_host_equals_cocoeval_when_updated_in_batches(scene):
    """CocoEvaluator.update arrives once per batch in the reference's loop: several evaluate() calls, and one image evaluated twice."""
    images, anns, cats, dets, _ = scene
    want = S.run(ce.COCOeval(ce.CocoGT(images, anns, cats)), images, dets, batches=4)
    got = S.run(ce.FlatCOCOeval(ce.CocoGT(images, anns, cats)), images, dets, batches=4)
    S.assert_same_eval(got, want)
    again = [images[3]["id"], images[4]["id"]]
    for ev in (want, got):
        ev.evaluate(again); ev.accumulate(); ev.summarize(quiet=True)
    S.assert_same_eval(got, want)


def test_flat_evaluator_through_cocoevaluator_arrays(scene):
    """add_predictions (arrays straight from the detector's output dicts) == prepare_for_coco_detection + add_results."""
    images, anns, cats, dets, want = scene
    preds = {}
    for im in images:
        mine = [d for d in dets if d["image_id"] == im["id"]]
        b = np.array([d["bbox"] for d in mine], np.float64).reshape(-1, 4)
        preds[im["id"]] = {"boxes": np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1), "scores": np.array([d["score"] for d in mine]),
                           "labels": np.array([d["category_id"] for d in mine], np.int64)}
    got = ce.FlatCOCOeval(ce.CocoGT(images, anns, cats))
    got.add_predictions(preds)
    got.evaluate(list(preds)); got.accumulate(); got.summarize(quiet=True)
    S.assert_same_eval(got, want)


def test_flat_host_on_the_known_answer_scene(golden):
    g = golden("coco_ap_known_answers")
    images, anns, cats, dets = S.golden_scene(g)
    want = S.run(ce.COCOeval(ce.CocoGT(images, anns, cats)), images, dets)
    got = S.run(ce.FlatCOCOeval(ce.CocoGT(images, anns, cats), matching="host"), images, dets)
    S.assert_same_eval(got, want)
    np.testing.assert_allclose(got.stats, g["stats"], rtol=0, atol=1e-12)


def test_empty_evaluations():
    images, anns, cats, dets = S.random_scene(1, n_img=4, n_cat=2)
    for a, d in ((anns, []), ([], dets), ([], [])):
        want = S.run(ce.COCOeval(ce.CocoGT(images, a, cats)), images, d)
        got = S.run(ce.FlatCOCOeval(ce.CocoGT(images, a, cats)), images, d)
        S.assert_same_eval(got, want)


TOUCHED = [ce.CocoEvaluator.__init__, ce.FlatCOCOeval.__init__, ve.voc_eval_thresholds, ve.do_python_eval, engine.voc_evaluate, engine.coco_evaluate]


def test_matching_defaults_to_host_everywhere():
    for fn in TOUCHED:
        assert inspect.signature(fn).parameters["matching"].default == "host", fn
    images, anns, cats, _ = S.random_scene(1, n_img=2, n_cat=2)
    assert type(ce.CocoEvaluator(ce.CocoGT(images, anns, cats)).coco_eval["bbox"]) is ce.COCOeval


def test_unknown_matching_raises_value_error(tmp_path):
    images, anns, cats, _ = S.random_scene(1, n_img=2, n_cat=2)
    gt = ce.CocoGT(images, anns, cats)
    calls = [lambda: ce.CocoEvaluator(gt, ["bbox"], matching="gpu"), lambda: ce.FlatCOCOeval(gt, matching="gpu"),
             lambda: ve.voc_eval_thresholds("cat", str(tmp_path / "none.txt"), None, matching="gpu"),
             lambda: ve.do_python_eval(None, "2007", "res", matching="gpu"),
             lambda: engine.voc_evaluate(None, None, "2007", matching="gpu"), lambda: engine.coco_evaluate(None, None, matching="gpu")]
    for call in calls:
        with pytest.raises(ValueError, match="matching"):
            call()


def test_device_matching_raises_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    images, anns, cats, dets = S.random_scene(1, n_img=2, n_cat=2)
    ev = ce.FlatCOCOeval(ce.CocoGT(images, anns, cats), matching="device")
    ev.add_results(dets)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.evaluate([im["id"] for im in images])
    fn = tmp_path / "det.txt"
    fn.write_text("a 0.9 1.0 1.0 9.0 9.0\n")
    ann = ve.VocAnnotations.__new__(ve.VocAnnotations)
    ann._per_class = {"cat": ({"a": (np.array([[1., 1., 9., 9.]]), np.array([False]))}, 1)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ve.voc_eval_thresholds("cat", str(fn), ann, matching="device")
    assert len(ve.voc_eval_thresholds("cat", str(fn), ann)) == 10


def test_device_matching_refuses_several_ranks(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    images, anns, cats, _ = S.random_scene(1, n_img=2, n_cat=2)
    gt = ce.CocoGT(images, anns, cats)
    for call in (lambda: ce.CocoEvaluator(gt, ["bbox"], matching="device"), lambda: ce.FlatCOCOeval(gt, matching="device")):
        with pytest.raises(NotImplementedError):
            call()
    assert type(ce.CocoEvaluator(gt, ["bbox"]).coco_eval["bbox"]) is ce.COCOeval      # the host path is untouched by it
