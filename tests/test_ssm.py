"""CPU tests of the SSM method (cald_amd/ssm.py) and of the tail's restatement (tests/_ssm_restatement.py) against tests/golden/ssm.npz,
the recorded outputs of the reference's own ssm_postprocess_detections, judge_y, judge_uv, calcu_iou and image_cross_validation
(tools/make_golden_ssm.py).  The GPU side is tests/test_gpu_ssm.py."""
import random

import numpy as np
import pytest
import torch

import _ssm_restatement as R
from cald_amd import ssm


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ssm")


def test_the_oracles_exp_is_exact_where_the_boundary_cases_need_it(oracle):
    R.check_exp(oracle)


def test_restatement_matches_the_executed_reference_tail(oracle, fx):
    """al, row counts, row order and labels exactly; probabilities to 1e-5 and boxes to 1e-3, the tolerances of the existing tail against
    the executed reference (test_frcnn_postprocess_kernels_match_the_reference_method_body): the reference computes with torch's exp."""
    assert int(fx["t_n"]) == 4
    seen_al = set()
    for k in range(int(fx["t_n"])):
        H, W = [int(v) for v in fx["t%d_hw" % k]]
        margins = {}
        got = R.ssm_tail(oracle, fx["t%d_logits" % k], fx["t%d_deltas" % k], fx["t%d_props" % k], H, W, H, W, margins=margins)
        want_scores, want_boxes, want_labels = fx["t%d_scores" % k], fx["t%d_boxes" % k], fx["t%d_labels" % k]
        assert got["al"] == int(fx["t%d_al" % k])
        seen_al.add(got["al"])
        assert got["boxes"].shape == want_boxes.shape and got["scores"].shape == want_scores.shape
        assert np.array_equal(got["labels"], want_labels)
        assert np.abs(got["scores"] - want_scores).max(initial=0.0) <= 1e-5
        assert np.abs(got["boxes"] - want_boxes).max(initial=0.0) <= 1e-3
        # the row order: every row's class is the column of its own score that the per-class sort used; rows of a class are score-descending
        if len(got["cls"]):
            assert np.all(np.diff(got["cls"]) >= 0)
            own = want_scores[np.arange(len(got["cls"])), got["cls"] - 1]
            for c in np.unique(got["cls"]):
                assert np.all(np.diff(own[got["cls"] == c]) <= 0)
        # the fixture's decisions do not hang on a last bit, here as in the reference's run
        rec = fx["t%d_margins" % k]
        assert rec[0] > 1e-4 and rec[1] > 1e-5 and rec[2] > 1e-5
        assert margins["iou"] > 5e-5 and margins["thr"] > 5e-6 and margins["half"] > 5e-6
    assert seen_al == {0, 1}


def test_judge_y_is_a_comparison_with_one_half(fx):
    """judge_y (frcnn_ssm.py:29-39) on 0, 1 and the 2 000 floats on each side of 0.5 is +1 exactly where the score is > 0.5: what the
    kernel writes."""
    x, y = fx["jy_in"], fx["jy_out"]
    assert x.size == 4003 and x[0] == 0 and x[1] == 1 and np.float32(0.5) in x
    assert np.array_equal(y, np.where(x > np.float32(0.5), 1, -1).astype(np.int8))


def test_judge_uv_matches_the_reference(fx):
    flags = []
    for loss, gamma, lam, flag, v in zip(fx["uv_loss"], fx["uv_gamma"], fx["uv_lambda"], fx["uv_flag"], fx["uv_v"]):
        got_flag, got_v = ssm.judge_uv(loss, gamma, lam)
        assert bool(got_flag) == bool(flag) and got_v.dtype == np.float64 and np.array_equal(got_v, v)
        flags.append(bool(flag))
    assert True in flags and False in flags
    eq = ssm.judge_uv(np.array([0.25, 0.25, 0.5]), 1.0, np.array([0.5, 0.5, 0.5]))        # lsum == gamma falls through
    assert eq[0] is True and not eq[1].any()


def test_calcu_iou_matches_the_reference(fx):
    for a, b, want in zip(fx["iou_a"], fx["iou_b"], fx["iou_out"]):
        assert float(ssm.calcu_iou(list(a), list(b))) == want
    assert ssm.calcu_iou([0, 0, 4, 4], [20, 20, 30, 30]) == 0


def test_softmax_is_the_flattened_exponential_ratio():
    a = np.array([[0.1, -2.0], [3.0, 0.5]])
    got = ssm.softmax(a)
    e = np.exp(a.flatten())
    assert got.shape == (4,) and np.array_equal(got, e / np.sum(e))


def test_box_loss_in_the_references_mixed_arithmetic():
    """ssm_train.py:228-229 evaluated literally (float32 logs, float64 label factors), scores 0 and 1 included: a score of 1 under +1 costs
    nothing, under -1 log(1e-30); a score of 0 under -1 is 0 * -inf = NaN, which judge_uv lets through as (True, zeros)."""
    score = np.array([1.0, 1.0, 0.0, 0.0, 0.3, 0.8], np.float32)
    label = np.array([1, -1, 1, -1, -1, 1], np.int64)
    got = ssm.box_loss(score, label)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = -((1 + label) / 2 * np.log(score) + (1 - label) / 2 * np.log(1 - score + 1e-30))
    assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
    assert got[0] == 0 and got[1] == -np.float64(np.log(np.float32(1e-30))) and got[2] == np.inf and np.isnan(got[3])
    assert got[4] == -np.float64(np.log(np.float32(1) - np.float32(0.3))) and got[5] == -np.float64(np.log(np.float32(0.8)))
    flag, v = ssm.judge_uv(got, 1.0, np.full(6, 0.5))
    assert flag is True and not v.any()


# views per forward the batching must show: 5, then 5 - curr_select (derived by hand from the scenes' scripts)
FORWARDS = {"five_straight": [5], "rounds_5_2_1": [5, 2, 1], "loader_ends": [3], "empty_patch": []}


@pytest.mark.parametrize("s", range(len(R.SCENES)), ids=[sc["name"] for sc in R.SCENES])
def test_image_cross_validation_follows_the_references_run(fx, s):
    scene = R.SCENES[s]
    _, labeled = R.scene_loaders(scene, torch, as_float=False)
    before = [im[0].clone() for im, _ in labeled]
    model = R.ScriptedModel(scene, torch)
    curr, _ = R.scene_loaders(scene, torch, as_float=False)
    random.seed(scene["seed"])
    flag, score = ssm.image_cross_validation(model, curr, labeled, scene["pre_box"], torch.tensor([scene["pre_cls"]]))
    state = np.array(random.getstate()[1], np.int64)
    assert bool(flag) == bool(fx["x%d_flag" % s]) and float(score) == float(fx["x%d_score" % s])
    assert np.array_equal(state, fx["x%d_state" % s])                       # the same number of random draws
    assert [k for call in model.calls for k in call] == fx["x%d_visited" % s].tolist()
    assert [r for _, r in model.pastes] == fx["x%d_pastes" % s].tolist()     # the same places, so the same draws in the same order
    assert [len(c) for c in model.calls] == FORWARDS[scene["name"]]
    assert model.modes == [False]
    for (im, _), b in zip(labeled, before):                                  # the loader's images are pasted into as copies
        assert torch.equal(im[0], b)


def test_image_cross_validation_also_reads_float_chw_images(fx):
    """What a torchvision loader yields (to_tensor's float32 CHW) gives the same run."""
    flag, score, model, state = R.run_scene(ssm.image_cross_validation, R.SCENES[1], torch, as_float=True)
    assert flag == bool(fx["x1_flag"]) and score == float(fx["x1_score"]) and np.array_equal(state, fx["x1_state"])


class _SelectModel:
    """image_cross_validation's model for ssm_select: class-`cls` detections on the pasted rectangle when the candidate's image is in
    `passing`, none otherwise (the candidate's image is recognised by its patch colour)."""

    def __init__(self, passing):
        self.passing, self.seen = passing, []

    def eval(self):
        return self

    def ssm_mode(self, flag):
        pass

    def __call__(self, images):
        out = []
        for img in images:
            a = img.cpu().numpy()
            tag = int(a[..., 0].max())                       # the patch's channel 0 = 200 + candidate index
            ys, xs = np.nonzero(a[..., 0] == tag)
            rect = [float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1)]
            self.seen.append(tag - 200)
            ok = (tag - 200) in self.passing
            out.append(dict(labels=torch.tensor([2] if ok else [7]), boxes=torch.tensor([rect]), scores=torch.tensor([0.9])))
        return out


def _select_setup():
    """Pool images 100..105 swept in this order; 101 was flagged by stage 1 (al).  Per remaining position i the lists hold, as in the
    reference, the detections of the i-th image WITH al == 0 -- while subset[i] indexes the set-difference list."""
    K = 4
    pool = [100, 101, 102, 103, 104, 105]

    def img(idx):
        a = np.full((40, 40, 3), 10, np.uint8)
        a[..., 0] = 200 + (idx - 100) if idx in pool else 10
        return torch.from_numpy(a)

    def factory(indices, shuffle):
        return [([img(i)], [{"labels": torch.tensor([9])}]) for i in indices]

    sure = [0.01, 0.01, 0.97, 0.01]          # one confident class at index 2: small loss, goes to the cross-validation
    first = [0.97, 0.01, 0.01, 0.01]         # the only +1 at index 0: skipped by the `!= 0` test
    vague = [0.45, 0.45, 0.45, 0.45]         # a large summed loss: fails judge_uv
    allScore = [torch.tensor([first, sure], dtype=torch.float32), torch.tensor([vague], dtype=torch.float32),
                torch.tensor([sure, sure], dtype=torch.float32), torch.tensor([sure], dtype=torch.float32), torch.tensor([sure], dtype=torch.float32)]
    allY = [np.where(s.numpy() > 0.5, 1, -1).tolist() for s in allScore]
    allBox = [torch.tensor([[2.0, 3.0, 12.0, 15.0]] * len(s)) for s in allScore]
    return K, pool, factory, allScore, allBox, allY


def test_ssm_select_walks_the_references_stage_two():
    K, pool, factory, allScore, allBox, allY = _select_setup()
    lam0 = np.full(K, 0.6)
    subset = list(set(pool) - {101})
    labeled = [900, 901, 902, 903, 904, 905]
    # position 0: box 0 skipped by `!= 0`, box 1 passes the cross-validation; 1: fails judge_uv; 2: fails the validation; 3, 4: pass
    passing = {subset[0] - 100, subset[3] - 100, subset[4] - 100}
    model = _SelectModel(passing)
    random.seed(5)
    al, gamma, lam = ssm.ssm_select(model, factory, pool, labeled, allScore, allBox, allY, [101], 4, 0.5, lam0)
    assert al[:3] == [101, subset[1], subset[2]]
    assert len(al) == 4 and al[3] in set(subset) - {subset[1], subset[2]}           # the fill-up to the budget
    assert gamma == min(0.5 + 0.05, 1)
    # the pace update from the losses of every box the loop reached; cls_sum counts the boxes of every image it reached (2 + 1 + 2 + 1 + 1)
    total = np.zeros(K)
    for i, j in [(0, 0), (0, 1), (1, 0), (2, 0), (3, 0), (4, 0)]:
        total += ssm.box_loss(allScore[i][j].numpy(), allY[i][j])
    assert np.array_equal(lam, 0.9 * lam0 - 0.1 * np.log(ssm.softmax(total / (7 + 1e-30))))
    # the validations that ran: five pasted images for a passing box; all six labeled images (5 + 1) for the one no detection answers
    want_seen = [subset[0] - 100] * 5 + [subset[2] - 100] * 6 + [subset[3] - 100] * 5 + [subset[4] - 100] * 5
    assert model.seen == want_seen

    # a budget the loop itself fills: it stops before position 3
    model = _SelectModel(passing)
    al, _, _ = ssm.ssm_select(model, factory, pool, labeled, allScore, allBox, allY, [101], 3, 0.5, lam0)
    assert al == [101, subset[1], subset[2]] and model.seen == want_seen[:11]


def test_ssm_select_leaves_early_when_stage_one_fills_the_budget():
    K, pool, factory, allScore, allBox, allY = _select_setup()
    lam0 = np.full(K, 0.6)
    al, gamma, lam = ssm.ssm_select(None, factory, pool, [900], allScore, allBox, allY, [101, 103, 105], 2, 0.98, lam0)
    assert al == [101, 103] and gamma == 1
    assert np.array_equal(lam, 0.9 * lam0 - 0.1 * np.log(ssm.softmax(np.zeros(K) / 1e-30)))


def test_the_min_size_restatement_with_zero_is_the_oracles_tail(oracle, golden):
    """tests/_ssm_restatement.py frcnn_tail_min, which the GPU test of cald_model_set_box_min_size compares against: with min_size 0 it is the
    oracle's postprocess on the executed reference's cases, bit for bit; with 1e-2 it drops a zero-width box and nothing else."""
    g = golden("postprocess")
    for k in (0, 2):
        H, W = [int(v) for v in g["f%d_hw" % k]]
        a = (g["f%d_logits" % k], g["f%d_deltas" % k], g["f%d_props" % k], H, W, H, W)
        want = oracle.frcnn_postprocess(*a)
        got = R.frcnn_tail_min(oracle, *a, min_size=0.0)
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), (k, key)
    logits = np.full((2, 3), -5.0, np.float32); logits[:, 1] = [2.0, 3.0]
    props = np.array([[10, 10, 40, 50], [60, 20, 60, 70]], np.float32)
    a = (logits, np.zeros((2, 12), np.float32), props, 100, 100, 100, 100)
    assert oracle.frcnn_postprocess(*a)["props"].tolist() == [props[1].tolist(), props[0].tolist()]
    assert R.frcnn_tail_min(oracle, *a, min_size=1e-2)["props"].tolist() == [props[0].tolist()]
