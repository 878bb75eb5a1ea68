"""CPU side of the training front end / target / loss edge tests: tests/_train_edges_restatement.py pinned to live torch and to the recorded
reference, and the census of its case tables -- every condition tests/test_gpu_train_edges.py relies on is asserted here from the inputs
alone, and every kernel mistake the GPU tests name is applied to the restatement and must change the expected value."""
import numpy as np
import pytest
import torch

import _train_edges_restatement as E
from oracle import torch_train as tt


def _tt_match(gt, boxes, hi, lo, low):
    return tt.matcher(tt.box_iou(torch.from_numpy(gt), torch.from_numpy(boxes)), hi, lo, low).numpy()


def _all_match_tables():
    yield "designed", E.designed_table()
    yield "designed+lonely", E.designed_table(lonely=True)
    yield "extended", E.designed_table(extended=True)
    yield "extended+lonely", E.designed_table(extended=True, lonely=True)
    for nb in E.MATCH_N_BOXES:
        for ng in E.MATCH_N_GT:
            yield "random %d x %d" % (nb, ng), E.random_match_case(nb, ng)


# ---- Matcher -----------------------------------------------------------------------------------------------------------------------
def test_designed_table_gives_the_stated_matches_under_live_torch():
    gt, boxes = E.designed_table()
    iou = tt.box_iou(torch.from_numpy(gt), torch.from_numpy(boxes)).numpy()
    for v in (0.7, 0.3, 0.5, 0.4):                           # the float32 quotients ARE the float32 thresholds
        assert (iou == np.float32(v)).any(), v
    for (hi, lo, low), want in E.DESIGNED_EXPECT.items():
        assert _tt_match(gt, boxes, hi, lo, low).tolist() == want, (hi, lo, low)
    gt4, _ = E.designed_table(lonely=True)
    assert _tt_match(gt4, boxes, 0.7, 0.3, True).tolist() == E.LONELY_EXPECT
    assert not tt.box_iou(torch.from_numpy(gt4[3:]), torch.from_numpy(boxes)).any()


def test_numpy_matcher_and_iou_equal_live_torch_on_every_table():
    for name, (gt, boxes) in _all_match_tables():
        iou = E.box_iou_np(gt, boxes)
        assert iou.tobytes() == tt.box_iou(torch.from_numpy(gt), torch.from_numpy(boxes)).numpy().tobytes(), name
        for hi, lo, low in E.MATCH_MODES:
            assert np.array_equal(E.matcher_np(iou, hi, lo, low), _tt_match(gt, boxes, hi, lo, low)), (name, hi, lo, low)


def test_numpy_matcher_equals_the_recorded_reference_matches(golden):
    """the matches torchvision's own RetinaNet matcher (0.5, 0.4, low quality) produced when the losses fixture was recorded"""
    fx = golden("train_losses")
    for i in range(int(fx["l_n"])):
        for n in range(int(fx["l%d_N" % i])):
            got = E.matcher_np(E.box_iou_np(fx["l%d_gt%d" % (i, n)], fx["l%d_anchors" % i]), 0.5, 0.4, True)
            assert np.array_equal(got, fx["l%d_matched" % i][n]), (i, n)


@pytest.mark.parametrize("hi,lo", E.THRESHOLDS)
def test_extended_table_census(hi, lo):
    gt, boxes = E.designed_table(extended=True)
    assert np.array_equal(gt, np.round(gt)) and np.array_equal(E.EXTRA_BOXES, np.round(E.EXTRA_BOXES)), "the extension is integer boxes"
    c = E.match_census(gt, boxes, hi, lo)
    for key in ("iou_eq_hi", "iou_eq_lo", "best_eq_hi", "best_eq_lo", "cand_tie", "cand_tie_kept", "gt_tie", "gt_tie_below_hi", "band_restored",
                "band_stays", "below_restored"):
        assert c[key], (key, c)
    assert not c["gt_without_overlap"]
    assert E.match_census(*E.designed_table(extended=True, lonely=True), hi, lo)["gt_without_overlap"]
    # allow_low = False over the same inputs is another answer
    iou = E.box_iou_np(gt, boxes)
    assert not np.array_equal(E.matcher_np(iou, hi, lo, True), E.matcher_np(iou, hi, lo, False))


@pytest.mark.parametrize("hi,lo", E.THRESHOLDS)
def test_random_tables_census(hi, lo):
    """For the chosen seed, over the 5 x 4 sizes: every kind of tie is present, and at the sizes that span more than one 256-thread block."""
    seen, seen_multi = {}, {}
    for nb in E.MATCH_N_BOXES:
        for ng in E.MATCH_N_GT:
            gt, boxes = E.random_match_case(nb, ng)
            assert gt.shape == (ng, 4) and boxes.shape == (nb, 4)
            for a in (gt, boxes):
                assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() <= 64 and (a[:, 2:] > a[:, :2]).all()
            for k, v in E.match_census(gt, boxes, hi, lo).items():
                seen[k] = seen.get(k, 0) + int(v)
                if nb > 256:
                    seen_multi[k] = seen_multi.get(k, 0) + int(v)
    print(hi, lo, seen, seen_multi)
    for key in ("iou_eq_hi", "iou_eq_lo", "best_eq_hi", "best_eq_lo", "cand_tie", "cand_tie_kept", "gt_tie", "gt_tie_below_hi", "band_restored",
                "band_stays", "below_restored", "gt_without_overlap"):
        # (a ground truth that nothing overlaps is rare among 257+ candidates and does not depend on the block count)
        assert seen[key] >= 1 and (seen_multi[key] >= 1 or key == "gt_without_overlap"), (key, seen, seen_multi)


@pytest.mark.parametrize("mistake", E.MATCH_MISTAKES, ids=lambda m: "%s=%s" % list(m.items())[0])
def test_every_matcher_mistake_changes_the_expected_matches(mistake):
    """`>=` for `>` in the first-maximum rule, `<=` for `<` at a threshold, the zero-overlap rule repaired, only one of the tied candidates
    restored: each gives other matches than the correct rule on the designed tables AND on some random table, for both threshold pairs."""
    for hi, lo in E.THRESHOLDS:
        hit = {}
        for name, (gt, boxes) in _all_match_tables():
            iou = E.box_iou_np(gt, boxes)
            differs = not np.array_equal(E.matcher_np(iou, hi, lo, True), E.matcher_np(iou, hi, lo, True, **mistake))
            kind = "random" if name.startswith("random") else "designed"
            hit[kind] = hit.get(kind, False) or differs
        assert hit["designed"] and hit["random"], (mistake, hi, lo, hit)
    if "below" in mistake:                                    # the threshold rule alone, without low-quality matches
        gt, boxes = E.designed_table()
        iou = E.box_iou_np(gt, boxes)
        assert not np.array_equal(E.matcher_np(iou, 0.5, 0.5, False), E.matcher_np(iou, 0.5, 0.5, False, **mistake))


# ---- AnchorGenerator ---------------------------------------------------------------------------------------------------------------
def test_anchor_restatement_equals_the_recorded_reference_anchors(golden):
    """tests/golden/train_losses.npz: the anchors torchvision's AnchorGenerator itself produced (RetinaNet's set, kind 1)"""
    fx = golden("train_losses")
    uneven = 0
    for i in range(int(fx["l_n"])):
        Hp, Wp = [int(v) for v in fx["l%d_hw" % i]]
        level_hw = [tuple(int(v) for v in hw) for hw in fx["l%d_level_hw" % i]]
        assert E.anchors_np(1, Hp, Wp, level_hw).tobytes() == fx["l%d_anchors" % i].tobytes(), i
        uneven += any(Hp % h or Wp % w for h, w in level_hw)
    print("recorded cases with a level that does not divide the padded size:", uneven)


def test_base_anchors_equal_the_oracle(oracle):
    for l, sizes in enumerate(E.anchor_sizes(0)):
        assert E.base_anchors_np(sizes).tobytes() == oracle.base_anchors(list(sizes), list(E.RATIOS)).reshape(-1, 4).tobytes(), l
    for l, sizes in enumerate(E.anchor_sizes(1)):                # the oracle's order for several sizes is the generator's: ratio major
        assert E.base_anchors_np(sizes).tobytes() == oracle.base_anchors(list(sizes), list(E.RATIOS)).reshape(-1, 4).tobytes(), l
    assert E.anchor_sizes(1)[0] == (32.0, 40.0, 50.0) and E.anchor_sizes(1)[4] == (512.0, 645.0, 812.0)


def test_anchor_cases_census_and_mistakes():
    Hp, Wp = E.ANCHOR_PAD
    strides = {}
    for kind, hp, wp, level_hw in E.ANCHOR_CASES:
        assert len(level_hw) == 5
        got = E.anchors_np(kind, hp, wp, level_hw)
        assert got.shape == (sum(h * w for h, w in level_hw) * (9 if kind else 3), 4)
        strides[(kind, hp, wp)] = [(hp // h, wp // w) for h, w in level_hw]
        for mistake in ("fixed", "square", "ceil"):
            differs = not np.array_equal(got, E.anchors_np(kind, hp, wp, level_hw, stride=mistake))
            if (hp, wp) == (Hp, Wp):
                assert differs, (kind, mistake)              # a fixed 4 << l stride, one stride for both axes, a quotient rounded up: all seen
    assert strides[(0, Hp, Wp)][4] == (48, 53) and strides[(1, Hp, Wp)][3:] == [(48, 53), (96, 80)]
    assert any(lv[-1] == (1, 1) for _, _, _, lv in E.ANCHOR_CASES)
    for kind in (0, 1):                                       # one divisible shape per kind: the nominal strides
        assert any(k == kind and all(hp % h == 0 and wp % w == 0 for h, w in lv) for k, hp, wp, lv in E.ANCHOR_CASES)


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------
def test_pool_inputs_census():
    """all-negative inputs give all-negative maxima and a zero-padded border would not; the NaN and -inf pixels are where the table says"""
    zero_pad_seen = 0
    for H, W in E.POOL_HW:
        for N in E.POOL_N:
            x = E.pool_input("negative", N, H, W, 4)
            want = E.pool_ref(x, True)
            assert x.max() < 0 and want.max() < 0 and want.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 4)
            zero_pad_seen += int(not np.array_equal(want, E.pool_ref(x, True, pad_value=0.0)))
            assert E.pool_ref(x, True).tobytes() == E.pool_ref(x, True, pad_value=float("-inf")).tobytes()
            x = E.pool_input("nan", N, H, W, 4)
            assert np.isnan(x[:, H // 2, W // 2]).all() and np.isnan(x[:, 0, W - 1, 0]).all() and np.isnan(E.pool_ref(x, True)).any()
            if W > 1 and H > 1:
                assert not np.isnan(x[:, 0, W - 1, 1]).any() or (H // 2, W // 2) == (0, W - 1)
            x = E.pool_input("neg_inf", N, H, W, 4)
            assert np.isneginf(x).sum() == N * 4
            assert np.array_equal(E.pool_ref(x, False), x[:, ::2, ::2])
    assert zero_pad_seen == len(E.POOL_HW) * len(E.POOL_N), "every shape has a border window: 0 padding changes every all-negative case"
    assert np.isneginf(E.pool_ref(E.pool_input("neg_inf", 1, 1, 1, 4), True)).all()


# ---- preprocess --------------------------------------------------------------------------------------------------------------------
def test_preprocess_batches_census(oracle):
    from cald_amd import train_ops
    kinds, sources, clamp = set(), set(), 0
    for mn, mx, sizes, rem in E.PREPROCESS_BATCHES:
        resized = []
        for H, W in sizes:
            Hr, Wr, Hp, Wp = train_ops.transform_size(H, W, mn, mx)
            assert (Hr, Wr, Hp, Wp) == oracle.transform_size(H, W, mn, mx) and Hr >= 1 and Wr >= 1
            resized.append((Hr, Wr)); sources.add((H, W))
            kinds.add("up" if Hr > H else ("down" if Hr < H else "one"))
            if (Hr, Wr) == (H, W):
                kinds.add("ratio 1")
            clamp += int(max(H, W) * (mn / float(min(H, W))) > mx)
        assert len(set(resized)) == 3, "three different resized sizes under one padded size"
        assert rem is None or 0 <= rem < 3
    assert {"up", "down", "ratio 1"} <= kinds and clamp >= 1
    assert {(1, 1), (2, 3), (7, 9), (33, 31), (150, 210)} <= sources
    r = E.preprocess_remainder(5, 7)
    assert r.shape == (3, 5, 7) and r.min() >= 0 and r.max() < np.float32(1.0 / 255.0)


# ---- BoxCoder.encode and the RoI gather ------------------------------------------------------------------------------------------------
def test_encode_rows_census():
    for n in E.ENCODE_N:
        ref, prop, kind = E.encode_rows(n)
        assert ref.shape == prop.shape == (n, 4)
        for w in E.ENCODE_WEIGHTS:
            e64 = tt.encode(torch.from_numpy(ref).double(), torch.from_numpy(prop).double(), w).numpy()
            e32 = tt.encode(torch.from_numpy(ref), torch.from_numpy(prop), w).numpy()
            assert np.all(e64[kind == 0] == 0) and np.array_equal(np.isneginf(e64), np.isneginf(e32))
            assert np.array_equal(np.isneginf(e64[:, 2]), kind == 3) and not np.isneginf(e64[:, [0, 1, 3]]).any() and not np.isnan(e64).any()
            fin = ~np.isneginf(e64).any(axis=1)
            scale = max(1e-30, np.abs(e64[fin]).max())
            print("encode n=%d w=%s: torch float32 is %.3g of the largest entry from float64" % (n, w[0], np.abs(e32[fin] - e64[fin]).max() / scale))
        if n == 1:
            assert kind.tolist() == [0]
        else:
            assert set(kind[kind >= 0].tolist()) == {0, 1, 2, 3}
            wr = (ref[:, 2] - ref[:, 0]) / (prop[:, 2] - prop[:, 0])
            assert np.all(wr[kind == 1] == 1000) and np.all(wr[kind == 2] == np.float32(1e-3))
        if n == 257:
            assert (kind[:4] >= 0).all() and (kind[253:] >= 0).all(), "special rows on both sides of the 256-thread boundary"


def test_roi_cases_census():
    from cald_amd import train_ops
    R = {}
    for name in E.ROI_CASES:
        c = E.roi_case(train_ops, name)
        R[name] = c["R"]
        blk, cap = c["blk"], c["cap"]
        assert cap == len(c["slots"]) * E.ROI_CASES[name][3] and c["R"] == sum(c["per"]) and 0 <= c["n_pos"] <= c["R"] <= cap
        rois, tgt = E.roi_want(c, (10.0, 10.0, 5.0, 5.0))
        assert rois.shape == (c["R"], 5) and tgt.shape == (c["n_pos"], 4) and np.isfinite(tgt.numpy()).all()
    assert E.roi_case(train_ops, "no_foreground")["n_pos"] == 0 and R["no_foreground"] == 8
    c = E.roi_case(train_ops, "R_equals_cap")
    assert c["R"] == c["cap"] == 32 and c["n_pos"] > 0
    assert R["R_1"] == 1 and E.roi_case(train_ops, "R_1")["n_pos"] == 1
    assert R["R_255"] == 255 and R["R_257"] == 257
    assert E.roi_case(train_ops, "R_255")["n_pos"] > 0 and E.roi_case(train_ops, "R_257")["n_pos"] > 0
    c = E.roi_case(train_ops, "image_without_gt")
    blk, cap, per = c["blk"], c["cap"], c["per"]
    img = blk[5 * cap:].view(np.float32)[:c["R"]]
    mid = slice(per[0], per[0] + per[1])
    assert per[1] > 0 and np.all(img[mid] == 1.0) and np.all(blk[cap:cap + c["R"]][mid] == sum(c["n_gt"])), "rows of the image without boxes: the zero box"
    assert not c["gts"][sum(c["n_gt"])].any() and np.all(blk[2 * cap:2 * cap + c["R"]][mid] == 0) and c["n_pos"] > 0
    assert np.all(blk[cap:cap + c["R"]][per[0] + per[1]:] < sum(c["n_gt"]))


# ---- plain focal loss ---------------------------------------------------------------------------------------------------------------
def test_focal_shape_table_is_the_segmented_kernels_table():
    import test_gpu_retina_ll_ops as RL
    assert E.FOCAL_SHAPES == RL.SHAPES
    c, r = E.focal_case(*E.FOCAL_SHAPES[0], seed=3), RL._case(torch, *RL.SHAPES[0], seed=3)
    for k in ("flat", "matched", "gt_labels", "gt_off"):
        assert c[k].numpy().tobytes() == r[k].numpy().tobytes(), k


def test_focal_cases_census_and_the_block_image_mistake():
    for A, K, ld, level_pix in E.FOCAL_SHAPES:
        c = E.focal_case(A, K, ld, level_pix, seed=A * 1000 + K + level_pix[0])
        m = c["matched"]
        assert (m[0] == -1).all() and (m[1] == -2).all() and m[2, 0] >= 0 and m[2, -1] >= 0 and c["denom"][:2] == [1.0, 1.0]
        valid = torch.cat([b[:, :, :A * K].reshape(-1) for b in E.focal_blocks(c["flat"], 3, level_pix, ld)])
        pad = torch.cat([b[:, :, A * K:].reshape(-1) for b in E.focal_blocks(c["flat"], 3, level_pix, ld)])
        assert torch.isfinite(valid).all() and torch.isnan(pad).all() and (pad.numel() > 0 or ld == A * K)
        for v in (30.0, -30.0):
            assert (valid == v).any()
        assert ((valid == 0) & torch.signbit(valid)).any() and ((valid == 0) & ~torch.signbit(valid)).any()
    totals = sorted(A * sum(lp) for A, K, ld, lp in E.FOCAL_SHAPES)
    assert {256, 257, 512, 513} <= set(totals)
    # the straddling shape: N = 2, A_tot = 257, and for N in (2, 4) every denominator a power of two
    A, K, ld, level_pix = E.FOCAL_STRADDLE
    for N in (2, 4):
        c = E.focal_case(A, K, ld, level_pix, N=N, seed=11, pow2=True)
        assert c["At"] % 256 == 1 and c["denom"] == [float(2 ** (i + 1)) for i in range(N)]
        assert all(int(c["matched"][i, 0]) == 1 and int(c["matched"][i, -1]) == 2 and (c["matched"][i] == -2).any() for i in range(N))
    c = E.focal_case(A, K, ld, level_pix, N=2, seed=11, pow2=True)
    img = E.block_image(c)
    assert img(0, 256) == 0 and img(1, 0) == 0 and img(1, 254) == 0 and img(1, 255) == 1, "block 1: the last anchor of image 0 and 255 of image 1"
    loss, grad = E.focal_want(c)
    bad_loss, bad_grad = E.focal_want(c, image_of=img)
    assert abs(float(bad_loss) - float(loss)) > 1e-3 * abs(float(loss)), "the image index taken from the block changes the loss"
    assert float((bad_grad - grad).abs().max()) > 1e-3 * float(grad.abs().max())
    same_loss, same_grad = E.focal_want(c, image_of=lambda n, a: n)
    assert abs(float(same_loss) - float(loss)) <= 1e-12 * abs(float(loss)) and float((same_grad - grad).abs().max()) <= 1e-12
    for shape in E.FOCAL_SHAPES:                              # the cross-check's cases: powers of two at every shape
        for N in (2, 4):
            c = E.focal_case(*shape, N=N, seed=5, pow2=True)
            assert all(np.log2(d) == int(np.log2(d)) and d >= 2 for d in c["denom"])
            w = np.float32(1.0) / (np.float32(c["denom"][0]) * np.float32(N))
            assert np.float32(np.float32(1.0 / N) / np.float32(c["denom"][0])) == w, "both kernels scale by the same float"
