"""GPU tests of the SSM tail (cald_amd/csrc/ssm.hip: cald_op_ssm_postprocess, cald_sweep_ssm), of the stock small-box removal
(cald_model_set_box_min_size, cald_op_frcnn_postprocess_min) and of cald_amd/ssm.py end to end.  Bit for bit against
tests/_ssm_restatement.py unless a test says otherwise.  Constructed cases use integer boxes (zero deltas decode a proposal to itself,
integer class offsets keep the sums exact below 2^24), so an IoU p / q with q < 10^5 is either 3 / 10 itself or at least 1e-6 away from
it: each case asserts the margins it recorded."""
import ctypes as C
import random

import numpy as np
import pytest

import _ssm_restatement as R
from test_gpu_parity import small_retina      # noqa: F401  (the 300 / 500 RetinaNet of the parity tests)

F32 = np.float32
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc(oracle):
    R.check_exp(oracle)
    return oracle


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


def gpu_ssm(hip, logits, deltas, props, Hr, Wr, Ho, Wo, score_thr=0.05, det_max=100):
    ffi, L = hip["ffi"], hip["L"]
    logits = np.ascontiguousarray(logits, F32); deltas = np.ascontiguousarray(deltas, F32); props = np.ascontiguousarray(props, F32).reshape(-1, 4)
    Rn, Cn = logits.shape
    K, cap = Cn - 1, (Cn - 1) * det_max
    boxes = np.full((cap, 4), np.nan, F32); scores = np.full((cap, K), np.nan, F32); labels = np.full((cap, K), 99, np.int8)
    al, n = C.c_int(-1), C.c_int(-1)
    ffi.check(L.cald_op_ssm_postprocess(hip["ctx"], Rn, Cn, ffi.ptr(logits), ffi.ptr(deltas), ffi.ptr(props), Hr, Wr, Ho, Wo, score_thr, det_max,
                                        C.byref(al), C.byref(n), ffi.ptr(boxes), ffi.ptr(scores), ffi.ptr(labels, ffi.c_i8)))
    assert np.isnan(boxes[n.value:]).all() and np.isnan(scores[n.value:]).all() and (labels[n.value:] == 99).all()      # nothing past the count
    return dict(al=al.value, boxes=boxes[:n.value], scores=scores[:n.value], labels=labels[:n.value])


def assert_same(got, want, what):
    assert got["al"] == want["al"], what
    for k in ("boxes", "scores", "labels"):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def int_boxes(rs, n, Hr, Wr, lo=6, hi=90):
    x0 = rs.randint(0, Wr - hi, n); y0 = rs.randint(0, Hr - hi, n)
    return np.stack([x0, y0, x0 + rs.randint(lo, hi, n), y0 + rs.randint(lo, hi, n)], 1).astype(F32)


def random_case(seed, Rn, Cn, Hr, Wr, gain=3.0):
    rs = np.random.RandomState(seed)
    return R.integer_case(Rn, Cn, Hr, Wr, int_boxes(rs, Rn, Hr, Wr), (rs.randn(Rn, Cn - 1) * gain).astype(F32))


# (name, seed, R, C, Hr, Wr, Ho, Wo): one proposal; a handful; the full sort width (1 000 of the 1 024 keys); few and many classes
RANDOM_CASES = [("r1", 1, 1, 3, 200, 300, 200, 300), ("r5_c21", 2, 5, 21, 200, 300, 375, 563), ("r1000_c21", 3, 1000, 21, 600, 800, 333, 444),
                ("r200_c3", 4, 200, 3, 300, 500, 480, 800), ("r65_c21", 5, 65, 21, 300, 400, 300, 400)]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_ssm_tail_on_integer_boxes(hip, orc, case):
    name, seed, Rn, Cn, Hr, Wr, Ho, Wo = case
    logits, deltas, props = random_case(seed, Rn, Cn, Hr, Wr)
    if Rn == 1:
        logits[0, 1] = 4.0                                  # a confident class, so the one proposal is not an al = 1 view
    margins = {}
    want = R.ssm_tail(orc, logits, deltas, props, Hr, Wr, Ho, Wo, margins=margins)
    print(name, "rows", len(want["prop"]), "margins", margins)
    assert want["al"] == 0 and len(want["prop"]) > 0
    assert margins["thr"] > 1e-6 and margins["half"] > 1e-6          # a float32 rounding error at these values is 4e-9 / 3e-8
    assert margins["iou"] == 0.0 or margins["iou"] > 1e-6            # 3 / 10 itself rounds to the threshold's own float: not above it, exactly
    assert_same(gpu_ssm(hip, logits, deltas, props, Hr, Wr, Ho, Wo), want, name)


def test_cut_at_100_kept_boxes_of_a_class(hip, orc):
    """150 mutually disjoint boxes of class 1, all above 0.05: the class gives its first 100 by score; class 2 stays under 0.05."""
    ys, xs = np.divmod(np.arange(150), 15)
    boxes = np.stack([xs * 20, ys * 20, xs * 20 + 10, ys * 20 + 10], 1).astype(F32)
    cls_logit = np.stack([2.0 + rs_perm(150) * 0.01, np.full(150, -5.0)], 1).astype(F32)
    logits, deltas, props = R.integer_case(150, 3, 220, 320, boxes, cls_logit)
    want = R.ssm_tail(orc, logits, deltas, props, 220, 320, 220, 320)
    assert len(want["prop"]) == 100 and (want["cls"] == 1).all()
    assert sorted(want["prop"].tolist()) == sorted(np.argsort(-cls_logit[:, 0], kind="stable")[:100].tolist())
    assert (want["scores"][:, 0] > 0.05).all() and (want["scores"][:, 1] < 0.05).all()
    assert_same(gpu_ssm(hip, logits, deltas, props, 220, 320, 220, 320), want, "cut at 100")
    # a smaller cap cuts earlier, and the 150 fit under a larger one
    for det_max, n in ((7, 7), (64, 64), (65, 65), (200, 150)):
        w = R.ssm_tail(orc, logits, deltas, props, 220, 320, 220, 320, det_max=det_max)
        assert len(w["prop"]) == n
        assert_same(gpu_ssm(hip, logits, deltas, props, 220, 320, 220, 320, det_max=det_max), w, "cap %d" % det_max)


def rs_perm(n):
    return np.random.RandomState(n).permutation(n).astype(np.float64)


def test_a_class_without_rows_in_the_middle(hip, orc):
    """Class 2 of 3 foreground classes is wholly <= 0.05: the rows of class 3 follow those of class 1 directly."""
    rs = np.random.RandomState(8)
    boxes = int_boxes(rs, 30, 200, 300)
    cls_logit = np.stack([2.0 + rs.rand(30), np.full(30, -6.0), 1.5 + rs.rand(30)], 1).astype(F32)
    logits, deltas, props = R.integer_case(30, 4, 200, 300, boxes, cls_logit)
    want = R.ssm_tail(orc, logits, deltas, props, 200, 300, 200, 300)
    assert set(want["cls"].tolist()) == {1, 3}
    assert_same(gpu_ssm(hip, logits, deltas, props, 200, 300, 200, 300), want, "empty class in the middle")


def test_exact_score_ties_go_to_the_lower_index(hip, orc):
    """Every proposal has the same logits; proposals 2 i and 2 i + 1 overlap far above 0.3: the even one survives."""
    i = np.arange(20)
    even = np.stack([(i % 5) * 50, (i // 5) * 45, (i % 5) * 50 + 30, (i // 5) * 45 + 30], 1)
    boxes = np.empty((40, 4), F32); boxes[0::2] = even; boxes[1::2] = even + np.array([1, 0, 1, 0])
    logits, deltas, props = R.integer_case(40, 3, 200, 300, boxes, np.tile(np.array([1.5, 0.5], F32), (40, 1)))
    want = R.ssm_tail(orc, logits, deltas, props, 200, 300, 200, 300)
    assert want["prop"].tolist() == list(range(0, 40, 2)) * 2
    assert_same(gpu_ssm(hip, logits, deltas, props, 200, 300, 200, 300), want, "ties")


# two class-20 boxes found by search (random boxes whose raw IoU is within 1e-5 of 0.3): whether the first suppresses the second depends on the
# rounding of the coordinates + offset, so on the offset itself
PAIR_A = [7.710205554962158, 6.412424087524414, 17.710205078125, 16.412424087524414]
PAIR_B = [13.09480094909668, 6.412424087524414, 23.09480094909668, 16.412424087524414]


def test_the_class_offset_uses_the_maximum_of_the_class(hip, orc):
    """A pair of class-20 boxes that overlap above 0.3 without an offset, and with the offset 20 * (max over ALL classes + 1) -- class 1's
    boxes are widened by its deltas and reach further --, but not with 20 * (max over class 20's boxes + 1): both are kept."""
    Cn, c = 21, 20
    props = np.array([PAIR_A, PAIR_B, [100, 50, 250.5, 180.25]], F32)
    logits = np.full((3, Cn), -5.0, F32); logits[:, 0] = 0; logits[:, c] = [3.0, 2.0, 1.0]
    deltas = np.zeros((3, 4 * Cn), F32); deltas[:, 4 * 1 + 2] = 2.0; deltas[:, 4 * 1 + 3] = 2.0
    prob, cbox = R.rows(orc, logits, deltas, props, 200, 300)
    own, everyone = cbox[:, c - 1].max(), cbox.max()
    assert everyone > own
    pair = cbox[:2, c - 1]
    assert R.pair_iou(pair, 0.0) > F32(0.3) and R.pair_iou(pair, F32(c) * F32(everyone + F32(1))) > F32(0.3)
    assert not R.pair_iou(pair, F32(c) * F32(own + F32(1))) > F32(0.3)
    want = R.ssm_tail(orc, logits, deltas, props, 200, 300, 200, 300)
    assert want["prop"].tolist() == [0, 1, 2] and want["cls"].tolist() == [c] * 3
    assert_same(gpu_ssm(hip, logits, deltas, props, 200, 300, 200, 300), want, "class offset")


def boundary_case(best_bg):
    """Three proposals; the best row's logits are {background: best_bg, class 2: 0, the rest: -200}: exp(0) = 1 and exp(-200) = 0 exactly."""
    logits = np.full((3, 4), -200.0, F32)
    logits[:, 0] = 5.0; logits[:, 1] = 0.0                       # rows 0 and 2: foreground far below 0.05
    logits[1] = [best_bg, -200.0, 0.0, -200.0]
    boxes = np.array([[10, 10, 60, 60], [100, 20, 180, 90], [30, 100, 90, 170]], F32)
    return logits, np.zeros((3, 16), F32), boxes


def test_al_boundary_at_exactly_one_half(hip, orc):
    logits, deltas, props = boundary_case(0.0)
    prob, _ = R.rows(orc, logits, deltas, props, 200, 300)
    assert prob[:, 1:].max() == F32(0.5) and prob[1, 2] == F32(0.5)
    want = R.ssm_tail(orc, logits, deltas, props, 200, 300, 200, 300)
    assert want["al"] == 0 and want["prop"].tolist() == [1] and want["cls"].tolist() == [2] and (want["labels"] == -1).all()
    assert_same(gpu_ssm(hip, logits, deltas, props, 200, 300, 200, 300), want, "al at 0.5")


def test_al_boundary_one_ulp_below_one_half(hip, orc):
    """A background logit of 2^-24 makes the class's exponential 1 - 2^-24 and the sum round to 2: the largest probability is the float
    just below 0.5, al = 1 and there are no rows."""
    logits, deltas, props = boundary_case(2.0 ** -24)
    prob, _ = R.rows(orc, logits, deltas, props, 200, 300)
    assert prob[:, 1:].max() == np.nextafter(F32(0.5), F32(0))
    want = R.ssm_tail(orc, logits, deltas, props, 200, 300, 200, 300)
    assert want["al"] == 1 and len(want["prop"]) == 0
    assert_same(gpu_ssm(hip, logits, deltas, props, 200, 300, 200, 300), want, "al one ulp below 0.5")


def test_no_proposals_is_an_al_view(hip, orc):
    got = gpu_ssm(hip, np.zeros((0, 21), F32), np.zeros((0, 84), F32), np.zeros((0, 4), F32), 200, 300, 200, 300)
    assert got["al"] == 1 and got["boxes"].shape == (0, 4)


def test_hook_rejects_bad_arguments(hip):
    ffi, L = hip["ffi"], hip["L"]
    a = np.zeros((1, 105), F32); out = np.zeros(4000, F32); lab = np.zeros(4000, np.int8); al, n = C.c_int(), C.c_int()
    args = lambda Rn, Cn, det: (hip["ctx"], Rn, Cn, ffi.ptr(a), ffi.ptr(a), ffi.ptr(a), 10, 10, 10, 10, 0.05, det, C.byref(al), C.byref(n), ffi.ptr(out),
                                ffi.ptr(out), ffi.ptr(lab, ffi.c_i8))
    assert L.cald_op_ssm_postprocess(*args(1001, 21, 100)) == -1 and L.cald_op_ssm_postprocess(*args(1, 1, 100)) == -1
    assert L.cald_op_ssm_postprocess(*args(1, 21, 513)) == -1
    assert L.cald_op_ssm_postprocess(hip["ctx"], 1, 21, None, ffi.ptr(a), ffi.ptr(a), 10, 10, 10, 10, 0.05, 100, C.byref(al), C.byref(n), ffi.ptr(out),
                                     ffi.ptr(out), ffi.ptr(lab, ffi.c_i8)) == -1


def test_hook_matches_the_executed_reference_tail(hip, golden):
    """The fixture's cases (the reference's own ssm_postprocess_detections, torch's exp): al, counts and labels exactly, probabilities to
    1e-5 and boxes to 1e-3 -- the tolerances of test_frcnn_postprocess_kernels_match_the_reference_method_body."""
    fx = golden("ssm")
    for k in range(int(fx["t_n"])):
        H, W = [int(v) for v in fx["t%d_hw" % k]]
        got = gpu_ssm(hip, fx["t%d_logits" % k], fx["t%d_deltas" % k], fx["t%d_props" % k], H, W, H, W)
        assert got["al"] == int(fx["t%d_al" % k]) and got["boxes"].shape == fx["t%d_boxes" % k].shape
        assert np.array_equal(got["labels"], fx["t%d_labels" % k])
        assert np.abs(got["scores"] - fx["t%d_scores" % k]).max(initial=0.0) <= 1e-5
        assert np.abs(got["boxes"] - fx["t%d_boxes" % k]).max(initial=0.0) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the stock small-box removal of the ordinary tail
# ---------------------------------------------------------------------------------------------------------------------------
def gpu_frcnn_min(hip, logits, deltas, props, Hr, Wr, Ho, Wo, min_size, det_max=100, score_thr=0.05, nms_thr=0.5, plain=False):
    ffi, L = hip["ffi"], hip["L"]
    logits = np.ascontiguousarray(logits, F32); deltas = np.ascontiguousarray(deltas, F32); props = np.ascontiguousarray(props, F32).reshape(-1, 4)
    Rn, Cn = logits.shape
    ob = np.empty((det_max, 4), F32); os_ = np.empty(det_max, F32); ol = np.empty(det_max, np.int64)
    op = np.empty((det_max, 4), F32); opm = np.empty(det_max, F32); osc = np.empty((det_max, Cn), F32); n = C.c_int(0)
    head = (hip["ctx"], Rn, Cn, ffi.ptr(logits), ffi.ptr(deltas), ffi.ptr(props), Hr, Wr, Ho, Wo, score_thr, nms_thr, det_max)
    tail = (ffi.ptr(ob), ffi.ptr(os_), ffi.ptr(ol, ffi.c_i64), ffi.ptr(op), ffi.ptr(opm), ffi.ptr(osc), C.byref(n))
    ffi.check(L.cald_op_frcnn_postprocess(*head, *tail) if plain else L.cald_op_frcnn_postprocess_min(*head, min_size, *tail))
    k = n.value
    return dict(boxes=ob[:k], scores=os_[:k], labels=ol[:k], props=op[:k], prob_max=opm[:k], scores_cls=osc[:k])


def test_box_min_size_zero_is_the_tail_as_it_was(hip, orc, golden):
    g = golden("postprocess")
    for k in range(int(g["f_n"])):
        H, W = [int(v) for v in g["f%d_hw" % k]]
        a = (g["f%d_logits" % k], g["f%d_deltas" % k], g["f%d_props" % k], H, W, H, W)
        want = orc.frcnn_postprocess(*a)
        for got in (gpu_frcnn_min(hip, *a, 0.0), gpu_frcnn_min(hip, *a, 0.0, plain=True)):
            for key in want:
                assert got[key].tobytes() == want[key].tobytes(), (k, key)
        small = R.frcnn_tail_min(orc, *a, min_size=0.0)
        for key in want:
            assert small[key].tobytes() == want[key].tobytes(), ("restatement", k, key)


def test_box_min_size_drops_degenerate_boxes_before_the_offset(hip, orc):
    """Class-20 candidates: the pair above, a far box holding the largest proper coordinate (250.5), a zero-width box further right
    (251.0137: counted into the maximum, its offset makes the pair overlap above 0.3 -- measured below) and a zero-width box with the best
    score.  Without the removal both degenerate boxes are detections and the pair's second box is suppressed; with min_size 1e-2 they
    are gone, the maximum is 250.5 and the pair survives."""
    Cn, c = 21, 20
    props = np.array([PAIR_A, PAIR_B, [100, 50, 250.5, 180.25], [251.01370239257812, 10, 251.01370239257812, 50], [30, 30, 30, 60]], F32)
    logits = np.full((5, Cn), -5.0, F32); logits[:, 0] = 0; logits[:, c] = [3.0, 2.0, 1.0, 1.5, 4.0]
    deltas = np.zeros((5, 4 * Cn), F32)
    a = (logits, deltas, props, 200, 300, 200, 300)
    _, cbox = R.rows(orc, *a[:5])
    pair = cbox[:2, c - 1]
    assert cbox[3, c - 1, 0] == cbox[3, c - 1, 2] == F32(251.01370239257812) and cbox[:, c - 1].max() == cbox[3, c - 1, 0]
    assert R.pair_iou(pair, F32(c) * F32(cbox[3, c - 1, 0] + F32(1))) > F32(0.3) and not R.pair_iou(pair, F32(c) * F32(F32(250.5) + F32(1))) > F32(0.3)
    off = orc.frcnn_postprocess(*a, nms_thr=0.3)
    on = R.frcnn_tail_min(orc, *a, nms_thr=0.3, min_size=1e-2)
    assert len(off["labels"]) == 4 and len(on["labels"]) == 3                 # [best degenerate, A, far, degenerate] against [A, B, far]
    got_off = gpu_frcnn_min(hip, *a, 0.0, nms_thr=0.3); got_on = gpu_frcnn_min(hip, *a, 1e-2, nms_thr=0.3)
    for key in off:
        assert got_off[key].tobytes() == off[key].tobytes(), ("off", key)
        assert got_on[key].tobytes() == on[key].tobytes(), ("on", key)


# ---------------------------------------------------------------------------------------------------------------------------
# the forward: cald_sweep_ssm on the small model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ssm_model(hip, orc):
    """The 300 / 500 ResNet-50 with synth.pseudo_trained_frcnn's weights, three images of different sizes, and per image the proposal
    count of the oracle's forward (the library's forward equals it bit for bit: test_forward_stagewise_bit_exact)."""
    from cald_amd import ssm, synth
    torch = hip["torch"]
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    model = ssm.fasterrcnn_resnet50_fpn_ssm(num_classes=21, min_size=300, max_size=500)
    model.to("cuda").load_state_dict(sd)
    model.eval()
    pool = synth.make_pool(3, "voc", 0, scale=0.5)
    imgs = [pool[0], pool[1], np.ascontiguousarray(pool[2][:200, :150])]
    assert len({im.shape for im in imgs}) == 3
    P = orc.prepare_frcnn(sd, 21, 50)
    counts = []
    for im in imgs:
        keep = {}
        orc.frcnn_forward(P, im, 300, 500, keep=keep)
        counts.append(keep["proposals"].shape[0])
    return model, imgs, [torch.from_numpy(im).cuda() for im in imgs], counts


def _sweep(ssm, model, dev_imgs, batch):
    return ssm.ssm_sweep_device_images(model, dev_imgs, batch_images=batch)


def test_sweep_equals_the_hook_on_the_forwards_own_tensors(hip, orc, ssm_model):
    from cald_amd import ssm, train_ops
    model, imgs, dev, counts = ssm_model
    al, cnt, boxes, scores, labels = _sweep(ssm, model, dev, 3)
    off = np.concatenate([[0], np.cumsum(cnt)])
    assert (al == 0).any() and cnt.sum() > 0 and boxes.shape == (cnt.sum(), 4) and scores.shape == (cnt.sum(), 20) and labels.shape == (cnt.sum(), 20)
    for v, im in enumerate(imgs):                      # the debug tensors are those of the last forward: all three views in one batch
        n = counts[v]
        Hr, Wr, _, _ = train_ops.transform_size(im.shape[0], im.shape[1], 300, 500)
        pred = model.debug_tensor("pred", v).reshape(1000, 105)[:n]
        props = model.debug_tensor("proposals", v).reshape(-1, 4)[:n]
        want = gpu_ssm(hip, pred[:, :21], pred[:, 21:], props, Hr, Wr, im.shape[0], im.shape[1])
        got = dict(al=int(al[v]), boxes=boxes[off[v]:off[v + 1]], scores=scores[off[v]:off[v + 1]], labels=labels[off[v]:off[v + 1]])
        assert_same(got, want, "view %d against the hook" % v)
        assert_same(got, R.ssm_tail(orc, pred[:, :21], pred[:, 21:], props, Hr, Wr, im.shape[0], im.shape[1]), "view %d against the restatement" % v)


def test_sweep_does_not_depend_on_the_batch_and_repeats_its_bytes(hip, ssm_model):
    from cald_amd import ssm
    model, _, dev, _ = ssm_model
    runs = [_sweep(ssm, model, dev, 3), _sweep(ssm, model, dev, 3), _sweep(ssm, model, dev, 1), _sweep(ssm, model, dev, 2)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_sweep_reports_the_rows_it_needs(hip, ssm_model, small_retina):
    from cald_amd import ssm
    from cald_amd.baselines import _arrays
    ffi, L = hip["ffi"], hip["L"]
    model, _, dev, _ = ssm_model
    total = int(_sweep(ssm, model, dev, 3)[1].sum())
    ptrs, Hs, Ws = _arrays(dev)
    al = np.zeros(3, np.int32); cnt = np.zeros(3, np.int32)
    boxes = np.zeros((total, 4), F32); scores = np.zeros((total, 20), F32); labels = np.zeros((total, 20), np.int8); need = C.c_int64(-1)

    def call(handle, cap, al_ptr=None):
        return L.cald_sweep_ssm(handle, 3, ptrs, ffi.ptr(Hs, ffi.c_i), ffi.ptr(Ws, ffi.c_i), 2, cap, al_ptr if al_ptr is not None else ffi.ptr(al, ffi.c_i),
                                ffi.ptr(cnt, ffi.c_i), ffi.ptr(boxes), ffi.ptr(scores), ffi.ptr(labels, ffi.c_i8), C.byref(need))
    assert call(model.handle(), total - 1) == -1 and need.value == total
    assert ("needs %d rows" % total) in L.cald_last_error().decode() and int(cnt.sum()) == total
    need.value = -1
    assert call(model.handle(), total) == 0 and need.value == total
    assert L.cald_sweep_ssm(model.handle(), 3, ptrs, ffi.ptr(Hs, ffi.c_i), ffi.ptr(Ws, ffi.c_i), 2, total, None, ffi.ptr(cnt, ffi.c_i), ffi.ptr(boxes),
                            ffi.ptr(scores), ffi.ptr(labels, ffi.c_i8), C.byref(need)) == -1                       # a null argument
    assert call(small_retina[0].handle(), total) == -1                                                             # a RetinaNet handle


# ---------------------------------------------------------------------------------------------------------------------------
# cald_amd/ssm.py end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_get_uncertainty_returns_the_references_types(hip, ssm_model):
    from cald_amd import ssm
    torch = hip["torch"]
    model, imgs, dev, _ = ssm_model
    loader = [([torch.from_numpy(im).permute(2, 0, 1).float().div(255)], [{}]) for im in imgs]       # to_tensor's float CHW, one image an item
    allScore, allBox, allY, al_idx = ssm.get_uncertainty(model, loader)
    al, cnt, boxes, scores, labels = _sweep(ssm, model, dev, 3)
    kept = [i for i in range(3) if al[i] == 0]
    assert al_idx == [i for i in range(3) if al[i] == 1] and len(allScore) == len(allBox) == len(allY) == len(kept) > 0
    off = np.concatenate([[0], np.cumsum(cnt)])
    for j, i in enumerate(kept):
        assert allScore[j].is_cuda and allScore[j].dtype == torch.float32 and tuple(allScore[j].shape) == (cnt[i], 20)
        assert allBox[j].is_cuda and tuple(allBox[j].shape) == (cnt[i], 4)
        assert isinstance(allY[j], list) and len(allY[j]) == cnt[i] and all(isinstance(y, list) and len(y) == 20 and set(y) <= {1, -1} for y in allY[j])
        assert allScore[j].cpu().numpy().tobytes() == scores[off[i]:off[i + 1]].tobytes() and allBox[j].cpu().numpy().tobytes() == boxes[off[i]:off[i + 1]].tobytes()
        assert np.array_equal(np.array(allY[j], np.int8), labels[off[i]:off[i + 1]])
    det = model([loader[kept[0]][0][0]])[0]                      # ssm_mode(True) is still on: the reference's dict
    assert set(det) == {"boxes", "scores", "labels", "al"} and det["al"] == 0 and torch.equal(det["scores"], allScore[0])
    with pytest.raises(ValueError):
        ssm.get_uncertainty(model, [([loader[0][0][0], loader[1][0][0]], [{}, {}])])


class _Recording:
    """The detector, with every batch it is handed kept."""

    def __init__(self, model):
        self.model, self.batches, self.results = model, [], []

    def eval(self):
        return self.model.eval()

    def ssm_mode(self, flag):
        self.model.ssm_mode(flag)

    def __call__(self, images):
        self.batches.append([im.clone() for im in images])
        out = self.model(images)
        self.results.append(out)
        return out


def test_image_cross_validation_end_to_end_on_two_candidates(hip, ssm_model):
    from cald_amd import ssm
    torch = hip["torch"]
    model, imgs, dev, _ = ssm_model
    allScore, allBox, _, _ = ssm.get_uncertainty(model, [([dev[0]], [{}])])
    def crop(b):
        return dev[0][int(b[0]):int(b[2]), int(b[1]):int(b[3])]
    fits = [b for b in allBox[0] if 0 < crop(b).shape[0] <= 187 and 0 < crop(b).shape[1] <= 150]       # a patch both labeled images can take
    box = fits[0] if fits else torch.tensor([12.6, 20.2, 70.9, 95.5])
    patch = crop(box)
    before = [d.clone() for d in dev]
    rec = _Recording(model)
    labeled = [([dev[1]], [{"labels": torch.tensor([1, 2])}]), ([dev[2]], [{"labels": torch.tensor([4])}])]
    random.seed(77)
    flag, score = ssm.image_cross_validation(rec, [([dev[0]], [{}])], labeled, box, torch.tensor([3]))
    assert isinstance(flag, bool) and flag is False and score == 0          # two images can never give more than 2.5 confirmations
    assert len(rec.batches) == 1 and len(rec.batches[0]) == 2 and model._ssm is False
    for res in rec.results[0]:                                              # the stock dict of ssm_mode(False)
        assert {"boxes", "labels", "scores"} <= set(res) and res["labels"].dtype == torch.int64
    random.seed(77)
    for k in (1, 2):                                                        # the pasted pixels, on the uint8 tensors the detector saw
        H, W = dev[k].shape[:2]
        sy = random.randint(0, H - patch.shape[0]); sx = random.randint(0, W - patch.shape[1])
        want = before[k].clone(); want[sy:sy + patch.shape[0], sx:sx + patch.shape[1]] = patch
        got = rec.batches[0][k - 1]
        assert got.dtype == torch.uint8 and torch.equal(got, want) and not torch.equal(got, before[k])
    for d, b in zip(dev, before):                                           # the resident images are as they were
        assert torch.equal(d, b)
