"""The detection tail at its capacity paths and gear changes: RetinaNet post-processing (retina.hip, through cald_op_retina_postprocess),
Faster R-CNN post-processing (roi.hip), the RPN's top-k / NMS / merge (rpn.hip), block_nms_sorted (sortnms.h) and the chunked scoring
loop (score.hip).

Method.  Every input is built so that each decision is exact in any precision: boxes are integers with areas below 2^24, deltas are
zero, scores are either exactly tied or far apart.  An IoU is then the correctly rounded quotient of two exact integers on the float32
side and the exact rational in tests/_tail_restatement.py (plain numpy float64, decisions only).  The condition, asserted by the CPU
half of every case: each pairwise IoU an NMS meets equals the threshold as a rational (1/2, 7/10 -- wanted, they pin `>` against `>=`)
or is at least 1e-4 away from it.  The comparison is then of index sets, not of floats within a tolerance:

  GPU vs oracle          tobytes()-equal on every output;
  GPU vs restatement     kept indices, labels and order equal;
  floats vs float64      1e-5 (scores), 1e-3 (boxes) -- the bounds of test_gpu_parity.py.

The CPU half (restatement vs oracle) runs without a GPU.  This file uses train_ops entry points, hence its name sorts behind
test_gpu_parity.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _tail_restatement as R

F32 = np.float32
MARGIN = 1e-4
SEED = 4000          # of the random score orders; a seed under which some case breaks the condition on the IoUs is replaced


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


def _assert_bytes(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


# ---------------------------------------------------------------------------------------------------------------------------
# RetinaNet post-processing
# ---------------------------------------------------------------------------------------------------------------------------
def _retina_base(orc):
    return np.stack([orc.base_anchors(list(s), [0.5, 1.0, 2.0]) for s in orc.retina_anchor_sizes()])      # [5][9][4]


def _retina_levels(Hp, Wp):
    hw = [(Hp // 8, Wp // 8), (Hp // 16, Wp // 16), (Hp // 32, Wp // 32)]
    for _ in range(2):
        hw.append(((hw[-1][0] - 1) // 2 + 1, (hw[-1][1] - 1) // 2 + 1))
    return hw


def _retina_reference(orc, case):
    """oracle output + restatement indices of one case (zero deltas)."""
    cls, base, K, A = case["cls"], case["base"], case["K"], case["A"]
    Hp, Wp, Hr, Wr = case["sizes"]
    Ho, Wo = case["orig"]
    reg = [np.zeros(c.shape[:2] + (A * 4,), F32) for c in cls]
    want = orc.retina_postprocess(cls, reg, base, Hp, Wp, Hr, Wr, Ho, Wo, K, A, 0.05, 0.5, case["per_class"])
    anchors = np.concatenate([R.grid_anchors(base[l], c.shape[0], c.shape[1], Hp // c.shape[0], Wp // c.shape[1]) for l, c in enumerate(cls)])
    boxes = R.clip(anchors, Hr, Wr)
    logits = np.concatenate([c.reshape(-1, K) for c in cls]).astype(np.float64)
    scores = 1.0 / (1.0 + np.exp(-logits))
    idx, margin, ncand = R.retina(scores, boxes, 0.05, 0.5, case["per_class"], float(F32(1e-2)))
    scale = np.array([Wo / Wr, Ho / Hr, Wo / Wr, Ho / Hr])
    return dict(want=want, reg=reg, idx=idx, margin=margin, ncand=ncand, boxes=boxes[idx[:, 0]] * scale, scores=scores[idx[:, 0]])


@functools.lru_cache(maxsize=None)
def _retina_flat_case(orc):
    """Hp = Wp = 256: 12 276 anchors, K = 2, every logit 0: every class has 12 276 > 8192 candidates (keys sorted in global memory), all
    tied, so the index half of the key decides the whole order."""
    hw = _retina_levels(256, 256)
    case = dict(cls=[np.zeros((h, w, 9 * 2), F32) for h, w in hw], base=_retina_base(orc), K=2, A=9, sizes=(256, 256, 240, 250), orig=(480, 1000),
                per_class=300)
    case.update(_retina_reference(orc, case))
    return case


def _rank_logits(rank):
    """distinct, well separated scores: logit 3.5 - rank / 2048 (sigmoid steps >= 1e-5, lowest score 0.076)"""
    return (3.5 - rank / 2048.0).astype(F32)


@functools.lru_cache(maxsize=None)
def _retina_k4_case(orc, per_class):
    """K = 4 on the same pyramid, resized image 176 x 176: class 0 has no candidate, class 1 exactly per_class survivors of the NMS, class 2
    per_class + 1 (the cut), class 3 only anchors that the clip leaves without width (candidates, all removed as small boxes).  Classes 1
    and 2 also hold such anchors among their best scores."""
    hw = _retina_levels(256, 256)
    base = _retina_base(orc)
    Hr = Wr = 176
    anchors = np.concatenate([R.grid_anchors(base[l], h, w, 256 // h, 256 // w) for l, (h, w) in enumerate(hw)])
    boxes = R.clip(anchors, Hr, Wr)
    n = boxes.shape[0]
    ok = R.not_small(boxes, 1e-2)
    rs = np.random.RandomState(SEED + per_class)
    logits = np.full((n, 4), -10.0, F32)
    survivors = {}
    gone = np.nonzero(~ok)[0]
    assert gone.size >= 64
    for k in (1, 2):
        rank = rs.permutation(n)
        g = gone[rs.randint(gone.size)]                       # the best score of the class belongs to an anchor without width
        rank[rank == 0], rank[g] = rank[g], 0
        order = np.argsort(rank)                              # anchors in score order
        valid = order[ok[order]]
        keep, _ = R.nms(boxes[valid], 0.5)
        want = per_class + (k - 1)
        assert keep.size > want, "the pool has too few survivors for this per_class"
        last = valid[keep[want - 1]]                          # candidates: everything down to the want-th survivor
        cand = order[:rank[last] + 1]
        logits[cand, k] = _rank_logits(rank[cand])
        survivors[k] = want
        assert (~ok[cand]).sum() > 0
    logits[gone, 3] = _rank_logits(rs.permutation(gone.size))
    cls, off = [], 0
    for h, w in hw:
        cls.append(np.ascontiguousarray(logits[off:off + h * w * 9].reshape(h, w, 36))); off += h * w * 9
    case = dict(cls=cls, base=base, K=4, A=9, sizes=(256, 256, Hr, Wr), orig=(Hr, Wr), per_class=per_class, survivors=survivors)
    case.update(_retina_reference(orc, case))
    return case


@functools.lru_cache(maxsize=None)
def _retina_min_box_case(orc):
    """remove_small_boxes keeps a side of EXACTLY min_size (>=): one anchor float32(1e-2) wide, one a float32 step narrower.  A = K = 1;
    only pixel (0, 0) of a level is a candidate, where the anchor shift is zero and the decoded box is the base anchor itself."""
    hw = _retina_levels(64, 64)
    mb = F32(1e-2)
    base = np.zeros((5, 1, 4), F32)
    base[0, 0] = [0, 0, mb, 16]; base[1, 0] = [0, 0, np.nextafter(mb, F32(0)), 16]; base[2, 0] = [0, 0, 16, mb]
    base[3, 0] = [0, 0, 16, np.nextafter(mb, F32(0))]; base[4, 0] = [0, 0, 16, 16]
    cls = [np.full((h, w, 1), -10.0, F32) for h, w in hw]
    for l in range(5):
        cls[l][0, 0, 0] = 2.0 - 0.25 * l
    case = dict(cls=cls, base=base, K=1, A=1, sizes=(64, 64, 64, 64), orig=(64, 64), per_class=300)
    case.update(_retina_reference(orc, case))
    return case


@functools.lru_cache(maxsize=None)
def _retina_designed_case(orc):
    """four anchors per pixel, all 16 wide, heights 16 (a0), 8 (a1), 10 (a2), 6 (a3), one corner shared: IoU = h_small / h_large.  Pixel P
    holds the chain a0 > a2 > a3 in score order: a0 drops a2 (5/8), a2 would drop a3 (3/5) but is dead, a0 does not (3/8): a3 stays.
    Pixel Q holds a0 and a1 at IoU exactly 1/2: both stay."""
    hw = _retina_levels(64, 64)
    base = np.tile(np.array([[-8, -8, 8, 8], [-8, -8, 8, 0], [-8, -8, 8, 2], [-8, -8, 8, -2]], F32), (5, 1, 1))
    cls = [np.full((h, w, 4), -10.0, F32) for h, w in hw]
    cls[0][2, 2, [0, 2, 3]] = [3.0, 2.5, 2.0]
    cls[0][2, 5, [0, 1]] = [1.5, 1.0]
    case = dict(cls=cls, base=base, K=1, A=4, sizes=(64, 64, 64, 64), orig=(64, 64), per_class=300)
    case.update(_retina_reference(orc, case))
    return case


RETINA_CASES = {"flat_global_keys": _retina_flat_case, "min_box": _retina_min_box_case, "designed": _retina_designed_case}
for _p in (1, 64, 65, 300):
    RETINA_CASES["k4_per%d" % _p] = functools.partial(_retina_k4_case, per_class=_p)


def _check_retina_reference(name, case):
    want, idx = case["want"], case["idx"]
    assert case["margin"] >= MARGIN, (name, case["margin"])
    assert len(want["labels"]) == len(idx), (name, len(want["labels"]), len(idx))
    np.testing.assert_array_equal(want["labels"], idx[:, 1])
    np.testing.assert_array_equal(want["boxes"], case["boxes"].astype(F32))
    np.testing.assert_allclose(want["scores_cls"], case["scores"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(want["scores"], case["scores"][np.arange(len(idx)), idx[:, 1]], rtol=0, atol=1e-5)
    np.testing.assert_allclose(want["prob_max"], case["scores"].max(1) if len(idx) else np.zeros(0), rtol=0, atol=1e-5)
    per_cls = np.bincount(idx[:, 1], minlength=case["K"])
    if name == "flat_global_keys":
        assert case["ncand"] == [12276, 12276] and min(case["ncand"]) > 8192            # the global-key branch of retina_class_nms_kernel
        assert list(per_cls) == [300, 300]
    elif name == "designed":
        np.testing.assert_array_equal(idx[:, 0], [18 * 4, 18 * 4 + 3, 21 * 4, 21 * 4 + 1])
    elif name == "min_box":
        np.testing.assert_array_equal(idx[:, 0], [0, 64 + 16, 64 + 16 + 4 + 1])          # levels 0, 2 and 4 stay; 1 and 3 are a step too narrow
    else:
        p = case["per_class"]
        assert case["ncand"][0] == 0 and list(per_cls) == [0, p, p, 0] and case["ncand"][3] >= 64
        assert case["survivors"] == {1: p, 2: p + 1}


@pytest.mark.parametrize("name", sorted(RETINA_CASES))
def test_retina_restatement_equals_oracle(orc, name):
    case = RETINA_CASES[name](orc)
    print("retina %s: candidates per class %s, detections %d, min |IoU - 1/2| %.6g" % (name, case["ncand"], len(case["idx"]), case["margin"]))
    _check_retina_reference(name, case)


def gpu_retina(hip, cls, reg, base, K, A, sizes, orig, per_class, score_thr=0.05, nms_thr=0.5):
    ffi, L = hip["ffi"], hip["L"]
    cls = [np.ascontiguousarray(c, F32) for c in cls]; reg = [np.ascontiguousarray(r, F32) for r in reg]
    base = np.ascontiguousarray(base, F32)
    hw = np.array([v for c in cls for v in c.shape[:2]], np.int32)
    cp = (ffi.c_f * 5)(*[ffi.ptr(c) for c in cls]); rp = (ffi.c_f * 5)(*[ffi.ptr(r) for r in reg])
    cap = K * per_class
    ob = np.empty((cap, 4), F32); osc = np.empty(cap, F32); ol = np.empty(cap, np.int64); opm = np.empty(cap, F32); ocl = np.empty((cap, K), F32)
    n = C.c_int(-1)
    Hp, Wp, Hr, Wr = sizes
    ffi.check(L.cald_op_retina_postprocess(hip["ctx"], cp, rp, ffi.ptr(hw, ffi.c_i), A, K, ffi.ptr(base), Hp, Wp, Hr, Wr, orig[0], orig[1],
                                           score_thr, nms_thr, per_class, ffi.ptr(ob), ffi.ptr(osc), ffi.ptr(ol, ffi.c_i64), ffi.ptr(opm),
                                           ffi.ptr(ocl), C.byref(n)))
    m = n.value
    assert 0 <= m <= cap
    return dict(boxes=ob[:m].copy(), scores=osc[:m].copy(), labels=ol[:m].copy(), prob_max=opm[:m].copy(), scores_cls=ocl[:m].copy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RETINA_CASES))
def test_retina_kernels_on_constructed_cases(hip, orc, name):
    """retina_cand_kernel / retina_class_nms_kernel / retina_emit_kernel: bytes vs the oracle, indices vs the float64 restatement."""
    case = RETINA_CASES[name](orc)
    got = gpu_retina(hip, case["cls"], case["reg"], case["base"], case["K"], case["A"], case["sizes"], case["orig"], case["per_class"])
    idx = case["idx"]
    assert len(got["labels"]) == len(idx), (name, len(got["labels"]), len(idx))
    np.testing.assert_array_equal(got["labels"], idx[:, 1])
    np.testing.assert_array_equal(got["boxes"], case["boxes"].astype(F32))
    np.testing.assert_allclose(got["scores_cls"], case["scores"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(got["scores"], case["scores"][np.arange(len(idx)), idx[:, 1]], rtol=0, atol=1e-5)
    _assert_bytes(got, case["want"], name)


@pytest.mark.gpu
def test_retina_kernels_match_the_reference_method_body(hip, orc, golden):
    """A22 on the GPU: the three golden cases recorded from the reference's own postprocess_detections (retinanet_cal.py:402-490,
    tests/golden/postprocess.npz) straight onto the kernels: count and labels exactly, floats to 1e-5 / 1e-3, bytes vs the oracle."""
    g = golden("postprocess")
    base = g["r_base"]
    assert int(g["r_n"]) == 3
    for k in range(3):
        K = int(g["r%d_K" % k]); Hp, Wp, Hr, Wr = [int(v) for v in g["r%d_sizes" % k]]
        cls = [g["r%d_cls%d" % (k, l)] for l in range(5)]; reg = [g["r%d_reg%d" % (k, l)] for l in range(5)]
        got = gpu_retina(hip, cls, reg, base, K, 9, (Hp, Wp, Hr, Wr), (Hr, Wr), 300)
        want = {n: g["r%d_out_%s" % (k, n)] for n in ("boxes", "scores", "labels", "scores_cls", "prob_max")}
        assert got["labels"].shape == want["labels"].shape, (k, got["labels"].shape, want["labels"].shape)
        np.testing.assert_array_equal(got["labels"], want["labels"])
        for n in ("scores", "prob_max", "scores_cls"):
            np.testing.assert_allclose(got[n], want[n].reshape(got[n].shape), rtol=0, atol=1e-5)
        np.testing.assert_allclose(got["boxes"], want["boxes"], rtol=0, atol=1e-3)
        _assert_bytes(got, orc.retina_postprocess(cls, reg, base, Hp, Wp, Hr, Wr, Hr, Wr, K), "r%d" % k)


# ---------------------------------------------------------------------------------------------------------------------------
# Faster R-CNN post-processing: more than 8192 candidates (keys sorted in global memory), the first-n cut around a chunk of 64,
# chains inside a chunk and across chunks, a pair at IoU exactly 1/2, more kept boxes than waves before the first suppression
# ---------------------------------------------------------------------------------------------------------------------------
FR_R, FR_C, FR_FLAT = 1000, 21, 10
FR_HW = (1024, 2048)
DET_MAX = [1, 63, 64, 65, 100, 512]


@functools.lru_cache(maxsize=None)
def _frcnn_inputs():
    """1000 proposals = 125 clusters of 8 nested boxes [x, y, x + 100, y + h] on a 128-pixel grid: IoU inside a cluster = h_small / h_large
    (exactly 1/2, or at least 1/200 away from it), 0 across clusters.  Ten foreground classes share one logit per proposal (exact ties
    between the classes of a proposal, scores of different proposals >= 1e-6 apart); 40 proposals stay below the score threshold."""
    rs = np.random.RandomState(7)
    boxes = np.zeros((FR_R, 4), np.float64)
    for c in range(125):
        x, y = 128 * (c % 16) + 8, 128 * (c // 16) + 8
        h = rs.choice(np.arange(20, 101), 8, replace=False)
        boxes[8 * c:8 * c + 8] = np.stack([np.full(8, x), np.full(8, y), np.full(8, x + 100), y + h], 1)
    # designed clusters: 0 = a chain A > B > C (A drops B, B would drop C, A does not), 1 = the same chain again, 2 = a pair at exactly 1/2
    boxes[0:3, 3] = boxes[0, 1] + np.array([100, 60, 35]); boxes[8:11, 3] = boxes[8, 1] + np.array([100, 60, 35])
    boxes[16:18, 3] = boxes[16, 1] + np.array([100, 50])
    for c in (0, 1, 2):                                     # the other members of the designed clusters: distinct heights again
        used = set(boxes[8 * c:8 * c + 3, 3] - boxes[8 * c, 1])
        free = [v for v in range(20, 100) if v not in used]
        boxes[8 * c + 3:8 * c + 8, 3] = boxes[8 * c, 1] + rs.choice(free, 5, replace=False)
    assert len({tuple(b) for b in boxes}) == FR_R
    # score rank per proposal: A, a far box, B, C at ranks 0..3 (inside the first chunk of 64 candidates = 6.4 proposals x 10 classes: 20 boxes
    # are kept before B is dropped); the second chain at ranks 5..7 (rank 6 straddles candidate 64); the 1/2 pair at ranks 8, 9
    rank = np.full(FR_R, -1)
    for r, p in zip([0, 1, 2, 3, 5, 6, 7, 8, 9], [0, 24, 1, 2, 8, 9, 10, 16, 17]):
        rank[p] = r
    rest = [r for r in range(FR_R) if r not in set(rank[rank >= 0])]
    rank[rank < 0] = rs.permutation(rest)
    t = np.where(rank < FR_R - 40, 1.5 - 0.002 * rank, -3.0)
    logits = np.full((FR_R, FR_C), -20.0, F32)
    logits[:, 0] = 0.0
    logits[:, 1:1 + FR_FLAT] = t[:, None].astype(F32)
    lg = logits.astype(np.float64)
    e = np.exp(lg - lg.max(1, keepdims=True))
    return logits, np.zeros((FR_R, 4 * FR_C), F32), boxes, e / e.sum(1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _frcnn_case(orc, det_max):
    logits, deltas, boxes, prob = _frcnn_inputs()
    Hr, Wr = FR_HW
    idx, margin, ncand = R.frcnn(prob, boxes, Hr, Wr, 0.05, 0.5, det_max)
    want = orc.frcnn_postprocess(logits, deltas, boxes.astype(F32), Hr, Wr, 2 * Hr, 4 * Wr, 0.05, 0.5, det_max)
    return dict(idx=idx, margin=margin, ncand=ncand, want=want)


def _check_frcnn(out, case, det_max):
    logits, deltas, boxes, prob = _frcnn_inputs()
    idx = case["idx"]
    scale = np.array([4.0, 2.0, 4.0, 2.0])
    assert len(out["labels"]) == len(idx) == det_max
    np.testing.assert_array_equal(out["labels"], idx[:, 1])
    np.testing.assert_array_equal(out["props"], (boxes[idx[:, 0]] * scale).astype(F32))
    np.testing.assert_array_equal(out["boxes"], (boxes[idx[:, 0]] * scale).astype(F32))
    np.testing.assert_allclose(out["scores"], prob[idx[:, 0], idx[:, 1]], rtol=0, atol=1e-5)
    np.testing.assert_allclose(out["scores_cls"], prob[idx[:, 0]], rtol=0, atol=1e-5)


@pytest.mark.parametrize("det_max", DET_MAX)
def test_frcnn_restatement_equals_oracle(orc, det_max):
    case = _frcnn_case(orc, det_max)
    print("frcnn det_max %d: candidates %d, min |IoU - 1/2| %.6g" % (det_max, case["ncand"], case["margin"]))
    assert case["ncand"] == 9600 and case["ncand"] > 8192          # the global-key branch of post_nms_kernel
    assert case["margin"] >= MARGIN
    _check_frcnn(case["want"], case, det_max)
    if det_max >= 100:
        pairs = [tuple(v) for v in case["idx"]]
        for c in range(1, 1 + FR_FLAT):
            assert (0, c) in pairs and (24, c) in pairs and (1, c) not in pairs and (2, c) in pairs          # chain inside the first chunk
            assert (8, c) in pairs and (9, c) not in pairs and (10, c) in pairs                              # chain across the chunk boundary
            assert (16, c) in pairs and (17, c) in pairs                                                     # IoU exactly 1/2 is not `>`
        assert pairs[:20] == [(0, c) for c in range(1, 11)] + [(24, c) for c in range(1, 11)]            # 20 kept before the first suppression


def gpu_frcnn(hip, logits, deltas, props, Hr, Wr, Ho, Wo, det_max, score_thr=0.05, nms_thr=0.5):
    ffi, L = hip["ffi"], hip["L"]
    logits, deltas, props = [np.ascontiguousarray(a, F32) for a in (logits, deltas, props)]
    Rn, Cn = logits.shape
    ob = np.empty((det_max, 4), F32); osc = np.empty(det_max, F32); ol = np.empty(det_max, np.int64); op = np.empty((det_max, 4), F32)
    opm = np.empty(det_max, F32); ocl = np.empty((det_max, Cn), F32); n = C.c_int(-1)
    ffi.check(L.cald_op_frcnn_postprocess(hip["ctx"], Rn, Cn, ffi.ptr(logits), ffi.ptr(deltas), ffi.ptr(props), Hr, Wr, Ho, Wo, score_thr, nms_thr, det_max,
                                          ffi.ptr(ob), ffi.ptr(osc), ffi.ptr(ol, ffi.c_i64), ffi.ptr(op), ffi.ptr(opm), ffi.ptr(ocl), C.byref(n)))
    m = n.value
    assert 0 <= m <= det_max
    return dict(boxes=ob[:m].copy(), scores=osc[:m].copy(), labels=ol[:m].copy(), props=op[:m].copy(), prob_max=opm[:m].copy(),
                scores_cls=ocl[:m].copy())


@pytest.mark.gpu
@pytest.mark.parametrize("det_max", DET_MAX)
def test_frcnn_postprocess_kernels_beyond_the_lds_key_capacity(hip, orc, det_max):
    """post_softmax_kernel / post_nms_kernel with 9600 > 8192 candidates: bytes vs the oracle, (proposal, label) order vs the restatement."""
    case = _frcnn_case(orc, det_max)
    assert case["ncand"] > 8192
    logits, deltas, boxes, prob = _frcnn_inputs()
    got = gpu_frcnn(hip, logits, deltas, boxes, FR_HW[0], FR_HW[1], 2 * FR_HW[0], 4 * FR_HW[1], det_max)
    _check_frcnn(got, case, det_max)
    _assert_bytes(got, case["want"], det_max)


# ---------------------------------------------------------------------------------------------------------------------------
# RPN: radix select (early exit vs eight passes), n against k, the 1024 / 2048 template switch, level NMS, merge
# ---------------------------------------------------------------------------------------------------------------------------
RPN_CFGS = [(64, 64, 64, 64, 64, 50), (128, 128, 128, 128, 1024, 300), (128, 128, 128, 128, 1025, 300), (64, 96, 37, 50, 2048, 2048),
            (128, 160, 120, 148, 1000, 1000)]
RPN_CASES = [cfg + (pat,) for cfg in RPN_CFGS for pat in ("equal", "perm", "ties")]
# a level of exactly pre_n anchors (16 x 16 x 3 = 768: no selection) and of pre_n + 1 (the selection drops one anchor)
RPN_CASES += [(64, 64, 64, 64, 768, 300, "equal"), (64, 64, 64, 64, 768, 300, "perm"), (64, 64, 64, 64, 767, 300, "equal"), (64, 64, 64, 64, 767, 300, "perm")]


def _rpn_levels(Hp, Wp):
    hw = [(Hp // 4, Wp // 4), (Hp // 8, Wp // 8), (Hp // 16, Wp // 16), (Hp // 32, Wp // 32)]
    hw.append(((hw[-1][0] - 1) // 2 + 1, (hw[-1][1] - 1) // 2 + 1))
    return hw


def _rpn_heads(Hp, Wp, pattern, seed):
    """zero-delta heads [H][W][15]: all logits equal (eight radix passes, the index half decides), a permutation (all distinct within a
    level, ties across levels), coarse ties (eight values)."""
    rs = np.random.RandomState(seed)
    heads = []
    for h, w in _rpn_levels(Hp, Wp):
        n = h * w * 3
        lg = {"equal": np.zeros(n), "perm": (rs.permutation(n) - n // 2) / 64.0, "ties": rs.randint(0, 8, n) * 0.25}[pattern]
        head = np.zeros((h, w, 15), F32)
        head[:, :, :3] = lg.reshape(h, w, 3)
        heads.append(head)
    return heads


def _rpn_base(orc):
    return np.stack([orc.base_anchors([s], [0.5, 1.0, 2.0]) for s in (32, 64, 128, 256, 512)])      # [5][3][4]


def _rpn_reference(orc, heads, Hp, Wp, Hr, Wr, pre, post):
    base = _rpn_base(orc)
    props, scores = orc.rpn_proposals(heads, base, Hp, Wp, Hr, Wr, A=3, pre_n=pre, post_n=post, nms_thr=0.7, min_size=1e-3)
    logits = [h[:, :, :3].reshape(-1) for h in heads]
    anchors = [R.grid_anchors(base[l], h.shape[0], h.shape[1], Hp // h.shape[0], Wp // h.shape[1]) for l, h in enumerate(heads)]
    idx, boxes, margin = R.rpn(logits, anchors, Hr, Wr, pre, post, 0.7, 1e-3)
    return dict(props=props, scores=scores, idx=idx, boxes=boxes, margin=margin, logits=logits)


@functools.lru_cache(maxsize=None)
def _rpn_case(orc, case):
    Hp, Wp, Hr, Wr, pre, post, pattern = case
    heads = _rpn_heads(Hp, Wp, pattern, seed=pre + Hr)
    ref = _rpn_reference(orc, heads, Hp, Wp, Hr, Wr, pre, post)
    ref["heads"] = heads
    return ref


def _check_rpn_reference(ref):
    assert ref["margin"] >= MARGIN, ref["margin"]
    assert len(ref["props"]) == len(ref["idx"])
    np.testing.assert_array_equal(ref["props"], ref["boxes"].astype(F32))
    np.testing.assert_array_equal(ref["scores"], np.array([ref["logits"][l][i] for l, i in ref["idx"]], F32))      # raw logits, in order


@pytest.mark.parametrize("case", RPN_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_rpn_restatement_equals_oracle(orc, case):
    ref = _rpn_case(orc, case)
    print("rpn %s: proposals %d, min |IoU - 7/10| %.6g" % (case, len(ref["idx"]), ref["margin"]))
    _check_rpn_reference(ref)
    n0 = ref["logits"][0].size
    if case[4] in (767, 768):
        assert n0 == 768


def gpu_rpn(hip, heads_per_view, Hp, Wp, image_sizes, pre, post):
    torch = hip["torch"]
    from cald_amd import train_ops
    dev = []
    for l in range(5):
        h16 = np.zeros((len(heads_per_view),) + heads_per_view[0][l].shape[:2] + (16,), F32)
        for v, heads in enumerate(heads_per_view):
            h16[v, :, :, :15] = heads[l]
        dev.append(torch.from_numpy(h16).cuda().contiguous())
    props, counts = train_ops.rpn_proposals(dev, Hp, Wp, image_sizes, pre_n=pre, post_n=post, nms_thr=0.7, min_size=1e-3)
    props, counts = props.cpu().numpy(), counts.cpu().numpy()
    return [props[v, :int(counts[v])].copy() for v in range(len(heads_per_view))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", RPN_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_rpn_kernels_on_constructed_logits(hip, orc, case):
    """rpn_topk_kernel<1024 / 2048>, rpn_level_nms_kernel, rpn_merge_kernel: the proposal list, in order, bytes vs the oracle and equal to
    the restatement's boxes (integers: exact in float32)."""
    Hp, Wp, Hr, Wr, pre, post, _ = case
    ref = _rpn_case(orc, case)
    got = gpu_rpn(hip, [ref["heads"]], Hp, Wp, [(Hr, Wr)], pre, post)[0]
    assert got.shape == ref["props"].shape, (got.shape, ref["props"].shape)
    np.testing.assert_array_equal(got, ref["boxes"].astype(F32))
    assert got.tobytes() == ref["props"].tobytes()


@functools.lru_cache(maxsize=None)
def _rpn_two_views(orc):
    Hp, Wp, pre, post = 128, 160, 1000, 1000
    views = [((120, 148), _rpn_heads(Hp, Wp, "perm", 11)), ((97, 160), _rpn_heads(Hp, Wp, "ties", 12))]
    return Hp, Wp, pre, post, views, [_rpn_reference(orc, h, Hp, Wp, hr, wr, pre, post) for (hr, wr), h in views]


def test_rpn_two_view_restatement_equals_oracle(orc):
    for ref in _rpn_two_views(orc)[5]:
        _check_rpn_reference(ref)


@pytest.mark.gpu
def test_rpn_two_view_batch_equals_the_single_view_runs(hip, orc):
    """one launch over two views with different resized sizes and logits: each view equals its own single-view launch and the oracle"""
    Hp, Wp, pre, post, views, refs = _rpn_two_views(orc)
    both = gpu_rpn(hip, [h for _, h in views], Hp, Wp, [s for s, _ in views], pre, post)
    for v, ((size, heads), ref) in enumerate(zip(views, refs)):
        single = gpu_rpn(hip, [heads], Hp, Wp, [size], pre, post)[0]
        assert both[v].shape == single.shape and both[v].tobytes() == single.tobytes(), v
        assert both[v].tobytes() == ref["props"].tobytes(), v
        np.testing.assert_array_equal(both[v], ref["boxes"].astype(F32))


# ---------------------------------------------------------------------------------------------------------------------------
# Scoring: the chunked path of consistency_kernel (M > 2048 detections)
# ---------------------------------------------------------------------------------------------------------------------------
SCORE_M = [2047, 2048, 2049, 4096, 4100]
SC_N, SC_C = 50, 21


SAME_LANE_PAIR = (1984, 2112)          # 31 * 64 and 2048 + 64: both fall to lane 0, in chunk 0 and in chunk 1


@functools.lru_cache(maxsize=None)
def _scoring_case(M):
    """50 integer reference boxes against M integer detections.  Exact copies of reference boxes sit at detection 0, 2047, 2048, 2049, 4095,
    4096 and M - 1 (those below M).  The detections at the chunk boundary (2047, 2048; the last two when M <= 2048) are the upper and the
    lower half of reference box F: both have IoU exactly 1/2 with F, the first index must win.  That pair meets only in the reduction
    across lanes (lane 63 and lane 0).  Where M allows it, detections 1984 and 2112 are the halves of a second reference box G: one lane
    meets both, in different chunks, and the chunk-local index of the later one (64) is below the global index of the earlier one -- an
    argmax that compared a local with a global index would pick 2112."""
    rs = np.random.RandomState(M)
    x, y = rs.randint(500, 3800, M), rs.randint(500, 3800, M)
    boxes = np.stack([x, y, x + rs.randint(30, 200, M), y + rs.randint(30, 200, M)], 1).astype(np.float64)
    refs = boxes[rs.choice(M, SC_N, replace=False)] + rs.randint(-10, 11, (SC_N, 4))
    pair = (2047, 2048) if M > 2048 else (M - 2, M - 1)
    boxes[pair[0]] = [100, 100, 200, 150]; boxes[pair[1]] = [100, 150, 200, 200]
    special = sorted({p for p in (0, 2047, 2048, 2049, 4095, 4096, M - 1) if p < M} | set(pair))
    slots = [(5 + 6 * k) % SC_N for k in range(len(special) + 2)]        # spread over the rounds and waves of the kernel
    assert len(set(slots)) == len(slots)
    expect = {slots[0]: pair[0]}
    refs[slots[0]] = [100, 100, 200, 200]
    for s, p in zip(slots[1:], special):
        refs[s] = boxes[p]; expect[s] = p
    if M > SAME_LANE_PAIR[1]:
        assert SAME_LANE_PAIR[0] % 64 == SAME_LANE_PAIR[1] % 64 and SAME_LANE_PAIR[0] < 2048 <= SAME_LANE_PAIR[1]
        assert SAME_LANE_PAIR[1] - 2048 < SAME_LANE_PAIR[0] and not set(SAME_LANE_PAIR) & set(special)
        boxes[SAME_LANE_PAIR[0]] = [300, 100, 400, 150]; boxes[SAME_LANE_PAIR[1]] = [300, 150, 400, 200]
        refs[slots[-1]] = [300, 100, 400, 200]; expect[slots[-1]] = SAME_LANE_PAIR[0]
    arg, gap = R.iou_argmax(refs, boxes)
    return dict(refs=refs.astype(F32), boxes=boxes.astype(F32), arg=arg, gap=gap, expect=expect)


def _isolating_inputs(M, k):
    """score inputs under which the result of the pair is a function of reference box k's (best IoU, argmax) alone: uniform class
    vectors (JS = 0), prob_max = j / 32768 for detection j, a prob_max of 1000 for every other reference box (score > 1, never the
    minimum): consistency = |best_k - 1/2 + j / 65536|."""
    scls_r = np.full((SC_N, SC_C), 1.0 / SC_C, F32); scls_d = np.full((M, SC_C), 1.0 / SC_C, F32)
    pm_r = np.full(SC_N, 1000.0, F32); pm_r[k] = 0.0
    return scls_r, pm_r, scls_d, (np.arange(M) / 32768.0).astype(F32), 0.5


def _natural_inputs(M):
    rs = np.random.RandomState(M + 1)
    scls_r = rs.dirichlet(np.ones(SC_C), SC_N).astype(F32); scls_d = rs.dirichlet(np.ones(SC_C), M).astype(F32)
    return scls_r, scls_r[:, 1:].max(1), scls_d, scls_d[:, 1:].max(1), 1.3


@pytest.mark.parametrize("M", SCORE_M)
def test_scoring_restatement_equals_oracle(orc, M):
    case = _scoring_case(M)
    print("scoring M %d: min gap between best and second IoU %.6g" % (M, case["gap"]))
    assert case["gap"] >= 1e-6            # far above a float32 rounding of an IoU: the argmax is the same in any precision
    for s, p in case["expect"].items():
        assert case["arg"][s] == p, (s, p, case["arg"][s])
    scls_r, pm_r, scls_d, pm_d, bp = _natural_inputs(M)
    _, d = orc.consistency_view(case["refs"], scls_r, pm_r, case["boxes"], scls_d, pm_d, bp, detail=True)
    np.testing.assert_array_equal(d[1], case["arg"])
    for k in case["expect"]:              # the isolating inputs do isolate: the oracle's score of pair k is the stated function of (best, argmax)
        scls_r, pm_r, scls_d, pm_d, bp = _isolating_inputs(M, k)
        s, d = orc.consistency_view(case["refs"], scls_r, pm_r, case["boxes"], scls_d, pm_d, bp, detail=True)
        assert d[1][k] == case["arg"][k] and d[2][k] == 0.0
        assert abs(s - abs(float(d[0][k]) - 0.5 + case["arg"][k] / 65536.0)) <= 1e-6


def gpu_consistency(hip, refs, scls_r, pm_r, boxes, scls_d, pm_d, bp):
    ffi, L = hip["ffi"], hip["L"]
    refs, scls_r, pm_r, boxes, scls_d, pm_d = [np.ascontiguousarray(a, F32) for a in (refs, scls_r, pm_r, boxes, scls_d, pm_d)]
    out = np.zeros(1, F32)
    ffi.check(L.cald_op_consistency(hip["ctx"], refs.shape[0], ffi.ptr(refs), ffi.ptr(scls_r), ffi.ptr(pm_r), boxes.shape[0], ffi.ptr(boxes),
                                    ffi.ptr(scls_d), ffi.ptr(pm_d), scls_r.shape[1], bp, ffi.ptr(out)))
    return out[0]


@pytest.mark.gpu
@pytest.mark.parametrize("M", SCORE_M)
def test_consistency_kernel_chunked_detection_lists(hip, orc, M):
    """consistency_kernel around SCORE_LDS_BOXES = 2048: the score bytes vs the oracle on natural inputs, and once per reference box on
    inputs that make the score a function of that box's (best IoU, argmax) alone -- the kernel returns only the minimum over the boxes."""
    case = _scoring_case(M)
    scls_r, pm_r, scls_d, pm_d, bp = _natural_inputs(M)
    want = F32(orc.consistency_view(case["refs"], scls_r, pm_r, case["boxes"], scls_d, pm_d, bp))
    got = gpu_consistency(hip, case["refs"], scls_r, pm_r, case["boxes"], scls_d, pm_d, bp)
    assert got.tobytes() == want.tobytes(), (M, got, want)
    for k in range(SC_N):
        scls_r, pm_r, scls_d, pm_d, bp = _isolating_inputs(M, k)
        want, d = orc.consistency_view(case["refs"], scls_r, pm_r, case["boxes"], scls_d, pm_d, bp, detail=True)
        assert d[1][k] == case["arg"][k]
        got = gpu_consistency(hip, case["refs"], scls_r, pm_r, case["boxes"], scls_d, pm_d, bp)
        assert got.tobytes() == F32(want).tobytes(), (M, k, got, want, case["arg"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 6300])
def test_cls_corr_kernel_list_lengths(hip, orc, n):
    """cls_corr_kernel on an empty list, one detection and RetinaNet's longest list (21 x 300), label 0 included (python's negative index)"""
    ffi, L = hip["ffi"], hip["L"]
    rs = np.random.RandomState(n)
    sc = rs.rand(n).astype(F32); lab = (np.arange(n) % SC_C).astype(np.int64)
    rs.shuffle(lab)
    out = np.full(SC_C - 1, -1.0, F32)
    ffi.check(L.cald_op_cls_corr(hip["ctx"], n, ffi.ptr(sc), ffi.ptr(lab, ffi.c_i64), SC_C, ffi.ptr(out)))
    want = orc.cls_corr_view(sc, lab, SC_C)
    assert out.tobytes() == want.tobytes()
    ref = np.zeros(SC_C - 1)
    for s, l in zip(sc.astype(np.float64), lab):
        ref[(l - 1) % (SC_C - 1)] = max(ref[(l - 1) % (SC_C - 1)], s)
    np.testing.assert_array_equal(out, ref.astype(F32))


# ---------------------------------------------------------------------------------------------------------------------------
# The hooks above run the forward's own scratch layout and argument filling (host.h: RetinaTailBufs / PostBufs / RoiBufs and
# retina_args / post_args / roi_args): fed a forward's intermediate tensors, each returns that forward's bytes.
# ---------------------------------------------------------------------------------------------------------------------------
from test_gpu_parity import _gpu_roi_align, small_model, small_retina      # noqa: E402,F401  (the 300 / 500 models of the parity tests)


def _one_view(hip, model):
    from cald_amd import synth, train_ops
    img = synth.make_pool(3, "voc", 0, scale=0.5)[1]
    got = model.forward_views([(hip["torch"].from_numpy(img).cuda(), False, None)])[0]
    Hr, Wr, Hp, Wp = train_ops.transform_size(img.shape[0], img.shape[1], model.cfg.min_size, model.cfg.max_size)
    return img, {k: v.cpu().numpy() for k, v in got.items()}, (Hp, Wp, Hr, Wr)


@pytest.mark.gpu
def test_retina_hook_on_the_forwards_head_maps_returns_the_forwards_detections(hip, orc, small_retina):
    model, _ = small_retina
    img, want, sizes = _one_view(hip, model)
    cls = [model.debug_tensor("cls%d" % l, 0) for l in range(5)]; reg = [model.debug_tensor("reg%d" % l, 0) for l in range(5)]
    got = gpu_retina(hip, cls, reg, _retina_base(orc), model.num_classes, 9, sizes, img.shape[:2], model.cfg.detections_per_img,
                     model.cfg.box_score_thresh, model.cfg.box_nms_thresh)
    assert len(want["labels"]) > 0
    _assert_bytes(got, want, "retina tail")


def _frcnn_view(hip, orc, small_model):
    model, P = small_model
    img, want, sizes = _one_view(hip, model)
    keep = {}
    orc.frcnn_forward(P, img, 300, 500, keep=keep)
    n = keep["proposals"].shape[0]
    assert 0 < n <= 1000
    return model, img, want, sizes, np.ascontiguousarray(model.debug_tensor("proposals", 0).reshape(-1, 4)[:n])


@pytest.mark.gpu
def test_frcnn_hook_on_the_forwards_predictions_returns_the_forwards_detections(hip, orc, small_model):
    model, img, want, (Hp, Wp, Hr, Wr), props = _frcnn_view(hip, orc, small_model)
    Cn = model.num_classes
    pred = model.debug_tensor("pred", 0).reshape(1000, 5 * Cn)[:len(props)]
    got = gpu_frcnn(hip, pred[:, :Cn], pred[:, Cn:], props, Hr, Wr, img.shape[0], img.shape[1], model.cfg.detections_per_img,
                    model.cfg.box_score_thresh, model.cfg.box_nms_thresh)
    assert set(want) == set(got) and len(want["labels"]) > 0          # all six outputs; the count is their common length
    assert len(got["labels"]) == len(want["labels"])
    _assert_bytes(got, want, "frcnn tail")


@pytest.mark.gpu
def test_roi_align_hook_on_the_forwards_pyramid_returns_the_forwards_rows(hip, orc, small_model):
    model, _, _, _, props = _frcnn_view(hip, orc, small_model)
    got = _gpu_roi_align(hip, [model.debug_tensor("P%d" % (2 + l), 0) for l in range(4)], props)
    want = model.debug_tensor("roi", 0).reshape(1000, 49, 256)[:len(props)]
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
