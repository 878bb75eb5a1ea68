"""The scoring stage without a GPU: the numpy restatement of score.hip (tests/_score_restatement.py) against the oracle on the constructed
cases of tests/_score_cases.py, the host-only hooks cald_op_pair_params and cald_op_ls_tail against both, and the proof that the cases
would notice each of the mistakes the restatement can be told to make.  test_gpu_score_batch.py runs the same cases through the
kernels."""
import ctypes as C
import functools

import numpy as np
import pytest

import _score_cases as K
import _score_restatement as R

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _case(Cn):
    return K.batch_case(Cn)


@functools.lru_cache(maxsize=None)
def _expected(Cn, wrong=()):
    from oracle import oracle as orc
    orc.build()
    return R.score_batch(_case(Cn), orc.js_divergence, wrong)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(got, want, what):
    """byte for byte, except that a NaN equals a NaN of any payload"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert _bits(np.where(nan, 0, got)) == _bits(np.where(nan, 0, want)), what


def _rows(case, p):
    """pair p as the oracle takes it: transformed reference boxes, their class vectors and prob_max, the view's detections"""
    rv, av, img = int(case["ref_view"][p]), int(case["aug_view"][p]), int(case["pair_img"][p])
    sel = R.selection(case, img)
    M = int(case["count"][av])
    ab = R.aug_box(case["boxes"][rv][sel], int(case["aug_kind"][p]), case["aug_param"][p])
    return sel, ab, (case["scores_cls"][rv][sel], case["prob_max"][rv][sel], case["boxes"][av][:M], case["scores_cls"][av][:M], case["prob_max"][av][:M])


@pytest.mark.parametrize("Cn", [21, 91])
def test_batch_restatement_equals_oracle(oracle, Cn):
    """consistency (with the per-row best IoU, argmax and score), class-max vectors, lt_c and the max-IoU rows of every pair and view"""
    case, want = _case(Cn), _expected(Cn)
    for p in range(case["P"]):
        sel, ab, rest = _rows(case, p)
        detail = []
        got = R.consistency(ab, *rest, case["bp"], oracle.js_divergence, detail=detail)
        if len(rest[2]) and len(sel):
            cons, d = oracle.consistency_view(ab, *rest, case["bp"], detail=True)
            _same(np.array([x[0] for x in detail], F32), d[0], ("max iou", p))
            assert [x[1] for x in detail] == d[1].tolist(), ("argmax", p)
            _same(np.array([x[2] for x in detail], F32), d[3], ("score", p))
        else:
            cons = oracle.consistency_view(ab, *rest, case["bp"]) if len(sel) else (1.0 if len(rest[2]) else 0.0)
        _same(F32(got), F32(cons), ("consistency", p))
        _same(want["cons"][p], F32(cons), ("batch consistency", p))
        # ls_c's rows: the untransformed boxes, through the oracle's own walk
        refs = case["boxes"][int(case["ref_view"][p])][sel]
        row = np.zeros(len(sel), F32)
        if len(sel) and len(rest[2]):
            oracle.lib().orc_max_iou_rows(C.c_int(len(sel)), oracle._p(oracle.f32(refs)), C.c_int(len(rest[2])), oracle._p(oracle.f32(rest[2])), oracle._p(row))
        _same(want["max_iou"][p, :len(sel)], row, ("max iou rows", p))
    for v in range(case["V"]):
        n = int(case["count"][v])
        sel = np.array(R.selection(case, int(case["view_img"][v])), int) if case["view_isref"][v] else np.arange(n)
        _same(want["cls_corr"][v], oracle.cls_corr_view(case["scores"][v][sel], case["labels"][v][sel], Cn), ("cls_corr", v))
        out = dict(boxes=case["boxes"][v][:n], props=case["props"][v][:n], prob_max=case["prob_max"][v][:n])
        _same(want["lt"][v], F32(oracle.lt_uncertainty(out)), ("lt", v))


def test_batch_reaches_its_edges():
    """what the case table promises, so that it cannot lose an edge silently"""
    case = _case(21)
    cnt = case["count"]
    assert sorted(set(cnt[case["aug_view"]])) == [0, 1, 63, 64, 65, 100, 2049]
    assert sorted(set(case["aug_kind"])) == [0, 1, 2, 3] and sorted(case["ref_n"]) == [0, 3, 50]
    assert case["ref_sel"][0].tolist() == R.subsample_indices(73).tolist() and case["ref_sel"][1][:3].tolist() == sorted(case["ref_sel"][1][:3], reverse=True)
    chunked = cnt[case["aug_view"]] > R.CHUNK
    assert 0 < chunked.sum() < len(chunked) and set(case["pair_img"][chunked]) == {0, 1}
    gap = np.inf
    zero_rows = tied = 0
    ties = {(p, r): (a, b) for p, r, a, b in case["ties"]}
    for p in range(case["P"]):
        sel, ab, rest = _rows(case, p)
        if not len(sel) or len(rest[2]) < 2:
            continue
        iou = R.iou_matrix(ab, rest[2])
        if case["pair_img"][p] == 1 and len(rest[2]) <= R.CHUNK:      # image 1's own views isolate one row: the other two meet nothing
            assert ((iou.max(1) == 0).sum(), (iou.max(1) > 0).sum()) == (2, 1), p
        for r in range(len(sel)):
            if (p, r) in ties:
                a, b = ties[(p, r)]
                assert iou[r, a] == iou[r, b] == F32(0.5) == iou[r].max() and a < b
                tied += 1
            elif iou[r].max() == 0:
                zero_rows += 1                      # exact zeros: disjoint integer boxes
            else:
                gap = min(gap, R.second_gap(iou[r:r + 1]))
    print("smallest gap between best and second IoU: %.6g (%d all-zero rows, %d deliberate ties)" % (gap, zero_rows, tied))
    assert gap >= 1e-6 and zero_rows > 0 and tied == 2
    want = _expected(21)
    assert set(want["pair_audit"][:, 1]) == {0.0, 1.0} and np.isinf(want["pair_audit"][:, 0]).any() and (want["pair_audit"][:, 0] < 1).any()
    for v in range(case["V"]):                      # label 0 and a label beyond the table among what counts; they decide the last slot
        n = int(cnt[v])
        if n >= 3 and not (case["view_isref"][v] and case["ref_n"][case["view_img"][v]] < 2):
            assert (case["labels"][v][:n] == 0).any() and (case["labels"][v][:n] >= 21).any() and want["cls_corr"][v][-1] == F32(0.97)
            assert want["cls_corr"][v].max() == F32(0.97)


@pytest.mark.parametrize("wrong", R.WRONG)
def test_cases_notice_the_mistake(oracle, wrong):
    """a restatement with one deliberate mistake changes at least one expected output of the constructed cases"""
    differs = []
    if wrong == "ls_ties_reversed":
        differs = [c["name"] for c in K.ls_cases() if R.ls_select(c["pm"]) != R.ls_select(c["pm"], (wrong,))]
    elif wrong == "lt_no_plus_1":
        case = K.lt_case(0)
        good, bad = R.score_batch(case, None), R.score_batch(case, None, (wrong,))
        differs = [v for v in range(case["V"]) if _bits(good["lt"][v]) != _bits(bad["lt"][v])]
    else:
        good, bad = _expected(21), _expected(21, (wrong,))
        differs = [k for k in good if _bits(good[k]) != _bits(bad[k])]
    print(wrong, "changes", differs)
    assert differs


def test_nan_iou_is_maximal_as_in_the_oracle(oracle):
    """two boxes without area at one point: 0 / 0.  The first NaN is the argmax, the row's maximum is NaN, the audit counts the row as
    one without a positive IoU"""
    refs = np.array([[10, 10, 10, 10], [0, 0, 20, 20]], F32)
    boxes = np.array([[0, 0, 5, 5], [10, 10, 10, 10], [10, 10, 10, 10], [0, 0, 20, 20]], F32)
    scls = np.full((4, 5), 0.2, F32); pm = np.array([0.1, 0.2, 0.3, 0.4], F32)
    detail = []
    got = R.consistency(refs, scls[:2], pm[:2], boxes, scls, pm, 1.3, oracle.js_divergence, detail=detail)
    cons, d = oracle.consistency_view(refs, scls[:2], pm[:2], boxes, scls, pm, 1.3, detail=True)
    assert [x[1] for x in detail] == d[1].tolist() == [1, 3] and np.isnan(detail[0][0]) and np.isnan(d[0][0])
    _same(F32(got), F32(cons), "consistency")
    row = np.zeros(2, F32)
    oracle.lib().orc_max_iou_rows(C.c_int(2), oracle._p(refs), C.c_int(4), oracle._p(boxes), oracle._p(row))
    _same(R.max_iou_rows(refs, boxes), row, "max iou rows")
    assert np.isnan(row[0]) and row[1] == 1.0
    gap, zero = R.pair_audit(refs, boxes, boxes)
    assert zero == 1.0 and gap == F32(1.0) - R.iou_matrix(refs[1:], boxes[:1])[0, 0]


def test_lt_case_restatement_equals_oracle(oracle):
    for turn in K.LT_TURNS:
        case = K.lt_case(turn)
        want = R.score_batch(case, None)["lt"]
        assert want[0] == 1.0
        for v, n in enumerate(K.LT_COUNTS):
            out = dict(boxes=case["boxes"][v][:n], props=case["props"][v][:n], prob_max=case["prob_max"][v][:n])
            _same(want[v], F32(oracle.lt_uncertainty(out)), (turn, v))
            if n:                                   # the planted minimum wins, not the NaN, not the proposal-equal detection
                k = case["where"][v - 1]
                _same(want[v], R.lt_uncertainty(case["boxes"][v][k:k + 1], case["props"][v][k:k + 1], case["prob_max"][v][k:k + 1]), (turn, v))
                assert want[v] < 0.01


def test_aug_box_equals_the_oracles_transforms(oracle):
    rs = np.random.RandomState(3)
    for (H, W) in K.IMG_HW:
        b = K._rand_boxes(rs, 40, 0, 0, W, H, 5, 40)
        b[0] = [0, 0, 30, 20]; b[1] = [W - 30, H - 20, W, H]; b[2] = [0, H - 20, 30, H]
        _same(R.aug_box(b, 0, R.pair_params(0, H, W)), b, "identity")
        _same(R.aug_box(b, 1, R.pair_params(1, H, W)), oracle.flip_boxes(b, W), "flip")
        for ratio in (0.8, 1.2):
            _same(R.aug_box(b, 2, R.pair_params(2, H, W, ratio)), (b * np.float32(ratio)).astype(F32), "resize")
        img = np.zeros((H, W, 3), np.uint8)
        for angle in (5.0, -5.0, 90.0, 37.0):
            _same(R.aug_box(b, 3, R.pair_params(3, H, W, angle)), oracle.rotate_aug(img, b, angle)[1], ("rotate", angle))
    for n in (0, 1, 40, 41, 73, 100, 1000):
        assert R.subsample_indices(n).tolist() == oracle.subsample_indices(n).tolist()


def test_pair_params_hook_equals_restatement():
    from cald_amd import _ffi
    L = _ffi.lib()
    canvases = set()
    for (H, W) in K.IMG_HW + [(37, 53)]:
        for kind, prm in ((0, 0.0), (1, 0.0), (2, 0.8), (2, 1.2), (3, 5.0), (3, -5.0), (3, 90.0), (3, 37.0), (3, 270.0)):
            got = np.full(12, 7.0, F32)
            _ffi.check(L.cald_op_pair_params(kind, H, W, prm, _ffi.ptr(got)))
            _same(got, R.pair_params(kind, H, W, prm), (H, W, kind, prm))
            if kind == 3:
                canvases.add(R.rotate_canvas(H, W, prm) == (W, H))
    assert canvases == {False}                      # every rotation here changes the canvas: sx, sy are not 1
    assert L.cald_op_pair_params(4, 10, 10, 0.0, _ffi.ptr(np.zeros(12, F32))) != 0
    assert L.cald_op_pair_params(1, 10, 10, 0.0, None) != 0 and L.cald_op_pair_params(1, 0, 10, 0.0, _ffi.ptr(np.zeros(12, F32))) != 0


def test_ls_tail_hook_equals_restatement_and_oracle(oracle):
    from cald_amd import _ffi
    L = _ffi.lib()
    worst = 0.0
    for c in K.ls_cases():
        pm, n = c["pm"], len(c["pm"])
        sel = np.full(30, -1, np.int32); nsel = C.c_int(-1); score = C.c_double(-1.0)
        want_sel = R.ls_select(pm)
        N = len(want_sel)
        rows = np.stack([R.max_iou_rows(c["ref"][want_sel], v) for v in c["views"]]) if N else np.zeros((6, 0), F32)
        _ffi.check(L.cald_op_ls_tail(n, _ffi.ptr(pm), 6, _ffi.ptr(np.ascontiguousarray(rows)), _ffi.ptr(sel, _ffi.c_i), C.byref(nsel), C.byref(score)))
        assert nsel.value == N == min(n, 30) and sel[:N].tolist() == want_sel and (sel[N:] == -1).all(), c["name"]
        assert want_sel == (oracle.topk_indices(pm, 30).tolist() if n > 30 else list(range(n))), c["name"]
        assert (rows[3] == 0).all()
        want = R.ls_tail(pm[want_sel], rows)
        ref = dict(boxes=c["ref"], prob_max=pm)
        orc_score = oracle.ls_score_image(ref, [dict(boxes=v) for v in c["views"]])
        worst = max(worst, abs(score.value - want), abs(score.value - orc_score))
        assert score.value == want == orc_score, (c["name"], score.value, want, orc_score)
        sel2 = np.full(30, -1, np.int32)
        _ffi.check(L.cald_op_ls_tail(n, _ffi.ptr(pm), 0, None, _ffi.ptr(sel2, _ffi.c_i), C.byref(nsel), None))       # selection only
        assert sel2.tolist() == sel.tolist()
    print("ls_c score: largest difference between hook, restatement and oracle %.3g" % worst)
    names = [c["name"] for c in K.ls_cases()]
    assert {"n0", "n1", "n7", "n8", "n9", "n29", "n30", "n31", "n100", "ties_across_rank_30", "all_equal"} <= set(names)
    ties = [c for c in K.ls_cases() if c["name"] == "ties_across_rank_30"][0]
    order = sorted(range(40), key=lambda i: (-ties["pm"][i], i))
    assert ties["pm"][order[28]] == ties["pm"][order[29]] == ties["pm"][order[30]] and ties["pm"][order[27]] > ties["pm"][order[28]] > ties["pm"][order[31]]
    assert L.cald_op_ls_tail(-1, None, 0, None, _ffi.ptr(sel, _ffi.c_i), C.byref(nsel), None) != 0
    assert L.cald_op_ls_tail(3, _ffi.ptr(np.zeros(3, F32)), 0, None, None, C.byref(nsel), None) != 0
