"""GPU tests of the RetinaNet SSM tail (cald_amd/csrc/retina_ssm.hip: cald_op_retina_ssm_postprocess, cald_sweep_ssm_retina) and of
cald_amd/ssm.py on a RetinaNet end to end.

The hook gets its picks from a ctypes callback the test controls.  Three yardsticks:
  * identity picks (0 .. n_c - 1): the stock tail, cald_op_retina_postprocess, whose kernels are pinned to the oracle -- bit for bit;
  * other picks: tests/_retina_ssm_restatement.py on the oracle's exponential (the library's sigmoid bits), with zero deltas and integer
    anchors, so that boxes are exact and an IoU is the correctly rounded quotient of two integers -- each case asserts that every IoU the
    NMS met is exactly the threshold's rational or at least 1e-6 away -- equality is the bar;
  * the executed reference (tests/golden/retina_ssm.npz) with its recorded picks: decisions exactly, floats to 1e-5 / 1e-3 (torch's
    sigmoid and exp), the tolerances of test_retina_kernels_match_the_reference_method_body.
"""
import ctypes as C
import random

import numpy as np
import pytest

import _retina_ssm_restatement as R
from test_gpu_tail_edges import gpu_retina

F32 = np.float32
TAKE = R.TAKE
pytestmark = pytest.mark.gpu
TINY = ((5, 7), (3, 4), (2, 2), (1, 1), (1, 1))            # 53 pixels, 477 anchors at A = 9, padded input 40 x 56
TINY_PAD = (40, 56)
MID = ((8, 8), (4, 4), (2, 2), (1, 1), (1, 1))             # 86 pixels, 774 anchors: level 0 ends at 576, past two 256-anchor blocks
MID_PAD = (64, 64)


@pytest.fixture(scope="module")
def orc(oracle):
    y = oracle.exp_array(np.array([0.0], F32))
    assert y[0] == F32(1.0)                                  # sigmoid(0) is then exactly 0.5
    return oracle


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


class Picker:
    """A cald_ssm_pick_fn over `fn(image, counts) -> per-class pick lists`; keeps what it was asked.  A class's entry may be (n, list): an n_picks that is not the list's length."""

    def __init__(self, ffi, fn, ret=0):
        self.calls, self.fn, self.ret = [], fn, ret
        self.cb = ffi.PICK_FN(self._call)
        self.ptr = C.cast(self.cb, C.c_void_p)

    def _call(self, user, image, K, counts, picks, n_picks):
        cn = [counts[k] for k in range(K)]
        self.calls.append((image, cn))
        out = self.fn(image, cn)
        for k in range(K):
            n_picks[k] = out[k][0] if isinstance(out[k], tuple) else len(out[k])      # (n, list): an n_picks that is not the list's length
            for j, p in enumerate(out[k][1] if isinstance(out[k], tuple) else out[k]):
                picks[k * TAKE + j] = int(p)
        return self.ret


def identity(image, counts):
    return [list(range(min(n, TAKE))) for n in counts]


def split_levels(flat, level_hw, per_pixel):
    out, off = [], 0
    for h, w in level_hw:
        out.append(np.ascontiguousarray(flat[off:off + h * w * 9].reshape(h, w, 9 * per_pixel), F32)); off += h * w * 9
    assert off == flat.shape[0]
    return out


def gpu_rssm(hip, cls, reg, base, K, sizes, orig, per_class, picker, score_thr=0.05, nms_thr=0.5, A=9):
    ffi, L = hip["ffi"], hip["L"]
    cls = [np.ascontiguousarray(c, F32) for c in cls]; reg = [np.ascontiguousarray(r, F32) for r in reg]
    base = np.ascontiguousarray(base, F32)
    hw = np.array([v for c in cls for v in c.shape[:2]], np.int32)
    cp = (ffi.c_f * 5)(*[ffi.ptr(c) for c in cls]); rp = (ffi.c_f * 5)(*[ffi.ptr(r) for r in reg])
    cap = K * per_class
    boxes = np.full((cap, 4), np.nan, F32); scores = np.full(cap, np.nan, F32); labels = np.full((cap, K - 1), 99, np.int8)
    counts = np.full(K, -7, np.int32); al, n = C.c_int(-1), C.c_int(-1)
    Hp, Wp, Hr, Wr = sizes
    ffi.check(L.cald_op_retina_ssm_postprocess(hip["ctx"], cp, rp, ffi.ptr(hw, ffi.c_i), A, K, ffi.ptr(base), Hp, Wp, Hr, Wr, orig[0], orig[1],
                                               score_thr, nms_thr, per_class, picker.ptr, None, C.byref(al), C.byref(n), ffi.ptr(counts, ffi.c_i),
                                               ffi.ptr(boxes), ffi.ptr(scores), ffi.ptr(labels, ffi.c_i8)))
    m = n.value
    assert 0 <= m <= cap and np.isnan(boxes[m:]).all() and np.isnan(scores[m:]).all() and (labels[m:] == 99).all()      # nothing past the count
    return dict(al=al.value, counts=counts.astype(np.int64), boxes=boxes[:m], scores=scores[:m], labels=labels[:m])


def int_base(seed, A=9):
    """[5][A][4] integer anchors centred on the pixel's corner, sides 6 .. 40."""
    rs = np.random.RandomState(seed)
    w = rs.randint(3, 21, (5, A)) * 2; h = rs.randint(3, 21, (5, A)) * 2
    return np.stack([-w / 2, -h / 2, w / 2, h / 2], -1).astype(F32)


def restate(orc, logits, base, level_hw, sizes, orig, picks, per_class, score_thr=0.05):
    """The restatement on zero deltas (decoded boxes = clipped anchors) and the oracle's exponential."""
    Hp, Wp, Hr, Wr = sizes
    anchors = R.grid_anchors(base, level_hw, Hp, Wp)
    dec = R.decode(np.zeros_like(anchors), anchors, Hr, Wr, exp=orc.exp_array)
    want = R.tail(R.scores_of(logits, exp=orc.exp_array), dec, picks, Hr, Wr, orig[0], orig[1], score_thr=score_thr, per_class=per_class)
    m = want["margins"]["iou"]
    assert m == 0.0 or m > 1e-6, m                  # 1 / 2 itself is not above the threshold, exactly; anything else is far from it
    return want


def run_int_case(hip, orc, logits, base, level_hw, sizes, orig, pick_fn, per_class=50, score_thr=0.05):
    """(hook result, restatement, the picker) of one zero-delta case; pick_fn(image, counts) -> per-class lists."""
    K = logits.shape[1]
    picker = Picker(hip["ffi"], pick_fn)
    cls = split_levels(logits, level_hw, K)
    reg = [np.zeros(c.shape[:2] + (36,), F32) for c in cls]
    got = gpu_rssm(hip, cls, reg, base, K, sizes, orig, per_class, picker, score_thr=score_thr)
    used = picker.calls[0][1] if picker.calls else None
    want = restate(orc, logits, base, level_hw, sizes, orig, (lambda k, n: pick_fn(0, used)[k]) if used is not None else (lambda k, n: []), per_class, score_thr)
    return got, want, picker


def assert_same(got, want, what):
    assert got["al"] == want["al"], what
    assert np.array_equal(got["counts"], want["counts"] if want["al"] == 0 else np.zeros_like(got["counts"])), (what, got["counts"], want["counts"])
    for k in ("boxes", "scores", "labels"):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def n_anchors(level_hw):
    return sum(h * w for h, w in level_hw) * 9


# ---------------------------------------------------------------------------------------------------------------------------
# identity picks: the stock tail
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,per_class", [(4, 50), (21, 50), (4, 300)])
def test_identity_picks_equal_the_stock_tail(hip, orc, K, per_class):
    """Every n_c <= 500 (477 anchors), picks 0 .. n_c - 1, the same thresholds: boxes and scores equal cald_op_retina_postprocess's row for
    row and bit for bit (random deltas, an original size unlike the resized one), labels equal scores_cls[:, 1:] > 0.5."""
    rs = np.random.RandomState(100 + K)
    N = n_anchors(TINY)
    logits = (rs.randn(N, K) * 2.0 - 1.5).astype(F32)
    logits[rs.randint(N), 1] = 3.0
    s = R.scores_of(logits, exp=orc.exp_array)
    for k in range(K):                                       # no exact ties among a class's candidates
        c = s[s[:, k] > F32(0.05), k]
        assert np.unique(c).size == c.size
    deltas = (rs.randn(N, 4) * 0.4).astype(F32)
    base = np.stack([orc.base_anchors([8 * 2 ** l, 10 * 2 ** l, 13 * 2 ** l], [0.5, 1.0, 2.0]) for l in range(5)]).astype(F32)
    cls, reg = split_levels(logits, TINY, K), split_levels(deltas, TINY, 4)
    sizes, orig = TINY_PAD + (37, 50), (111, 163)
    picker = Picker(hip["ffi"], identity)
    got = gpu_rssm(hip, cls, reg, base, K, sizes, orig, per_class, picker)
    stock = gpu_retina(hip, cls, reg, base, K, 9, sizes, orig, per_class)
    assert got["al"] == 0 and len(picker.calls) == 1 and picker.calls[0][0] == 0
    assert np.array_equal(got["counts"], (s > F32(0.05)).sum(0)) and got["counts"].max() <= TAKE
    assert len(stock["boxes"]) > K and got["boxes"].tobytes() == stock["boxes"].tobytes() and got["scores"].tobytes() == stock["scores"].tobytes()
    assert np.array_equal(got["labels"], np.where(stock["scores_cls"][:, 1:] > F32(0.5), 1, -1))
    assert (got["labels"] == 1).any() and (got["labels"] == -1).any()


# ---------------------------------------------------------------------------------------------------------------------------
# other picks: the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def recorded_picks(seed):
    """Reversed lists for even classes, a seeded permutation for odd ones, every third class only the first half of it."""
    def fn(image, counts):
        out = []
        for k, n in enumerate(counts):
            p = list(range(n))[::-1] if k % 2 == 0 else np.random.RandomState(seed + k).permutation(n).tolist()
            p = p[:TAKE]
            out.append(p[:max(1, len(p) // 2)] if k % 3 == 2 else p)
        return out
    return fn


@pytest.mark.parametrize("K,seed", [(4, 1), (21, 2)])
def test_reversed_and_random_picks_equal_the_restatement(hip, orc, K, seed):
    rs = np.random.RandomState(seed)
    N = n_anchors(TINY)
    logits = (rs.randn(N, K) * 2.0 - 1.0).astype(F32)
    logits[rs.randint(N), 0] = 2.5
    got, want, _ = run_int_case(hip, orc, logits, int_base(seed), TINY, TINY_PAD + (36, 50), (90, 101), recorded_picks(seed))
    assert want["al"] == 0 and len(want["boxes"]) > K and len(set(want["cls"].tolist())) == K
    assert_same(got, want, "K %d" % K)


def rank_logits(rank):
    """distinct, well separated scores above 0.05: logit 3.5 - rank / 256 (rank < 1 500)"""
    return (3.5 - np.asarray(rank) / 256.0).astype(F32)


def test_counts_of_0_1_500_and_501(hip, orc):
    """K = 5 on 774 anchors: class 0 has one candidate, class 1 none (in the middle), class 2 exactly 500, class 3 501 (the shuffle drops
    one), class 4 a few; shuffled picks.  The resized image is smaller than the padded one: picked boxes that the clip leaves without
    width or height use up their pick and give no row."""
    rs = np.random.RandomState(11)
    N = n_anchors(MID)
    logits = np.full((N, 5), -10.0, F32)
    logits[rs.randint(N), 0] = 1.0
    for k, n in ((2, 500), (3, 501), (4, 40)):
        idx = rs.permutation(N)[:n]
        logits[idx, k] = rank_logits(rs.permutation(n))

    def shuffled(image, counts):
        rng = random.Random(5)
        out = []
        for n in counts:
            x = list(range(n)); rng.shuffle(x); out.append(x[:TAKE])
        return out
    got, want, picker = run_int_case(hip, orc, logits, int_base(3), MID, MID_PAD + (44, 40), (88, 100), shuffled)
    assert picker.calls == [(0, [1, 0, 500, 501, 40])]
    assert want["counts"].tolist() == [1, 0, 500, 501, 40] and set(want["cls"].tolist()) == {0, 2, 3, 4}
    assert_same(got, want, "counts 0 / 1 / 500 / 501")


def test_more_than_8192_candidates_all_tied(hip, orc):
    """256 x 256: 12 276 anchors, K = 2, every logit 0: both classes list every anchor (48 blocks of 256, scanned across blocks), every
    score is 0.5 (al = 0) and tied, so the earlier of two overlapping picks wins; 500 picks spread over the whole list."""
    level_hw = ((32, 32), (16, 16), (8, 8), (4, 4), (2, 2))
    N = n_anchors(level_hw)
    assert N == 12276
    base = np.stack([orc.base_anchors(list(s), [0.5, 1.0, 2.0]) for s in orc.retina_anchor_sizes()]).astype(F32)

    def spread(image, counts):
        return [np.random.RandomState(40 + k).permutation(n)[:TAKE].tolist() for k, n in enumerate(counts)]
    got, want, picker = run_int_case(hip, orc, np.zeros((N, 2), F32), base, level_hw, (256, 256, 240, 250), (480, 1000), spread, per_class=300)
    assert picker.calls == [(0, [N, N])] and want["al"] == 0 and (want["scores"] == F32(0.5)).all() and (want["labels"] == -1).all()
    assert len(want["boxes"]) > 100
    assert_same(got, want, "12 276 tied candidates")


def test_the_list_is_ordered_across_blocks_and_levels(hip, orc):
    """The same twelve candidates in each of twelve classes -- on both sides of the 256-anchor block boundaries (255 | 256, 511 | 512), of
    the level boundaries (575 | 576, 719 | 720) and at both ends; class k picks position k alone, so row k is the k-th candidate's box."""
    cand = [0, 254, 255, 256, 257, 511, 512, 575, 576, 719, 720, 773]
    K = len(cand)
    N = n_anchors(MID)
    logits = np.full((N, K), -10.0, F32)
    logits[cand] = 1.0
    got, want, picker = run_int_case(hip, orc, logits, int_base(10), MID, MID_PAD + (64, 64), (64, 64), lambda image, counts: [[k] for k in range(len(counts))])
    assert picker.calls == [(0, [K] * K)]
    assert want["anchor"].tolist() == cand and want["cls"].tolist() == list(range(K))
    assert len(np.unique(want["boxes"], axis=0)) == K          # the boxes tell the candidates apart
    assert_same(got, want, "ordered list")


def test_a_picked_small_box_takes_a_slot_and_gives_no_row(hip, orc):
    """A = 9 anchors at pixel (0, 7) of level 0 start at x = 56 - w / 2 >= 36: clipped to a resized width of 30 they have no width.  Class 1
    holds three of them and three ordinary ones; all six are picked, three rows come out."""
    N = n_anchors(MID)
    logits = np.full((N, 2), -10.0, F32)
    small = [7 * 9 + a for a in (0, 1, 2)]; fine = [(2 * 8 + 1) * 9, (5 * 8 + 2) * 9 + 3, 576 + 9]
    logits[small, 1] = [3.0, 2.0, 1.0]; logits[fine, 1] = [2.5, 1.5, 0.5]
    got, want, picker = run_int_case(hip, orc, logits, int_base(4), MID, MID_PAD + (64, 30), (64, 30), identity)
    assert picker.calls == [(0, [0, 6])] and want["counts"].tolist() == [0, 6]
    assert len(want["boxes"]) <= 3 and len(want["boxes"]) >= 1 and not set(want["anchor"].tolist()) & set(small)
    assert_same(got, want, "small boxes")


def test_more_survivors_than_per_class(hip, orc):
    """Level 0's 64 pixels, anchor 0 of each (8 x 8 boxes on a stride of 8: disjoint), distinct scores: the first per_class by score stay."""
    N = n_anchors(MID)
    base = int_base(1); base[0, 0] = [-4, -4, 4, 4]
    pix = np.arange(64)
    ok = ((pix // 8) > 0) & ((pix % 8) > 0)                    # away from the clipped border
    idx = pix[ok] * 9
    logits = np.full((N, 2), -10.0, F32)
    logits[idx, 1] = rank_logits(np.random.RandomState(2).permutation(idx.size))
    for per in (1, 7, 48, 49, 50):
        got, want, _ = run_int_case(hip, orc, logits, base, MID, MID_PAD + (64, 64), (64, 64), recorded_picks(7), per_class=per)
        assert want["counts"].tolist() == [0, 49] and len(want["boxes"]) == min(per, 49)
        assert_same(got, want, "per_class %d" % per)


def test_exact_score_ties_go_to_the_earlier_pick(hip, orc):
    """Two nested anchors of one pixel with the same logit (IoU 3 / 4): with identity picks the lower anchor stays, with reversed picks
    the higher one -- the candidate earlier in the shuffled list."""
    N = n_anchors(MID)
    base = int_base(1); base[0, 0] = [-8, -8, 8, 8]; base[0, 1] = [-8, -8, 8, 4]
    a0 = (3 * 8 + 3) * 9
    logits = np.full((N, 2), -10.0, F32)
    logits[[a0, a0 + 1], 1] = 1.0
    for fn, winner in ((identity, a0), (lambda image, counts: [list(range(n))[::-1] for n in counts], a0 + 1)):
        got, want, _ = run_int_case(hip, orc, logits, base, MID, MID_PAD + (64, 64), (64, 64), fn)
        assert want["anchor"].tolist() == [winner]
        assert_same(got, want, "tie, winner %d" % winner)


def test_a_score_of_exactly_the_threshold_is_no_candidate(hip, orc):
    """score_thr = 0.5 and logits of exactly 0: `>` leaves them out; the one logit above 0 is the only candidate."""
    N = n_anchors(TINY)
    logits = np.full((N, 3), -10.0, F32)
    logits[[5, 100, 300], 1] = 0.0; logits[200, 1] = 0.5; logits[7, 2] = 0.0
    got, want, picker = run_int_case(hip, orc, logits, int_base(2), TINY, TINY_PAD + (40, 56), (40, 56), identity, score_thr=0.5)
    assert picker.calls == [(0, [0, 1, 0])] and want["anchor"].tolist() == [200]
    assert_same(got, want, "score == threshold")


def al_case(top_logit):
    N = n_anchors(TINY)
    logits = np.full((N, 4), -2.0, F32)                      # scores of 0.119 everywhere: candidates of every class
    logits[123, 0] = top_logit
    return logits


def test_largest_score_exactly_one_half_in_class_0_only(hip, orc):
    """logit 0 in class 0: the maximum over ALL classes is 0.5, not below it: al = 0, and no score of classes 1..K-1 is above 0.5."""
    logits = al_case(0.0)
    assert R.scores_of(logits, exp=orc.exp_array).max() == F32(0.5)
    got, want, picker = run_int_case(hip, orc, logits, int_base(5), TINY, TINY_PAD + (40, 56), (40, 56), recorded_picks(3))
    assert want["al"] == 0 and len(picker.calls) == 1 and len(want["boxes"]) > 4 and (want["labels"] == -1).all()
    assert_same(got, want, "al at 0.5")


def test_largest_score_just_below_one_half_is_an_al_image(hip, orc):
    """The largest float32 below 0.5 that this sigmoid produces (1 + exp(-x) steps by 2^-22 at 2, so it lies two units in the last place
    below, at logit -2^-22): al = 1, no rows, counts zero, and the callback is not asked."""
    logits = al_case(-2.0 ** -22)
    top = R.scores_of(logits, exp=orc.exp_array).max()
    assert top < F32(0.5) and F32(0.5) - top <= F32(2.0 ** -24)
    assert R.scores_of(al_case(-2.0 ** -23), exp=orc.exp_array).max() == F32(0.5)       # half that logit already rounds to 0.5
    got, want, picker = run_int_case(hip, orc, logits, int_base(5), TINY, TINY_PAD + (40, 56), (40, 56), identity)
    assert want["al"] == 1 and picker.calls == [] and got["al"] == 1 and len(got["boxes"]) == 0 and (got["counts"] == 0).all()
    assert_same(got, want, "al just below 0.5")


# ---------------------------------------------------------------------------------------------------------------------------
# bad picks and arguments: CALD_ERR_INVALID from the host checks, before phase B is launched
# ---------------------------------------------------------------------------------------------------------------------------
def test_bad_picks_and_arguments_are_refused(hip, orc):
    ffi, L = hip["ffi"], hip["L"]
    N, K = n_anchors(TINY), 3
    logits = np.full((N, K), -10.0, F32)
    logits[[10, 20, 30, 40], 1] = [2.0, 1.5, 1.0, 0.5]; logits[50, 2] = 1.0            # counts [0, 4, 1]
    cls = split_levels(logits, TINY, K); reg = [np.zeros(c.shape[:2] + (36,), F32) for c in cls]
    base = int_base(6)
    hw = np.array([v for c in cls for v in c.shape[:2]], np.int32)
    cp = (ffi.c_f * 5)(*[ffi.ptr(c) for c in cls]); rp = (ffi.c_f * 5)(*[ffi.ptr(r) for r in reg])
    boxes = np.zeros((K * 50, 4), F32); scores = np.zeros(K * 50, F32); labels = np.zeros((K * 50, K - 1), np.int8)
    counts = np.zeros(K, np.int32); al, n = C.c_int(), C.c_int()

    def call(picker, K_=K, cls_=cp, al_=None, pick_=None):
        return L.cald_op_retina_ssm_postprocess(hip["ctx"], cls_, rp, ffi.ptr(hw, ffi.c_i), 9, K_, ffi.ptr(base), 40, 56, 40, 56, 40, 56, 0.05, 0.5, 50,
                                                picker.ptr if pick_ is None else pick_, None, C.byref(al) if al_ is None else al_, C.byref(n),
                                                ffi.ptr(counts, ffi.c_i), ffi.ptr(boxes), ffi.ptr(scores), ffi.ptr(labels, ffi.c_i8))
    good = Picker(ffi, identity)
    assert call(good) == 0 and n.value == 5 and counts.tolist() == [0, 4, 1]
    for what, fn, ret, text in (("out of range", lambda i, c: [[], [0, 4], [0]], 0, "image 0 class 1: pick 1 is 4"),
                                ("negative", lambda i, c: [[], [0, 1], [-1]], 0, "image 0 class 2: pick 0 is -1"),
                                ("n_picks above the count", lambda i, c: [[], (5, [0, 1, 2, 3]), [0]], 0, "image 0 class 1: 5 picks of 4"),
                                ("picks for an empty class", lambda i, c: [(1, [0]), [0], [0]], 0, "image 0 class 0: 1 picks of 0"),
                                ("negative n_picks", lambda i, c: [[], (-1, []), [0]], 0, "image 0 class 1: -1 picks"),
                                ("callback says no", identity, 7, "returned 7 for image 0")):
        assert call(Picker(ffi, fn, ret)) == -1, what
        assert text in L.cald_last_error().decode(), (what, L.cald_last_error().decode())
    assert call(good, pick_=C.c_void_p(None)) == -1 and call(good, al_=C.POINTER(C.c_int)()) == -1 and call(good, cls_=None) == -1
    assert call(good, K_=1) == -1 and "K >= 2" in L.cald_last_error().decode()
    assert call(good) == 0 and n.value == 5                   # and the context is as good as before


def test_a_faster_rcnn_model_is_refused_by_the_retinanet_sweep(hip):
    from cald_amd import ssm, synth
    from cald_amd.baselines import _arrays
    ffi, L, torch = hip["ffi"], hip["L"], hip["torch"]
    model = ssm.fasterrcnn_resnet50_fpn_ssm(num_classes=21, min_size=300, max_size=500)
    model.to("cuda").load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0))
    dev = [torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda")]
    ptrs, Hs, Ws = _arrays(dev)
    al = np.zeros(1, np.int32); cnt = np.zeros(1, np.int32); boxes = np.zeros((8, 4), F32); scores = np.zeros(8, F32); labels = np.zeros((8, 20), np.int8)
    need = C.c_int64(-1)
    picker = Picker(ffi, identity)
    rc = L.cald_sweep_ssm_retina(model.handle(), 1, ptrs, ffi.ptr(Hs, ffi.c_i), ffi.ptr(Ws, ffi.c_i), 1, picker.ptr, None, 8, ffi.ptr(al, ffi.c_i),
                                 ffi.ptr(cnt, ffi.c_i), ffi.ptr(boxes), ffi.ptr(scores), ffi.ptr(labels, ffi.c_i8), C.byref(need))
    assert rc == -1 and "RetinaNet only" in L.cald_last_error().decode() and picker.calls == []


# ---------------------------------------------------------------------------------------------------------------------------
# the executed reference
# ---------------------------------------------------------------------------------------------------------------------------
def test_hook_matches_the_executed_reference_tail(hip, golden):
    """tests/golden/retina_ssm.npz (the reference's own ssm_postprocess_detections; torch's sigmoid and exp), its recorded picks replayed:
    al, the per-class counts, the row count and the labels exactly, scores to 1e-5 and boxes to 1e-3."""
    fx = golden("retina_ssm")
    for c in range(int(fx["n"])):
        K = int(fx["c%d_K" % c]); Hp, Wp, Hr, Wr = [int(v) for v in fx["c%d_sizes" % c]]
        picks = R.unpack_picks(fx["c%d_picks" % c], fx["c%d_n_picks" % c])
        picker = Picker(hip["ffi"], lambda image, counts, picks=picks: [p.tolist() for p in picks])
        got = gpu_rssm(hip, [fx["c%d_cls%d" % (c, l)] for l in range(5)], [fx["c%d_reg%d" % (c, l)] for l in range(5)], fx["base"], K,
                       (Hp, Wp, Hr, Wr), (Hr, Wr), int(fx["c%d_per" % c]), picker, score_thr=float(fx["c%d_thr" % c]))
        name = str(fx["names"][c])
        assert got["al"] == int(fx["c%d_al" % c]) and np.array_equal(got["counts"], fx["c%d_counts" % c]), name
        assert len(picker.calls) == (0 if got["al"] else 1)
        assert got["boxes"].shape == fx["c%d_boxes" % c].shape and np.array_equal(got["labels"], fx["c%d_labels" % c]), name
        assert np.abs(got["scores"] - fx["c%d_scores" % c]).max(initial=0.0) <= 1e-5
        assert np.abs(got["boxes"] - fx["c%d_boxes" % c]).max(initial=0.0) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the forward: cald_sweep_ssm_retina on the small model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rssm_model(hip, orc):
    """The 300 / 500 RetinaNet of the parity tests (synth.pseudo_trained_retinanet) as an SSM detector, its classification bias raised by 2
    so that the three pool images score above 0.5 somewhere (al = 0, many classes past 500 candidates) while a flat grey image stays
    below (al = 1: 0.03 before, 0.19 after); four images of three sizes, the grey one second."""
    from cald_amd import ssm, synth
    torch = hip["torch"]
    sd = dict(synth.pseudo_trained_retinanet(21, 50, seed=0))
    sd["head.classification_head.cls_logits.bias"] = np.asarray(sd["head.classification_head.cls_logits.bias"], F32) + F32(2.0)
    model = ssm.retinanet_resnet50_fpn_ssm(num_classes=21, min_size=300, max_size=500)
    model.to("cuda").load_state_dict(sd)
    model.eval()
    pool = synth.make_pool(3, "voc", 0, scale=0.5)
    imgs = [pool[0], np.full((160, 200, 3), 128, np.uint8), pool[1], np.ascontiguousarray(pool[2][:200, :150])]
    return model, imgs, [torch.from_numpy(im).cuda() for im in imgs]


def _sweep(model, dev, batch, seed=17):
    from cald_amd import ssm
    random.seed(seed)
    out = ssm.ssm_sweep_device_images(model, dev, batch_images=batch)
    return out, random.getstate()


def _raw_sweep(hip, model, dev, batch, picker, cap):
    from cald_amd.baselines import _arrays
    ffi, L = hip["ffi"], hip["L"]
    n = len(dev)
    ptrs, Hs, Ws = _arrays(dev)
    al = np.zeros(n, np.int32); cnt = np.zeros(n, np.int32)
    boxes = np.zeros((cap, 4), F32); scores = np.zeros(cap, F32); labels = np.zeros((cap, 20), np.int8); need = C.c_int64(-1)
    rc = L.cald_sweep_ssm_retina(model.handle(), n, ptrs, ffi.ptr(Hs, ffi.c_i), ffi.ptr(Ws, ffi.c_i), batch, picker.ptr, None, cap, ffi.ptr(al, ffi.c_i),
                                 ffi.ptr(cnt, ffi.c_i), ffi.ptr(boxes), ffi.ptr(scores), ffi.ptr(labels, ffi.c_i8), C.byref(need))
    return rc, need.value, al, cnt, boxes, scores, labels


def seeded_picks(image, counts):
    rng = random.Random(1000 + image)
    out = []
    for n in counts:
        x = list(range(n)); rng.shuffle(x); out.append(x[:TAKE])
    return out


def test_sweep_equals_the_hook_on_the_forwards_own_tensors(hip, orc, rssm_model):
    from cald_amd import train_ops
    model, imgs, dev = rssm_model
    picker = Picker(hip["ffi"], seeded_picks)
    rc, need, al, cnt, boxes, scores, labels = _raw_sweep(hip, model, dev, 4, picker, 4 * 21 * 50)
    assert rc == 0 and need == cnt.sum() and al.tolist() == [0, 1, 0, 0] and cnt[1] == 0 and (cnt[[0, 2, 3]] > 0).all()
    assert [c[0] for c in picker.calls] == [0, 2, 3]                       # one call per al = 0 image, in image order
    assert max(max(c[1]) for c in picker.calls) > TAKE
    print("candidates per image and class:", [c[1] for c in picker.calls])
    base = np.stack([orc.base_anchors(list(s), [0.5, 1.0, 2.0]) for s in orc.retina_anchor_sizes()]).astype(F32)
    off = np.concatenate([[0], np.cumsum(cnt)])
    for v, im in enumerate(imgs):                      # the debug tensors are those of the last forward: all four views in one batch
        Hr, Wr, Hp, Wp = train_ops.transform_size(im.shape[0], im.shape[1], 300, 500)
        cls = [model.debug_tensor("cls%d" % l, v) for l in range(5)]; reg = [model.debug_tensor("reg%d" % l, v) for l in range(5)]
        replay = Picker(hip["ffi"], lambda image, counts, v=v: seeded_picks(v, counts))
        want = gpu_rssm(hip, cls, reg, base, 21, (Hp, Wp, Hr, Wr), im.shape[:2], 50, replay)
        assert want["al"] == al[v] and len(want["boxes"]) == cnt[v]
        if al[v] == 0:
            assert replay.calls[0][1] == [c for c in picker.calls if c[0] == v][0][1]
        got = dict(boxes=boxes[off[v]:off[v + 1]], scores=scores[off[v]:off[v + 1]], labels=labels[off[v]:off[v + 1]])
        for k in got:
            assert got[k].tobytes() == want[k].tobytes(), (v, k)


def test_sweep_does_not_depend_on_the_batch_and_repeats_its_bytes(hip, rssm_model):
    model, _, dev = rssm_model
    runs = [_sweep(model, dev, 4), _sweep(model, dev, 4), _sweep(model, dev, 1)]
    assert runs[0][0][1].sum() > 0 and runs[0][0][3].ndim == 1 and runs[0][0][4].shape == (runs[0][0][1].sum(), 20)
    for r, state in runs[1:]:
        assert state == runs[0][1]
        for a, b in zip(runs[0][0], r):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_sweep_reports_the_rows_it_needs(hip, rssm_model):
    L = hip["L"]
    model, _, dev = rssm_model
    picker = Picker(hip["ffi"], seeded_picks)
    rc, total, al, cnt, _, _, _ = _raw_sweep(hip, model, dev, 2, picker, 4 * 21 * 50)
    assert rc == 0 and total == cnt.sum() > 1
    rc, need, al2, cnt2, _, _, _ = _raw_sweep(hip, model, dev, 2, picker, total - 1)
    assert rc == -1 and need == total and ("needs %d rows" % total) in L.cald_last_error().decode()
    assert np.array_equal(al2, al) and np.array_equal(cnt2, cnt)
    rc, need, _, _, _, _, _ = _raw_sweep(hip, model, dev, 2, picker, total)
    assert rc == 0 and need == total


def test_c_pick_and_python_pick_sweep_alike(hip, rssm_model, monkeypatch):
    from cald_amd import ssm
    model, _, dev = rssm_model
    monkeypatch.delenv("CALD_SSM_PICK", raising=False)
    assert ssm._c_pick_checked()
    c_run, c_state = _sweep(model, dev, 4, seed=23)
    monkeypatch.setenv("CALD_SSM_PICK", "python")
    p_run, p_state = _sweep(model, dev, 4, seed=23)
    assert c_state == p_state and c_state != random.Random(23).getstate()          # both drew, and the same amount
    for a, b in zip(c_run, p_run):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    other, _ = _sweep(model, dev, 4, seed=24)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(c_run, other))            # the picks matter: another seed, other rows


def test_an_al_image_between_two_others_draws_nothing(hip, rssm_model):
    model, _, dev = rssm_model
    (al, cnt, boxes, scores, labels), state = _sweep(model, [dev[0], dev[1], dev[2]], 3, seed=31)
    (al2, cnt2, boxes2, scores2, labels2), state2 = _sweep(model, [dev[0], dev[2]], 2, seed=31)
    assert al.tolist() == [0, 1, 0] and al2.tolist() == [0, 0] and cnt[1] == 0 and cnt[[0, 2]].tolist() == cnt2.tolist()
    assert state == state2
    assert boxes.tobytes() == boxes2.tobytes() and scores.tobytes() == scores2.tobytes() and labels.tobytes() == labels2.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# cald_amd/ssm.py end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_get_uncertainty_returns_the_references_types(hip, rssm_model):
    from cald_amd import ssm
    torch = hip["torch"]
    model, imgs, dev = rssm_model
    loader = [([torch.from_numpy(im).permute(2, 0, 1).float().div(255)], [{}]) for im in imgs]       # to_tensor's float CHW, one image an item
    random.seed(41)
    allScore, allBox, allY, al_idx = ssm.get_uncertainty(model, loader)
    (al, cnt, boxes, scores, labels), _ = _sweep(model, dev, 4, seed=41)
    kept = [i for i in range(4) if al[i] == 0]
    assert al_idx == [1] and len(allScore) == len(allBox) == len(allY) == 3
    off = np.concatenate([[0], np.cumsum(cnt)])
    for j, i in enumerate(kept):
        assert allScore[j].is_cuda and allScore[j].dtype == torch.float32 and tuple(allScore[j].shape) == (cnt[i],)          # 1-D
        assert allBox[j].is_cuda and tuple(allBox[j].shape) == (cnt[i], 4)
        assert isinstance(allY[j], list) and len(allY[j]) == cnt[i] and all(isinstance(y, list) and len(y) == 20 and set(y) <= {1, -1} for y in allY[j])
        assert allScore[j].cpu().numpy().tobytes() == scores[off[i]:off[i + 1]].tobytes() and allBox[j].cpu().numpy().tobytes() == boxes[off[i]:off[i + 1]].tobytes()
        assert np.array_equal(np.array(allY[j], np.int8), labels[off[i]:off[i + 1]])
    random.seed(41)
    det = model([loader[0][0][0]])[0]                            # ssm_mode(True) is still on: the reference's dict
    assert set(det) == {"boxes", "scores", "labels", "al"} and det["al"] == 0 and det["scores"].dim() == 1 and torch.equal(det["scores"], allScore[0])
    assert model([loader[1][0][0]])[0]["al"] == 1
    with pytest.raises(ValueError):
        ssm.get_uncertainty(model, [([loader[0][0][0], loader[1][0][0]], [{}, {}])])
    loss = ssm.box_loss(allScore[0][0].cpu().numpy(), np.asarray(allY[0][0], np.int64))                # stage 2's line on the sweep's own types
    assert loss.shape == (20,)


def test_image_cross_validation_end_to_end_on_one_candidate(hip, rssm_model):
    """ssm_mode(False) gives the stock RetinaNet tail (labels 0 .. K-1, 50 per class), which image_cross_validation reads."""
    from cald_amd import ssm
    torch = hip["torch"]
    model, imgs, dev = rssm_model
    random.seed(43)
    _, allBox, _, _ = ssm.get_uncertainty(model, [([dev[0]], [{}])])

    def crop(b):
        return dev[0][int(b[0]):int(b[2]), int(b[1]):int(b[3])]
    fits = [b for b in allBox[0] if 0 < crop(b).shape[0] <= 187 and 0 < crop(b).shape[1] <= 150]
    box = fits[0] if fits else torch.tensor([12.6, 20.2, 70.9, 95.5])
    labeled = [([dev[2]], [{"labels": torch.tensor([1, 2])}]), ([dev[3]], [{"labels": torch.tensor([4])}])]
    random.seed(77)
    flag, score = ssm.image_cross_validation(model, [([dev[0]], [{}])], labeled, box, torch.tensor([3]))
    assert flag is False and score == 0 and model._ssm is False       # two images can never give more than 2.5 confirmations
    assert random.getstate() != random.Random(77).getstate()         # both pastes drew their place
    res = model([dev[0]])[0]                                          # the stock dict
    assert {"boxes", "labels", "scores", "scores_cls", "prob_max"} <= set(res) and res["labels"].dtype == torch.int64 and res["scores"].dim() == 1
    assert int(torch.bincount(res["labels"], minlength=21).max()) <= 50
