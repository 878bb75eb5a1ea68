"""GPU tests of the training front end, target and loss kernels at their edges: train_ops.preprocess / maxpool / subsample2 (train_conv.hip
over elementwise.hip's kernels), match, anchors, box_encode, roi_gather (train_targets.hip) and the plain focal loss (train_loss.hip)
against the restatements and case tables of tests/_train_edges_restatement.py, which tests/test_train_edges.py pins to live torch and to the
recorded reference and whose census it takes on the CPU.  Integer and copy results, the pools, preprocess and the focal gradient cross-check
are exact; BoxCoder.encode is held to 1e-6 of the largest entry and the focal loss to 2e-6 (value) / 1e-5 (gradient), the bounds
test_gpu_train.py states for the same operators.  Each test names the one-line kernel mistake it exists to catch."""
import ctypes as C

import numpy as np
import pytest

import _train_edges_restatement as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    from cald_amd import train_ops
    if not torch.cuda.is_available():      # module-scoped: runs before conftest's function-scoped auto-skip
        pytest.skip("needs an MI355X")
    return torch, train_ops


def _close(got, want, tol, what):
    got = got.detach().double().cpu().numpy() if hasattr(got, "detach") else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if hasattr(want, "detach") else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    scale = max(1e-30, float(np.abs(want).max())) if want.size else 1.0
    err = float(np.abs(got - want).max()) / scale if want.size else 0.0
    print("%s: max err / max|ref| = %.3g" % (what, err))
    assert err <= tol, "%s: max err / max|ref| = %.3g > %.3g" % (what, err, tol)


def _same_but_nan(got, want, what):
    """equal NaN positions, equal bytes everywhere else"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert got[~nan].tobytes() == want[~nan].tobytes(), what


# ---- 1. front end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.POOL_KINDS)
def test_maxpool_and_subsample2_equal_torch_on_small_and_odd_maps(T, kind):
    """max_pool2d(3, 2, 1) and max_pool2d(1, 2, 0) against live torch, bit for bit, on maps of 1 .. 23 pixels a side.  Catches: a border
    padded with 0 instead of -inf (the all-negative input: every output must be negative), a window clipped one pixel short or long on maps
    of one to three pixels, `max` that drops a NaN or a -inf, the output size (H - 1) / 2 + 1 taken as H / 2."""
    torch, ops = T
    for H, W in E.POOL_HW:
        for Cc in E.POOL_C:
            for N in E.POOL_N:
                x = E.pool_input(kind, N, H, W, Cc)
                xd = torch.from_numpy(x).cuda()
                got = ops.maxpool(xd).cpu().numpy()
                _same_but_nan(got, E.pool_ref(x, True), ("maxpool", kind, N, H, W, Cc))
                if kind == "negative":
                    assert got.max() < 0, ("a padded border entered the maximum", N, H, W, Cc)
                _same_but_nan(ops.subsample2(xd).cpu().numpy(), E.pool_ref(x, False), ("subsample2", kind, N, H, W, Cc))


def test_pools_give_each_image_the_result_of_the_image_alone(T):
    """Catches: a window that reads across the seam between two images of the dense batch (the last row of image n - 1 or the first of
    n + 1 instead of the border), an image offset taken from another map's size."""
    torch, ops = T
    for H, W in ((7, 9), (2, 5)):
        x = torch.from_numpy(E.pool_input("gaussian", 3, H, W, 64, seed=5)).cuda()
        for op in (ops.maxpool, ops.subsample2):
            whole = op(x).cpu().numpy()
            for i in range(3):
                assert op(x[i:i + 1].contiguous()).cpu().numpy().tobytes() == whole[i:i + 1].tobytes(), (op.__name__, H, W, i)


def _preprocess_batch(torch, ops, batch, seed=0):
    mn, mx, src, rem_at = batch
    images = E.preprocess_images(src, seed)
    tr = [ops.transform_size(h, w, mn, mx) for h, w in src]
    Hp, Wp = max(t[2] for t in tr), max(t[3] for t in tr)
    rem = None if rem_at is None else [E.preprocess_remainder(*src[i], seed=i) if i == rem_at else None for i in range(len(src))]
    return images, [(t[0], t[1]) for t in tr], Hp, Wp, rem


@pytest.mark.parametrize("batch", E.PREPROCESS_BATCHES, ids=lambda b: "min%d-max%d" % (b[0], b[1]))
def test_preprocess_equals_the_oracle_view_embedded_in_the_padded_batch(T, oracle, batch):
    """Three images of different resized sizes under one padded size, against oracle.preprocess_view bit for bit.  Catches: the resize
    ratio taken from the padded instead of the resized size, a source row or column clamped at H instead of H - 1 (1 x 1 and 2 x 3
    sources), the batch's largest size used for every image, pad pixels or channel 3 left unwritten, the remainder tensor of one image
    added to (or its absence assumed for) its neighbours."""
    torch, ops = T
    images, sizes, Hp, Wp, rem = _preprocess_batch(torch, ops, batch)
    want, want_sizes = E.preprocess_want(oracle, images, batch[0], batch[1], rem, Hp, Wp)
    assert sizes == want_sizes
    got = ops.preprocess([torch.from_numpy(im).cuda() for im in images], sizes, Hp, Wp,
                         remainders=None if rem is None else [None if r is None else torch.from_numpy(r).cuda() for r in rem]).cpu().numpy()
    assert got.shape == (3, Hp, Wp, 4)
    for i, (hr, wr) in enumerate(sizes):
        assert not got[i, hr:].any() and not got[i, :, wr:].any() and not got[i, ..., 3].any(), i
        assert got[i, :hr, :wr, :3].any(), i
    assert got.tobytes() == want.tobytes()


def test_preprocess_writes_every_word_of_its_output_buffer(T, oracle):
    """The C entry point on a buffer filled with a sentinel.  Catches: a grid sized by the resized instead of the padded size (the zero
    border comes from the kernel, not from the allocation), an early return for pixels outside the image."""
    torch, ops = T
    from cald_amd import _ffi
    from cald_amd.detector import get_ctx
    batch = E.PREPROCESS_BATCHES[1]
    images, sizes, Hp, Wp, _ = _preprocess_batch(torch, ops, batch)
    want, _ = E.preprocess_want(oracle, images, batch[0], batch[1], None, Hp, Wp)
    dev = [torch.from_numpy(im).cuda() for im in images]
    out = torch.full((len(images) + 1, Hp, Wp, 4), E.SENTINEL, device="cuda")
    hw = [v for im, (hr, wr) in zip(images, sizes) for v in (im.shape[0], im.shape[1], hr, wr)]
    _ffi.check(_ffi.lib().cald_train_preprocess(get_ctx(0), len(images), ops._ptr_array(dev), None, ops._int_array(hw), Hp, Wp, C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got[:3] == np.float32(E.SENTINEL)).any(), "a word of the output was not written"
    assert got[:3].tobytes() == want.tobytes()
    assert (got[3] == np.float32(E.SENTINEL)).all(), "the call wrote past its [N][Hp][Wp][4] buffer"


def test_preprocess_reads_sources_at_every_byte_alignment(T):
    """Source images whose first byte lies 1, 2 and 3 bytes past a 4-byte boundary give the bits of an aligned copy: the kernel reads the
    aligned dwords that hold a tap's bytes and shifts.  Catches: a shift taken from the pixel instead of the address, the second or third
    dword not read when the six bytes straddle it."""
    torch, ops = T
    for batch in (E.PREPROCESS_BATCHES[1], E.PREPROCESS_BATCHES[0]):
        images, sizes, Hp, Wp, _ = _preprocess_batch(torch, ops, batch, seed=3)
        aligned = [torch.from_numpy(im).cuda() for im in images]
        assert all(t.data_ptr() % 4 == 0 for t in aligned)
        want = ops.preprocess(aligned, sizes, Hp, Wp).cpu().numpy()
        for k in (1, 2, 3):
            held = []
            for im in images:
                buf = torch.zeros(im.size + 16, dtype=torch.uint8, device="cuda")
                v = buf[k:k + im.size].view(im.shape)
                v.copy_(torch.from_numpy(im))
                assert v.data_ptr() % 4 == k and v.is_contiguous()
                held.append(v)
            assert ops.preprocess(held, sizes, Hp, Wp).cpu().numpy().tobytes() == want.tobytes(), k


# ---- 2. matcher --------------------------------------------------------------------------------------------------------------------
def _match(torch, ops, gt, boxes, hi, lo, low):
    return ops.match(torch.from_numpy(boxes).cuda(), torch.from_numpy(gt).cuda(), hi, lo, low).cpu().numpy().astype(np.int64)


def _tt_match(torch, gt, boxes, hi, lo, low):
    from oracle import torch_train as tt
    return tt.matcher(tt.box_iou(torch.from_numpy(gt), torch.from_numpy(boxes)), hi, lo, low).numpy()


def test_match_on_the_designed_table_of_ties_and_exact_thresholds(T):
    """IoUs bit-equal to 0.7, 0.3, 0.5 and 0.4, two identical ground truths, and the stated matches.  Catches: `<=` for `<` at a threshold
    (candidates 1 and 2 at (0.7, 0.3), 3 and 4 at (0.5, 0.4)), `>=` for `>` in the first-maximum rule (candidate 0 would match ground
    truth 1), an IoU computed as inter / (a + b - inter) in another association that moves 70 / 100 off 0.7f."""
    torch, ops = T
    gt, boxes = E.designed_table()
    for (hi, lo, low), want in E.DESIGNED_EXPECT.items():
        assert _match(torch, ops, gt, boxes, hi, lo, low).tolist() == want, (hi, lo, low)


def test_match_keeps_torchvisions_rule_for_a_ground_truth_that_overlaps_nothing(T):
    """A ground truth whose best IoU is 0 "matches" every candidate at IoU 0: all of them get their pre-threshold match back (torchvision
    0.8.2 Matcher.set_low_quality_matches_).  Catches: the rule repaired -- `v > 0` required where a candidate is compared with the ground
    truth's best IoU -- which would leave candidates 2 .. 7 at -2 / -1."""
    torch, ops = T
    gt, boxes = E.designed_table(lonely=True)
    assert _match(torch, ops, gt, boxes, 0.7, 0.3, True).tolist() == E.LONELY_EXPECT
    for extended in (False, True):
        gt, boxes = E.designed_table(extended=extended, lonely=True)
        for hi, lo, low in E.MATCH_MODES:
            assert np.array_equal(_match(torch, ops, gt, boxes, hi, lo, low), _tt_match(torch, gt, boxes, hi, lo, low)), (extended, hi, lo, low)


def test_match_restores_every_candidate_that_shares_a_ground_truths_best_iou(T):
    """The extended table: two candidates share a ground truth's best IoU at 0.4 and two at 0.2, one candidate in the band stays -2.
    Catches: only the first (or last) of the tied candidates restored (an argmax instead of the equality test), the restored value taken
    from the ground truth being compared instead of the candidate's own first maximum, low-quality matches applied with allow_low off."""
    torch, ops = T
    gt, boxes = E.designed_table(extended=True)
    for hi, lo, low in E.MATCH_MODES:
        got = _match(torch, ops, gt, boxes, hi, lo, low)
        assert np.array_equal(got, _tt_match(torch, gt, boxes, hi, lo, low)), (hi, lo, low)
        if low:
            assert got[12:16].tolist() == [3, 3, 4, 4] and got[16] == (-2 if hi == 0.7 else -1) and got[17] == -1, (hi, lo, got)
        else:
            assert (got[12:] < 0).all(), (hi, lo, got)


@pytest.mark.parametrize("n_gt", E.MATCH_N_GT)
def test_match_on_integer_boxes_at_block_boundaries(T, n_gt):
    """Random integer boxes on a 64 x 64 canvas (ties and exact thresholds by construction; the census is test_train_edges.py's) at 1, 255,
    256, 257 and 513 candidates.  Catches: the mistakes above at sizes where a ground truth's best IoU is found in another 256-thread block
    than the candidates that share it (the per-ground-truth maximum not reduced across blocks), a last partial block left unwritten."""
    torch, ops = T
    for n_boxes in E.MATCH_N_BOXES:
        gt, boxes = E.random_match_case(n_boxes, n_gt)
        for hi, lo, low in E.MATCH_MODES:
            assert np.array_equal(_match(torch, ops, gt, boxes, hi, lo, low), _tt_match(torch, gt, boxes, hi, lo, low)), (n_boxes, n_gt, hi, lo, low)


def test_match_writes_its_row_of_a_batch_tensor_only(T):
    """`out=` a row of an [N, n] int32 tensor, as the trainers pass it.  Catches: a store past n (a grid rounded up to 256 without the
    bound), a row offset applied twice."""
    torch, ops = T
    for n_boxes in (255, 257):
        gt, boxes = E.random_match_case(n_boxes, 3)
        out = torch.full((3, n_boxes), -77, dtype=torch.int32, device="cuda")
        ops.match(torch.from_numpy(boxes).cuda(), torch.from_numpy(gt).cuda(), 0.5, 0.4, True, out=out[1])
        got = out.cpu().numpy()
        assert (got[0] == -77).all() and (got[2] == -77).all()
        assert np.array_equal(got[1].astype(np.int64), _tt_match(torch, gt, boxes, 0.5, 0.4, True))


# ---- 3. anchors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.ANCHOR_CASES, ids=lambda c: "kind%d-%dx%d-last%dx%d" % (c[0], c[1], c[2], c[3][-1][0], c[3][-1][1]))
def test_anchors_equal_torchvisions_generator_on_uneven_pyramids(T, case):
    """Both anchor sets against the numpy restatement of AnchorGenerator (pinned to the recorded reference anchors and to the oracle's base
    anchors on the CPU; on the divisible shapes here it is pinned by the kernel too).  At 96 x 160 the last levels have strides 48 / 53 and
    96 / 80.  Catches: a fixed `4 << l` (or `8 << l`) stride, one stride for both axes, the quotient rounded up, kind 1's nine anchors
    ordered size-major instead of ratio-major, base anchors of level l + 1."""
    torch, ops = T
    kind, Hp, Wp, level_hw = case
    got = ops.anchors(Hp, Wp, level_hw, torch.device("cuda"), kind=kind)
    assert torch.equal(got.cpu(), torch.from_numpy(E.anchors_np(kind, Hp, Wp, level_hw)))


# ---- 4. box_encode and roi_gather ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.ENCODE_N)
def test_box_encode_on_equal_thin_and_empty_boxes(T, n):
    """BoxCoder.encode against float64, 1e-6 of the largest entry (test_gpu_train.py's bound), with rows where reference == proposal
    (exact zeros), 1000 : 1 width ratios both ways and a reference of width 0 (-inf, positions compared, rows left out of the norm), on
    both sides of the 256-thread boundary.  The ordinary rows are also held to their own largest entry: torch float32 is 1.33e-6 of it from
    float64 on these rows, the kernel is allowed 4 times that, 5.3e-6 (computed in the test from torch, never from the kernel).  Catches: the centre computed as (x0 + x1) / 2 from rounded halves (reference == proposal would
    not give 0), the weights swapped between the centre and the size terms, log of the inverse ratio, a last row left unwritten."""
    torch, ops = T
    from oracle import torch_train as tt
    ref, prop, kind = E.encode_rows(n)
    for w in E.ENCODE_WEIGHTS:
        out = ops.box_encode(torch.from_numpy(ref).cuda(), torch.from_numpy(prop).cuda(), w).cpu().numpy()
        want = tt.encode(torch.from_numpy(ref).double(), torch.from_numpy(prop).double(), w).numpy()
        assert np.array_equal(np.isneginf(out), np.isneginf(want)) and not np.isnan(out).any()
        fin = ~np.isneginf(want).any(axis=1)
        assert np.all(out[kind == 0] == 0), "reference == proposal"
        _close(out[fin], want[fin], 1e-6, "BoxCoder.encode n=%d w=%s" % (n, w))
        ordinary = kind < 0
        if ordinary.any():
            # the 1000 : 1 rows set the scale above (entries of thousands).  The ordinary rows against THEIR largest entry: torch's own float32
            # result is 1.33e-6 of it from float64 on these rows (measured here on the CPU, not taken from the kernel), so 1e-6 is not to be
            # had and the kernel gets 4 times torch's distance, 5.3e-6 -- its operation order may differ from torch's by what torch's
            # differs from exact
            t32 = tt.encode(torch.from_numpy(ref), torch.from_numpy(prop), w).numpy()
            d32 = float(np.abs(t32[ordinary].astype(np.float64) - want[ordinary]).max() / np.abs(want[ordinary]).max())
            assert 1e-7 < d32 < 2e-6, d32
            _close(out[ordinary], want[ordinary], 4 * d32, "BoxCoder.encode, ordinary rows (torch float32: %.3g) n=%d w=%s" % (d32, n, w))
        empty = np.flatnonzero(~fin)
        if len(empty):                                       # the finite columns of the rows with -inf, held to the same scale
            cols = [0, 1, 3]
            assert np.abs(out[empty][:, cols] - want[empty][:, cols]).max() <= 1e-6 * np.abs(want[fin]).max()


@pytest.mark.parametrize("name", sorted(E.ROI_CASES))
def test_roi_gather_on_the_samplers_own_block(T, name):
    """The int64 block train_ops.roi_sample_host writes, through roi_gather: RoI rows (image index, box) equal as bytes to the numpy
    gathers, targets within 1e-6 of float64 BoxCoder.encode.  Cases: no foreground row, R == cap, R of 1 / 255 / 257, an image without
    ground truth (its rows carry image index 1.0 and point at the extra zero box).  Catches: the image index read as an int64 instead of the
    float32 packed in the sixth list, a list stride of R instead of cap, targets written for R rows instead of n_pos, pos_rows used as a
    table row, a target written when n_pos == 0."""
    torch, ops = T
    from cald_amd import _ffi
    from cald_amd.detector import get_ctx
    c = E.roi_case(ops, name)
    w = (10.0, 10.0, 5.0, 5.0)
    want_rois, want_tgt = E.roi_want(c, w)
    table, gts, dev = torch.from_numpy(c["table"]).cuda(), torch.from_numpy(c["gts"]).cuda(), torch.from_numpy(c["blk"]).cuda()
    rois, tgt = ops.roi_gather(table, gts, dev, c["cap"], c["R"], c["n_pos"], w)
    assert rois.cpu().numpy().tobytes() == want_rois.tobytes()
    assert tgt.shape == (c["n_pos"], 4)
    if c["n_pos"]:
        _close(tgt, want_tgt, 1e-6, "roi_gather targets " + name)
    # the C entry point on buffers with a sentinel behind the rows it owns
    rois_buf = torch.full((c["R"] + 1, 5), E.SENTINEL, device="cuda")
    tgt_buf = torch.full((c["n_pos"] + 4, 4), E.SENTINEL, device="cuda")
    _ffi.check(_ffi.lib().cald_train_roi_gather(get_ctx(0), C.c_void_p(table.data_ptr()), C.c_void_p(gts.data_ptr()), C.c_void_p(dev.data_ptr()),
                                                c["cap"], c["R"], c["n_pos"], *w, C.c_void_p(rois_buf.data_ptr()), C.c_void_p(tgt_buf.data_ptr())))
    torch.cuda.synchronize()
    assert rois_buf[:c["R"]].cpu().numpy().tobytes() == want_rois.tobytes() and bool((rois_buf[c["R"]:] == E.SENTINEL).all())
    assert bool((tgt_buf[c["n_pos"]:] == E.SENTINEL).all()), "a target row beyond n_pos was written"
    assert tgt_buf[:c["n_pos"]].cpu().numpy().tobytes() == tgt.cpu().numpy().tobytes()
    if name == "image_without_gt":
        per = c["per"]
        assert bool((rois[per[0]:per[0] + per[1], 0] == 1.0).all()) and bool((rois[per[0] + per[1]:, 0] == 2.0).all())


# ---- 5. plain focal loss -----------------------------------------------------------------------------------------------------------
def _grad_buffer(torch, c):
    g = torch.full((c["N"] * sum(c["level_pix"]) * c["ld"],), E.SENTINEL)
    for b in E.focal_blocks(g, c["N"], c["level_pix"], c["ld"]):
        b[:, :, :c["A"] * c["K"]] = 0.0
    return g.cuda()


def _valid(torch, c, grad):
    bl = E.focal_blocks(grad, c["N"], c["level_pix"], c["ld"])
    ak = c["A"] * c["K"]
    return torch.cat([b[:, :, :ak].reshape(-1) for b in bl]), all(bool((b[:, :, ak:] == E.SENTINEL).all()) for b in bl)


def _plain(torch, ops, c, gscale):
    grad = _grad_buffer(torch, c)
    img_w = torch.tensor([1.0 / (d * c["N"]) for d in c["denom"]], dtype=torch.float32)
    loss = ops.focal_loss(c["flat"].cuda(), c["level_pix"], c["N"], c["A"], c["K"], c["ld"], c["matched"].cuda().contiguous(), c["gt_labels"].cuda(),
                          c["gt_off"].cuda(), img_w.cuda(), grad=grad, gscale=gscale)
    return loss, grad


def _check_against_float64(torch, c, loss, grad, gscale, what):
    want, want_grad = E.focal_want(c, gscale)
    _close(loss, want, 2e-6, what + ": focal loss")
    gv, intact = _valid(torch, c, grad)
    assert intact, "a pad column of the gradient was written"
    _close(gv, _valid(torch, c, want_grad)[0], 1e-5, what + ": focal loss gradient")
    gc = grad.cpu()
    for i in range(c["N"]):                                  # ignored anchors: the zeroed gradient untouched; the others written
        gi, m = E.focal_image_logits(gc, c, i), c["matched"][i]
        assert float(gi[m == -2].abs().max()) == 0.0 if bool((m == -2).any()) else True, i
        if bool((m != -2).any()):
            assert float(gi[m != -2].abs().max()) > 0.0, i


@pytest.mark.parametrize("A,K,ld,level_pix", E.FOCAL_SHAPES + [E.FOCAL_STRADDLE])
def test_plain_focal_loss_value_and_gradient_over_the_shape_table(T, A, K, ld, level_pix):
    """focal_loss over the segmented kernel's shape table, N = 3 with its planted values (0, -0, +-30, NaN in the pad columns, an image
    all background, one all ignored, foreground at the first and last anchor of the third), against float64: loss 2e-6, gradient 1e-5 of
    the largest entry.  Per-image totals of 256, 257, 512 and 513 anchors put two images into one 256-thread block.  Catches: the image
    index (weight, labels, logit row) taken from the block instead of from the thread, a level found with `>` for `>=` at a level's first
    anchor, a pad column read or written, an ignored anchor's gradient written."""
    torch, ops = T
    c = E.focal_case(A, K, ld, level_pix, seed=A * 1000 + K + level_pix[0])
    assert c["N"] == 3 and c["nfg"][0] == 0 and c["nfg"][1] == 0 and c["nfg"][2] >= 2
    loss, grad = _plain(torch, ops, c, 1.7)
    _check_against_float64(torch, c, loss, grad, 1.7, "N=3")
    loss2, grad2 = _plain(torch, ops, c, 1.7)
    assert loss2.cpu().numpy().tobytes() == loss.cpu().numpy().tobytes() and grad2.cpu().numpy().tobytes() == grad.cpu().numpy().tobytes()


@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("A,K,ld,level_pix", E.FOCAL_SHAPES + [E.FOCAL_STRADDLE])
def test_plain_focal_gradient_equals_the_segmented_kernels_bits(T, A, K, ld, level_pix, N):
    """Every image mixed, image n with 2^(n+1) foreground anchors, so max(1, #fg) and N are powers of two: focal_loss with img_weight
    1 / (denom N) and gscale 1, and focal_loss_seg with gscale 1 / N, scale the same g by the same float and the gradient buffers must be
    equal as bytes; the loss against float64 at 2e-6.  With A_tot = 257 and N = 2 the second block holds the last anchor of image 0 and 255
    of image 1.  Catches: the image index taken from the block (image 0's last anchor scaled and labelled as image 1's or the reverse: the
    two images' weights differ by a factor of two and their first and last anchors carry different classes)."""
    torch, ops = T
    c = E.focal_case(A, K, ld, level_pix, N=N, seed=5 + N, pow2=True)
    assert c["denom"] == [float(2 ** (i + 1)) for i in range(N)]
    loss, grad = _plain(torch, ops, c, 1.0)
    _check_against_float64(torch, c, loss, grad, 1.0, "N=%d" % N)
    seg_grad = _grad_buffer(torch, c)
    ops.focal_loss_seg(c["flat"].cuda(), c["level_pix"], N, A, K, ld, c["matched"].cuda().contiguous(), c["gt_labels"].cuda(), c["gt_off"].cuda(),
                       c["denom"], grad=seg_grad, gscale=torch.full((N,), 1.0 / N, dtype=torch.float32, device="cuda"))
    assert grad.cpu().numpy().tobytes() == seg_grad.cpu().numpy().tobytes()
