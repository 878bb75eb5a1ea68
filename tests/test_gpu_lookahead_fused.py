"""The certified RPN pruning's look-ahead as ONE launch (conv_h4.hip's head epilogue, cald_model_set_look_fuse) and the reworked
prune_scatter_kernel (rpn_prune.hip).

The fused epilogue claims the bits of the two-launch path: the hidden value in h16_epilogue's operation order, then per row and logit the
k-ascending fp32 fma chain the exact 1 x 1 kernel's v_mfma_f32_32x32x2_f32 evaluates, then the bias.  Nothing here takes that on trust: the
probe tests hold the fused launch against the two launches on the same inputs byte for byte, on ragged batches that reach every row-validity
path of the epilogue (a full workgroup, an absent second half, halves in different views, a workgroup with 12 valid rows, one row), with
3 x 3 convs of 9 and 18 k-steps (the general tail loop and the unrolled body of conv_h4's k-loop); the model tests compare whole forwards.
The scatter / select kernels are held against a numpy restatement of the selection on the dense head's maps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FP32, F16X3 = 0, 1
GENERIC, H4_GROUP = 4, 9
SENT = np.uint32(0xFFC0DEAD)          # a NaN no kernel produces from finite operands
GUARD = 128                           # guard rows after the last output row (one whole M tile)
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def hip():
    import torch
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


def split_words(x, Cn):
    """h16.h split form of x [pixels][Cn] (Cn % 16 == 0): per 16-channel chunk [16 fp16 hi | 16 fp16 lo] of 16 x, as uint32 [pixels][Cn]."""
    s = (np.asarray(x, np.float32) * np.float32(16)).astype(np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    P = s.shape[0]
    h = np.empty((P, Cn // 16, 2, 16), np.float16)
    h[:, :, 0, :] = hi.reshape(P, Cn // 16, 16)
    h[:, :, 1, :] = lo.reshape(P, Cn // 16, 16)
    return np.ascontiguousarray(h).view(np.uint32).reshape(P, Cn)


def _probe(hip, views, Cin, Cout, K, weight, bias, x, relu, path, precision, x16=None, out=None, head=None):
    """One launch through cald_op_conv_probe; `out` / head = (w, b, buf, ld) are the caller's buffers (guard words included)."""
    ffi = hip["ffi"]
    p = ffi.ConvProbe()
    p.V = len(views)
    for v, (H, W) in enumerate(views):
        p.in_hw[v][0], p.in_hw[v][1] = H, W
    p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad = Cin, Cout, K, K, 1, K // 2
    p.relu, p.in_relu, p.out_ld, p.cin_true = int(relu), 0, Cout, Cin
    p.weight, p.bias, p.in_ = ffi.ptr(weight), ffi.ptr(bias), ffi.ptr(x)
    p.in16 = ffi.ptr(x16, C.POINTER(C.c_uint32))
    if out is not None:
        p.out, p.out_n = ffi.ptr(out.view(np.float32)), out.size
    if head is not None:
        hw, hb, hbuf, hld = head
        p.head_w, p.head_b, p.head_out, p.head_out_n, p.head_ld = ffi.ptr(hw), ffi.ptr(hb), ffi.ptr(hbuf.view(np.float32)), hbuf.size, hld
    arr = (ffi.ConvProbe * 1)(p)
    name = C.create_string_buffer(256)
    ffi.check(hip["L"].cald_op_conv_probe(hip["ctx"], precision, arr, 1, path, 0, name, 256))
    return name.value.decode()


BATCHES = {
    "one_full_workgroup_16x16": [(16, 16)],
    "117_rows_second_half_absent": [(9, 13)],
    "halves_in_two_views_then_12_rows": [(9, 13), (20, 7)],
    "one_row": [(1, 1)],
}


@pytest.mark.parametrize("Cin", [16, 32])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_fused_head_equals_the_two_launch_path_byte_for_byte(hip, batch, Cin):
    """cald_op_conv_probe, conv_h4 grouped, 3 x 3 / pad 1 / 256 channels + ReLU: head_out[:, :3] of the fused launch == the hidden tensor of the
    same kernel without head fields followed by the exact 1 x 1 256 -> 15 launch (conv_mfma_f32_kernel<4,1,1,1>, the product's look-ahead
    head), channels 0..2; guard rows and channels 3..14 of head_out come back untouched."""
    views = BATCHES[batch]
    rs = np.random.RandomState(1000 * Cin + len(batch))
    R = sum(h * w for h, w in views)
    x = rs.randn(R, Cin).astype(np.float32)
    x[rs.rand(R, Cin) < 0.3] = 0.0
    w3 = (rs.randn(256, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b3 = rs.randn(256).astype(np.float32)
    w1 = (rs.randn(15, 256, 1, 1) * np.sqrt(1.0 / 256)).astype(np.float32)           # mixed signs
    b1 = rs.randn(15).astype(np.float32)
    x16 = split_words(x, Cin)
    # two launches: the hidden tensor, then the exact head
    hidden = np.full((R + GUARD, 256), SENT, np.uint32)
    assert _probe(hip, views, Cin, 256, 3, w3, b3, x, True, H4_GROUP, F16X3, x16=x16, out=hidden) == "conv_h4_group_kernel"
    hid = np.ascontiguousarray(hidden[:R]).view(np.float32)
    assert np.isfinite(hid).all() and (hid == 0).mean() > 0.2 and (hid > 0).mean() > 0.2      # the ReLU cut negative pre-activations
    two = np.full((R + GUARD, 15), SENT, np.uint32)
    assert _probe(hip, views, 256, 15, 1, w1, b1, hid, False, GENERIC, FP32, out=two).startswith("conv_mfma_f32_kernel<4,1,1,1,0,16,true>")
    # one launch
    one = np.full((R + GUARD, 15), SENT, np.uint32)
    hw = np.ascontiguousarray(w1[:3, :, 0, 0]); hb = np.ascontiguousarray(b1[:3])
    assert _probe(hip, views, Cin, 256, 3, w3, b3, x, True, H4_GROUP, F16X3, x16=x16, head=(hw, hb, one, 15)) == "conv_h4_look_kernel"
    bad = np.argwhere(one[:R, :3] != two[:R, :3])
    assert bad.size == 0, ("%d of %d logits differ, first (row, logit) %s: fused %r, two launches %r"
                           % (len(bad), 3 * R, bad[0], one[:R, :3].view(np.float32)[tuple(bad[0])], two[:R, :3].view(np.float32)[tuple(bad[0])]))
    assert (one[R:] == SENT).all(), "stores past the last valid row"
    assert (one[:R, 3:] == SENT).all(), "stores into channels 3..14"


def _small_model(hip):
    from cald_amd import synth
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    m = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=64, max_size=128).to("cuda")
    m.load_state_dict(sd); m.eval()
    return m


DET_KEYS = ("boxes", "scores", "labels", "props", "prob_max", "scores_cls", "count")
MAPS = ("rpn_look0", "rpn_look1", "rpn_pnorm0", "rpn_pnorm1", "rpn0", "rpn1")


def _capture(m, views):
    m.set_rpn_prune_capture(True)
    got = m.forward_views(views)
    det = [{k: got[v][k].cpu().numpy().copy() for k in DET_KEYS if k in got[v]} for v in range(len(views))]
    cap = [{n: m.debug_tensor(n, v) for n in MAPS} for v in range(len(views))]
    m.set_rpn_prune_capture(False)
    return det, cap


def test_fused_look_ahead_in_the_model_on_tiny_and_odd_views(hip):
    """Capture-mode forwards on small odd-sized views (conv_h4 would not take them by its own rule: mode 2 forces it): the look-ahead's logits,
    the scattered maps and the detections under set_look_fuse(2) == set_look_fuse(0) byte for byte; channels 3..14 of rpn_look are zero where
    the fused look-ahead ran and are the look-ahead's box deltas under mode 0."""
    torch = hip["torch"]
    from cald_amd import synth
    m = _small_model(hip)
    sizes = [(64, 128), (32, 40), (61, 47), (97, 401)]
    views = [(torch.from_numpy(synth.synth_image(950 + i, h, w)).cuda(), bool(i & 1), None) for i, (h, w) in enumerate(sizes)]
    assert m.set_look_fuse(2) == 1                       # mode 1 is the default
    det2, cap2 = _capture(m, views)
    assert m.set_look_fuse(0) == 2
    det0, cap0 = _capture(m, views)
    m.set_look_fuse(1)
    for v in range(len(views)):
        for k in det0[v]:
            assert det2[v][k].tobytes() == det0[v][k].tobytes(), (v, k)
        for l in range(2):
            a, b = cap2[v]["rpn_look%d" % l], cap0[v]["rpn_look%d" % l]
            assert a.shape == b.shape and a.shape[2] == 15
            assert a[:, :, :3].tobytes() == b[:, :, :3].tobytes(), (v, l)
            assert (a[:, :, 3:] == 0).all(), (v, l)
            assert (b[:, :, 3:] != 0).any(), (v, l)
            assert cap2[v]["rpn%d" % l].tobytes() == cap0[v]["rpn%d" % l].tobytes(), (v, l)
            assert cap2[v]["rpn_pnorm%d" % l].tobytes() == cap0[v]["rpn_pnorm%d" % l].tobytes(), (v, l)


def _kth_largest(vals, k):
    return np.sort(vals.reshape(-1))[::-1][k - 1]


def _restate_selection(look, pn, dense, c1, c0, pre_n):
    """rpn_prune.hip's two selection stages on one (level, view), in the kernels' float32 arithmetic: the selected pixel mask."""
    H, W, _ = look.shape
    n = H * W * 3
    if n <= pre_n:
        return np.ones((H, W), bool)
    B = (c1[None, None, :] * pn[:, :, None]).astype(np.float32) + c0[None, None, :]
    lg = look[:, :, :3]
    lb, ub = (lg - B).astype(np.float32), (lg + B).astype(np.float32)
    tau = _kth_largest(lb, pre_n)
    first = (lb >= tau).any(axis=2)
    exact0 = dense[:, :, :3][first]
    tau2 = tau
    if exact0.size >= pre_n:
        tau2 = max(tau, _kth_largest(exact0, pre_n))
    return first | (ub >= tau2).any(axis=2)


def test_scatter_and_select_against_the_dense_head(hip):
    """The two-launch look-ahead (set_look_fuse(0): only rpn_prune.hip differs from the dense path) on half-size VOC views, where the pruning does
    prune.  With the selection restated in numpy from the look-ahead's maps and the dense head's: the scattered maps rpn0/1 carry the dense
    head's bits in all 15 channels of every selected pixel and -FLT_MAX in the logits of every other; and a sweep over the same views reports
    exactly the restated selected fractions and the restated worst |look-ahead - exact| / bound (cald_profile_prune keeps the largest ratio of
    the context's life: it must end at max(its value before, the restated one)), finite and <= 1."""
    torch, ffi, L = hip["torch"], hip["ffi"], hip["L"]
    from cald_amd import synth, sweep
    sd = synth.pseudo_trained_frcnn(21, 50, seed=0)
    m = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=300, max_size=500).to("cuda")
    m.load_state_dict(sd); m.eval()
    pool = synth.make_pool(3, "voc", 4, scale=0.5)
    dev = [torch.from_numpy(im).cuda() for im in pool]
    views = [(d, False, None) for d in dev] + [(d, True, None) for d in dev]          # the views of a sweep with augs = ["flip"]
    c1, c0 = m.rpn_prune_bound()
    m.set_look_fuse(0)
    _, cap = _capture(m, views)
    m.forward_views(views)                                                             # the dense head
    sel_n, pix_n, worst = [0, 0], [0, 0], np.float32(0)
    for v in range(len(views)):
        for l in range(2):
            dense = m.debug_tensor("rpn%d" % l, v)
            look, pn, pruned = cap[v]["rpn_look%d" % l], cap[v]["rpn_pnorm%d" % l][:, :, 0], cap[v]["rpn%d" % l]
            sel = _restate_selection(look, pn, dense, c1, c0, 1000)
            assert np.array_equal(pruned[:, :, 0] != -FMAX, sel), (v, l)
            assert pruned[sel].tobytes() == dense[sel].tobytes(), (v, l)                # all 15 channels of every selected pixel
            assert (pruned[~sel][:, :3] == -FMAX).all(), (v, l)
            B = (c1[None, :] * pn[sel][:, None]).astype(np.float32) + c0[None, :]
            ratio = np.abs(look[sel][:, :3] - dense[sel][:, :3]).astype(np.float32) / B
            worst = max(worst, ratio.max())
            sel_n[l] += int(sel.sum()); pix_n[l] += sel.size
    assert 0 < sel_n[0] < 0.6 * pix_n[0]                                               # it does prune
    before = C.c_double()
    ffi.check(L.cald_profile_prune(hip["ctx"], None, None, None, C.byref(before), None))
    ffi.check(L.cald_profile_enable(hip["ctx"], 1))
    sweep.sweep_device_images(m, dev, [0, 1, 2], ["flip"], bp=1.3, base_seed=0, batch_images=3)
    after, frac = C.c_double(), (C.c_double * 2)()
    ffi.check(L.cald_profile_prune(hip["ctx"], None, None, frac, C.byref(after), None))
    ffi.check(L.cald_profile_enable(hip["ctx"], 0))
    m.set_look_fuse(1)
    print("selected %.4f of P2, %.4f of P3; worst ratio restated %.3e, context before %.3e, after %.3e"
          % (sel_n[0] / pix_n[0], sel_n[1] / pix_n[1], worst, before.value, after.value))
    assert [frac[0], frac[1]] == [sel_n[0] / pix_n[0], sel_n[1] / pix_n[1]]
    assert np.isfinite(worst) and 0 < worst <= 1
    assert after.value == max(before.value, float(worst))
