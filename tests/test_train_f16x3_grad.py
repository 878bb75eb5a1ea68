"""backward_precision="f16x3" on the host: the library's gradient-scale policy against its Python restatement, and the restatement of a
data gradient the GPU tests compare conv_h3 with (tests/_train_f16x3_grad_restatement.py) against float64 input gradients -- so the GPU
tests rest on a checked reference."""
import numpy as np
import pytest

import _train_f16x3_grad_restatement as GR
import _train_f16x3_restatement as R


def _policy_values():
    f32 = np.float32
    vals = [0.0, float("inf"), float("nan"), 1.5e-45, 1e-8, 1.0, 65504.0]
    for k in range(-40, 21):
        p = f32(2.0) ** f32(k)
        vals += [float(p), float(np.nextafter(p, f32(0)))]
    vals += [2.0 ** -100, 2.0 ** -60, 2.0 ** -54, 2.0 ** -53, 2.0 ** 66, 2.0 ** 67, 2.0 ** 70, 3.0e38]       # around and past the +-60 clamp
    return vals


def test_library_grad_scale_equals_the_restatement():
    from cald_amd import train_ops as ops
    seen = set()
    for v in _policy_values():
        got, want = ops.f16x3_grad_scale(v), GR.grad_scale(v)
        assert got == want, (v, got, want)
        seen.add(want[0])
        if np.isfinite(v) and v > 0 and abs(want[0]) < 60:
            assert 2.0 ** 10 <= float(np.float32(v)) * want[1] < 2.0 ** 11, v
    assert {60, -60, 0, 33, 6, -9}.issubset(seen), sorted(seen)        # both clamps, zero / non-finite, 1e-8, 1.0 and 65 504
    assert GR.grad_scale(1e-8) == (33, 2.0 ** 37) and GR.grad_scale(65504.0) == (-9, 2.0 ** -5)
    assert GR.grad_scale(float("nan"))[0] == 0 and GR.grad_scale(float("inf"))[0] == 0 and GR.grad_scale(1.5e-45)[0] == 60


DG_CASES = {   # forward weight shape, forward stride, forward pad, forward input H x W
    "3x3_pad1": ((32, 16, 3, 3), 1, 1, (6, 7)),
    "1x1": ((64, 32, 1, 1), 1, 0, (5, 9)),
    "3x3_stride2_dilated": ((32, 16, 3, 3), 2, 1, (9, 13)),
}


@pytest.mark.parametrize("mag", [1e-8, 1e-3, 1e3])
@pytest.mark.parametrize("case", sorted(DG_CASES))
def test_restatement_is_the_float64_input_gradient(oracle, case, mag):
    """The restatement alone -- transposed, flipped, BN-scaled filter; g * 2^G through the oracle's conv_h3; unscale 2^-(S_d + 4 + G);
    residual; mask -- stays within 4 * 2^-22 of the largest output entry of the float64 input gradient."""
    import torch
    shape, stride, pad, (H, W) = DG_CASES[case]
    rs = np.random.RandomState(sum(map(ord, case)))
    cout, cin, K = shape[0], shape[1], shape[2]
    w = (rs.standard_normal(shape) * 0.05).astype(np.float32)
    scale = (0.5 + rs.rand(cout)).astype(np.float32)
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    g = (rs.standard_normal((Ho, Wo, cout)) * mag).astype(np.float32)
    residual = (rs.standard_normal((H, W, cin)) * mag).astype(np.float32)
    mask = rs.standard_normal((H, W, cin)).astype(np.float32)
    G = GR.grad_scale(np.abs(g).max())[0]
    wd = GR.grad_filter(w, scale)
    gd = GR.dilate(g, stride, H + 2 * pad - K + 1, W + 2 * pad - K + 1) if stride > 1 else g
    got = GR.dgrad(oracle, gd, wd, K - 1 - pad, G, residual=residual, mask=mask)
    assert got.shape == (H, W, cin)
    g64 = torch.from_numpy(g).double().permute(2, 0, 1)[None] * torch.from_numpy(scale).double().view(1, -1, 1, 1)
    dx = torch.nn.grad.conv2d_input((1, cin, H, W), torch.from_numpy(w).double(), g64, stride=stride, padding=pad)[0].permute(1, 2, 0).numpy()
    want = np.where(mask > 0, dx + residual.astype(np.float64), 0.0)
    err = float(np.abs(got.astype(np.float64) - want).max()) / float(np.abs(want).max())
    print("%s at %g: G = %d, error / max |dx| = %.3g (bound %.3g)" % (case, mag, G, err, 4 * 2.0 ** -22))
    assert err <= 4 * 2.0 ** -22


def test_grad_filter_of_the_tap_major_linear_form():
    """fc6's form: the data gradient's 1 x 1 filter row co, column t * Cin + ci is torch's w[co, ci * taps + t] times the row scale."""
    cout, cin, taps = 6, 16, 49
    w = np.arange(cout * cin * taps, dtype=np.float32).reshape(cout, cin * taps)
    wd = GR.grad_filter(w, cin_k=8, taps=taps)
    assert wd.shape == (taps * cin, 8) and not wd[:, cout:].any()
    for co, ci, t in ((0, 0, 0), (5, 15, 48), (2, 7, 13)):
        assert wd[t * cin + ci, co] == w[co, ci * taps + t]
    S, words = GR.grad_twin(GR.grad_filter(w, cin_k=16, taps=taps))
    assert words.shape == (1, 2, R.cout_pad(taps * cin), 16) and S == R.f16x3_scale(w.max())[0]


def test_trainer_keyword_is_validated_before_any_device_work():
    from cald_amd import train
    for cls in (train.FasterRCNNTrainer, train.RetinaNetTrainer, train.RetinaNetLLTrainer):
        with pytest.raises(ValueError, match="backward_precision"):
            cls({}, 3, backward_precision="fp16", device="cpu")
