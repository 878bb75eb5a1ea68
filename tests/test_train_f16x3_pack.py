"""The split-fp16 weight pack of a forward_precision "f16x3" trainer, on the host: the numpy restatement the GPU tests compare the device
buffer with (tests/_train_f16x3_restatement.py) against the oracle's statement of the inference mode's pack (oracle.f16x3_weights:
values, S, unscale), and the library's host-side scale function against both -- over the value ranges where the scale policy or the
split can go wrong."""
import numpy as np
import pytest

import _train_f16x3_restatement as R

SHAPES = {"3x3_chunked": ((64, 16, 3, 3), None), "stem_rgb0": ((64, 3, 7, 7), 4), "1x1": ((32, 48), None)}
CASES = sorted(R.weight_cases((2, 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_restatement_equals_the_oracles_pack(oracle, shape, case):
    dims, cin_k = SHAPES[shape]
    w = R.weight_cases(dims, seed=3)[case]
    kh, kw = (dims[2], dims[3]) if len(dims) == 4 else (1, 1)
    cin = cin_k if cin_k is not None else dims[1]
    with np.errstate(over="ignore", invalid="ignore"):
        ref = oracle.f16x3_weights(R.hwc_rows(w, cin_k), kh, kw, cin)
    S, unscale = R.f16x3_scale(np.abs(w).max())
    assert (S, unscale) == (ref["S"], ref["unscale"])
    wk = R.kmajor(w, cin_k)
    assert wk.shape[0] == ref["Kpad"]
    hi, lo = R.split(wk, S)
    n = ref["Npad"] if ref["Npad"] < wk.shape[1] else wk.shape[1]
    # the halves are fp16 values: equal as bit patterns (inf included; the oracle hands them out widened to fp32)
    assert np.array_equal(hi.view(np.uint16)[:, :n], _bits(ref["vh"])[:, :n])
    assert np.array_equal(lo.view(np.uint16)[:, :n], _bits(ref["vl"])[:, :n])
    assert not hi[:, dims[0]:].any() and not lo[:, dims[0]:].any()          # padded output channels hold zeros
    # and the buffer layout puts element (k, n) of plane p at [k / 16][p][n][k % 16]
    buf = R.pack_w16(wk, S)
    k, col = wk.shape[0] - 3, dims[0] - 1
    assert buf[k // 16, 0, col, k % 16] == hi.view(np.uint16)[k, col] and buf[k // 16, 1, col, k % 16] == lo.view(np.uint16)[k, col]


def test_value_cases_reach_what_they_are_for():
    c = R.weight_cases((64, 16, 3, 3), seed=3)
    S = {k: R.f16x3_scale(np.abs(v).max())[0] for k, v in c.items()}
    assert S["pow2"] == 15 and S["pow2_minus_ulp"] == 16 and S["zero"] == 0 and S["tiny_1e-6"] == 33
    assert S["clamp_hi"] == 40 and S["clamp_lo"] == -40 and S["mixed_1_and_1e-7"] == 13
    hi, lo = R.split(c["mixed_1_and_1e-7"], 13)
    sub = (np.abs(lo.astype(np.float32)) < 2.0 ** -14) & (lo != 0)
    assert sub.any(), "the lo halves of the 1e-7 weights must be fp16 subnormals"
    hi, _ = R.split(c["clamp_lo"], -40)
    assert np.isinf(hi.astype(np.float32)).any()


def test_tap_major_linear_index():
    """fc6's form: torch column ci * taps + tap lands on K-major row tap * Cin + ci."""
    cout, cin, taps = 5, 16, 49
    w = np.arange(cout * cin * taps, dtype=np.float32).reshape(cout, cin * taps)
    wk = R.kmajor(w, taps=taps)
    assert wk.shape == (taps * cin, 32)
    for co, ci, t in ((0, 0, 0), (4, 15, 48), (2, 7, 13)):
        assert wk[t * cin + ci, co] == w[co, ci * taps + t]


@pytest.mark.parametrize("value", [0.25, float(np.nextafter(np.float32(0.25), np.float32(0))), 0.0, 1e-6, 1.0, 2.0 ** -60, 2.0 ** 70,
                                   float("inf"), float("nan"), 3.0e38, 1.5e-45])
def test_library_scale_function(value):
    from cald_amd import train_ops as ops
    assert ops.f16x3_scale(value) == R.f16x3_scale(value)


def test_trainer_keyword_is_validated_before_any_device_work():
    from cald_amd import train
    for cls in (train.FasterRCNNTrainer, train.RetinaNetTrainer, train.RetinaNetLLTrainer):
        with pytest.raises(ValueError, match="forward_precision"):
            cls({}, 3, forward_precision="fp16", device="cpu")
