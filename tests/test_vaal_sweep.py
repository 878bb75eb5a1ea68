"""CPU tests of the VAAL sweep's contract (cald_amd/vaal.py, tests/_vaal_restatement.py, tests/golden/vaal.npz): the weight generator and
the fixture agree, the package's modules carry the reference's state_dict() layout, the resize restatement equals live F.interpolate, the
float32 restatement of the whole path stays within its a-priori bound of float64 and about as close to the reference's float64 values as
the reference's own float32 run, the selection equals the reference's, and state loading rejects what it must."""
import numpy as np
import pytest

import _vaal_restatement as R

# How much farther from the float64 values the stated orders may be than torch's own float32 run, relative to max|tensor|.  Measured on the
# fixture (restatement / torch): mu 3.99e-6 / 1.13e-6 = 3.5x in train mode and 1.70e-6 / 9.56e-7 = 1.8x in eval mode; preds 1.70e-6 /
# 6.05e-7 = 2.8x and 2.43e-6 / 9.46e-7 = 2.6x.  The excess is the convolutions' contract: one sequential fmaf chain of 16 Cin = 1 024 ..
# 8 192 terms per output where torch sums in blocks (fc_mu's two-level order and the 256-pixel chunks of the statistics add nothing
# visible: their stages sit at 4e-4 and 4e-2 of their own bounds).  4 covers the largest ratio seen with the slack of one rounding draw;
# the ceiling for any order worth keeping is 8.
MARGIN = 4.0


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("vaal")
    return dict(g=g, images=[g["image%d" % i] for i in range(int(g["n_images"]))], budget=int(g["budget"]))


@pytest.fixture(scope="module")
def weights(fx):
    return R.make_weights(int(fx["g"]["seed"]))


@pytest.fixture(scope="module")
def evaluated(fx, weights, oracle):
    """Per BatchNorm mode the float32 restatement, the float64 evaluation and the a-priori bound: computed once."""
    out = {}
    wt = R.fc_weight_kprime(weights["fc_mu.weight"])
    for tag, running in (("train", False), ("eval", True)):
        mu, preds = R.sweep(oracle, weights, fx["images"], running, wt)
        mu64, p64, mub, pb = R.sweep64(weights, fx["images"], running, oracle)
        out[tag] = dict(mu=mu, preds=preds, mu64=mu64, p64=p64, mub=mub, pb=pb)
    return out


def test_generator_reproduces_the_fixture_hash(fx, weights):
    assert R.weights_sha1(weights) == str(fx["g"]["sha1"])
    for k, shape in R.used_keys():
        assert weights[k].shape == shape and weights[k].dtype == np.float32
    for l in range(5):      # non-trivial biases and BatchNorm tensors
        for k in ("encoder.%d.bias" % (3 * l), "encoder.%d.bias" % (3 * l + 1), "encoder.%d.running_mean" % (3 * l + 1)):
            assert np.unique(weights[k]).size > 16
        assert weights["encoder.%d.running_var" % (3 * l + 1)].min() > 0


def test_modules_have_the_reference_state_layout(fx):
    from cald_amd import vaal
    want = [(str(k), tuple(int(d) for d in s[:int(np.count_nonzero(s))])) for k, s in zip(fx["g"]["sd_keys"], fx["g"]["sd_shapes"])]
    got = []
    for mod in (vaal.VAE(), vaal.Discriminator()):
        got += [(k, tuple(v.shape)) for k, v in mod.state_dict().items()]
    assert got == want
    used = dict(want)
    for k, shape in vaal.expected_shapes().items():
        assert used[k] == shape
    assert sorted(vaal.expected_shapes()) == sorted(k for k, _ in R.used_keys())


def test_modules_compute_the_reference_forward(fx, weights):
    """The package's VAE / Discriminator, loaded with the generated weights, give the fixture's float32 mu and predictions in eval mode
    (batch of one, so the same torch kernels run) to float32 rounding."""
    import torch
    from cald_amd import vaal
    torch.manual_seed(0)
    vae, disc = vaal.VAE(), vaal.Discriminator()
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items() if not k.startswith("net.")}, strict=False)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items() if k.startswith("net.")})
    vae.eval()
    with torch.no_grad():
        for i in (0, 5):
            x = torch.from_numpy(fx["images"][i]).permute(2, 0, 1).float().div(255)
            _, _, mu, _ = vae([x])
            assert np.allclose(mu.numpy()[0], fx["g"]["mu_eval"][i], rtol=0, atol=1e-5 * np.abs(fx["g"]["mu_eval"][i]).max())
            assert abs(float(disc(mu)) - float(fx["g"]["preds_eval"][i])) < 1e-5


PAIRS = [(1, 1), (1333, 1), (1, 1333), (2, 255), (255, 2), (256, 257), (257, 256), (333, 500), (500, 1333), (256, 256)]


@pytest.mark.parametrize("H,W", PAIRS)
def test_resize_restatement_equals_live_interpolate(H, W):
    import torch
    import torch.nn.functional as F
    assert {h for h, _ in PAIRS} | {w for _, w in PAIRS} >= set(R.SIZES)
    img = np.random.RandomState(H * 2048 + W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    t = torch.from_numpy(img).permute(2, 0, 1).float().div(255)
    live = (F.interpolate(t[None], (256, 256)) * 255)[0].permute(1, 2, 0).numpy()
    assert np.array_equal(R.resize(img), live)


def test_times_255_gives_the_byte_back():
    u = np.arange(256, dtype=np.float32)
    assert np.array_equal((u / np.float32(255)).astype(np.float32) * np.float32(255), u)


def test_resize_index_float_and_integer_forms_agree():
    for n in list(range(1, 700)) + [1000, 1333, 2048, 4000]:
        f = np.minimum(np.floor(np.arange(256, dtype=np.float32) * np.float32(n / 256.0)).astype(np.int64), n - 1)
        assert np.array_equal(R.resize_index(n), f), n


def test_det_exp_restatement_equals_the_oracle(oracle):
    x = np.concatenate([np.linspace(-100, 100, 4001), [-87.0, 88.72283, 0.0, -0.0, 1e-8]]).astype(np.float32)
    assert np.array_equal(R.det_exp(x), oracle.exp_array(x))


@pytest.mark.parametrize("tag", ["train", "eval"])
def test_float32_restatement_within_its_bound_of_float64(tag, evaluated, fx):
    """The bound carried through the whole path is rigorous and worst-case: every layer multiplies it by its absolute-weight norm, so it
    ends many orders above the values (the printed ratios) and holds without pinning anything; the stage test below and the comparison
    with the reference's own float32 distance are the checks with teeth."""
    e = evaluated[tag]
    dmu, dp = np.abs(e["mu"].astype(np.float64) - e["mu64"]), np.abs(e["preds"].astype(np.float64) - e["p64"])
    print("%s: max |mu32 - mu64| / bound = %.3g, max |p32 - p64| / bound = %.3g" % (tag, (dmu / e["mub"]).max(), (dp / e["pb"]).max()))
    assert np.all(dmu <= e["mub"]) and np.all(dp <= e["pb"])
    # the fixture's float64 values are the same function: the bound holds against them as well
    assert np.all(np.abs(e["mu"].astype(np.float64) - fx["g"]["mu64_" + tag]) <= e["mub"])
    assert np.all(np.abs(e["preds"].astype(np.float64) - fx["g"]["preds64_" + tag]) <= e["pb"])
    assert np.abs(e["mu64"] - fx["g"]["mu64_" + tag]).max() <= 1e-9 * np.abs(e["mu64"]).max()


@pytest.mark.parametrize("running", [False, True])
def test_every_stage_within_its_own_bound(running, fx, weights, oracle):
    """One image (portrait, larger than 256 both ways), every stage against float64 on the same float32 input: the bounds with teeth."""
    for stage, ratio in R.stage_checks(oracle, weights, fx["images"][1], running):
        print("running=%s %s: |float32 - float64| / bound = %.3g" % (running, stage, ratio))
        assert ratio <= 1.0, stage


@pytest.mark.parametrize("tag", ["train", "eval"])
def test_as_close_to_float64_as_the_reference_float32(tag, evaluated, fx):
    g, e = fx["g"], evaluated[tag]
    for name, mine, ref32, ref64 in (("mu", e["mu"], g["mu_" + tag], g["mu64_" + tag]), ("preds", e["preds"], g["preds_" + tag], g["preds64_" + tag])):
        scale = np.abs(ref64).max()
        d_mine = np.abs(mine.astype(np.float64) - ref64).max() / scale
        d_ref = np.abs(ref32.astype(np.float64) - ref64).max() / scale
        print("%s %s: restatement %.3g, reference float32 %.3g of max|%s| (ratio %.2f)" % (tag, name, d_mine, d_ref, name, d_mine / d_ref))
        assert d_mine <= MARGIN * d_ref


@pytest.mark.parametrize("tag", ["train", "eval"])
def test_selection_equals_the_reference(tag, evaluated, fx):
    from cald_amd import vaal
    want = fx["g"]["idx_" + tag]
    assert np.array_equal(R.select_lowest(evaluated[tag]["preds"], fx["budget"]), want)
    assert np.array_equal(vaal.select_lowest(evaluated[tag]["preds"], fx["budget"]), want)
    assert np.array_equal(vaal.select_lowest(fx["g"]["preds_" + tag], fx["budget"]), want)


def test_ties_go_to_the_lower_position_and_budget_is_capped():
    from cald_amd import vaal
    p = np.array([0.5, 0.25, 0.5, 0.25, 0.75, 0.25], np.float32)
    for sel in (vaal.select_lowest, R.select_lowest):
        assert sel(p, 4).tolist() == [1, 3, 5, 0]
        assert sel(p, 6).tolist() == [1, 3, 5, 0, 2, 4]
        assert sel(p, 100).tolist() == [1, 3, 5, 0, 2, 4]
        assert sel(p, 0).tolist() == []
        assert sel(p, 4).dtype == np.int64


def test_state_loading_rejects_missing_and_misshaped_and_ignores_the_decoder():
    from cald_amd import vaal
    sd = {k: np.zeros(s, np.float32) for k, s in vaal.expected_shapes().items()}
    vsd = {k: v for k, v in sd.items() if not k.startswith("net.")}
    dsd = {k: v for k, v in sd.items() if k.startswith("net.")}
    extra = dict(vsd)
    extra.update({"decoder.0.weight": np.zeros((3, 5), np.float32), "fc_logvar.weight": np.zeros((2, 2), np.float32),
                  "encoder.1.num_batches_tracked": np.zeros((), np.int64)})
    assert sorted(vaal.checked_state(extra, dsd)) == sorted(sd)
    for missing in ("encoder.12.weight", "encoder.4.running_var", "fc_mu.bias"):
        with pytest.raises(KeyError, match=missing):
            vaal.checked_state({k: v for k, v in vsd.items() if k != missing}, dsd)
    with pytest.raises(KeyError, match="net.2.bias"):
        vaal.checked_state(vsd, {k: v for k, v in dsd.items() if k != "net.2.bias"})
    bad = dict(vsd); bad["encoder.3.weight"] = np.zeros((128, 64, 3, 3), np.float32)
    with pytest.raises(ValueError, match="encoder.3.weight"):
        vaal.checked_state(bad, dsd)
    bad = dict(dsd); bad["net.4.weight"] = np.zeros((512,), np.float32)
    with pytest.raises(ValueError, match="net.4.weight"):
        vaal.checked_state(vsd, bad)
    with pytest.raises((KeyError, ValueError)):
        vaal.VaalModel(bad, dsd)            # rejected before the library or a device is touched
