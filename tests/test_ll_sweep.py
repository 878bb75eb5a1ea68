"""CPU tests of the learning-loss sweep (cald_amd.baselines.ll_get_uncertainty): the reference's recorded scores (tests/golden/lossnet.npz,
tools/make_golden_lossnet.py) against the float32 restatement (tests/_ll_restatement.py) and a float64 evaluation, the group padding rule,
the no-GPU behaviour, and the per-batch row packing through the all-gather."""
import socket

import numpy as np
import pytest

import _ll_restatement as R

CASES = {"faster_rcnn": (0, 1, 2, 3), "retina": (0, 0, 0, 0)}      # ll_train.py:155-161: features[0] four times for RetinaNet


def fixture_case(g):
    sd = {k[3:]: g[k] for k in g.files if k.startswith("sd_")}
    feats = [[np.ascontiguousarray(g["feat%d" % l][i].transpose(1, 2, 0)) for i in range(g["feat0"].shape[0])] for l in range(4)]
    return sd, feats


@pytest.mark.parametrize("model", sorted(CASES))
def test_restatement_and_reference_within_bound_of_float64(golden, oracle, model):
    g = golden("lossnet")
    sd, feats = fixture_case(g)
    levels = CASES[model]
    got, pooled = R.score_features(sd, feats, levels)
    want64, bound = R.score_features64(sd, feats, levels)
    ref = g["out_" + model]
    assert ref.dtype == np.float32 and got.dtype == np.float32 and got.shape == ref.shape == (int(g["batches"].sum()),)
    print(model, "restatement err/bound", np.abs(got - want64) / bound, "reference err/bound", np.abs(ref - want64) / bound)
    assert np.all(bound > 0)
    assert np.all(np.abs(got.astype(np.float64) - want64) <= bound)
    assert np.all(np.abs(ref.astype(np.float64) - want64) <= bound)
    # the restatement's linear layers are oracle.linear's contract: the same bytes from the C oracle
    hs = [oracle.linear(pooled[:, j], np.ascontiguousarray(sd["FC%d.weight" % (j + 1)].T), sd["FC%d.bias" % (j + 1)], relu=True) for j in range(4)]
    via_oracle = oracle.linear(np.concatenate(hs, axis=1), np.ascontiguousarray(sd["linear.weight"].T), sd["linear.bias"])[:, 0]
    assert via_oracle.tobytes() == got.tobytes()
    if model == "retina":      # level 0 four times, and that is not what (0, 1, 2, 3) gives
        assert all(pooled[:, j].tobytes() == pooled[:, 0].tobytes() for j in range(1, 4))
        other, _ = R.score_features(sd, feats, (0, 1, 2, 3))
        assert np.all(np.abs(other.astype(np.float64) - ref) > 2 * bound)


def test_pooling_restatement_within_bound_of_float64():
    rs = np.random.RandomState(3)
    for (H, W) in [(1, 1), (1, 5), (3, 85), (17, 31), (40, 52)]:
        x = (rs.randn(H, W, 256) + 0.7).astype(np.float32)
        err = np.abs(R.gap(x).astype(np.float64) - R.gap64(x))
        assert np.all(err <= R.gap_bound(x)), (H, W, float((err / R.gap_bound(x)).max()))
    x = rs.randint(-2, 3, (7, 75, 256)).astype(np.float32)      # exact sums: any order gives float32(sum) / float32(N)
    assert R.gap(x).tobytes() == (x.reshape(-1, 256).sum(axis=0, dtype=np.float64).astype(np.float32) / np.float32(525)).astype(np.float32).tobytes()


def test_fma32_is_correctly_rounded():
    from fractions import Fraction
    rs = np.random.RandomState(5)
    a = rs.randn(4000).astype(np.float32); b = rs.randn(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b).astype(np.float32) * (1 + rs.randint(-3, 4, 4000) * 2.0 ** -23)).astype(np.float32)      # heavy cancellation
    got = R.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i


def test_group_padding_is_the_groupwise_maximum_of_transform_size(oracle):
    from cald_amd.baselines import ll_group_padding
    sizes = [(375, 500), (500, 375), (333, 500), (500, 334), (480, 640), (427, 640), (100, 3000), (31, 37), (600, 600), (281, 500), (500, 500)]
    groups = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 5]
    for (mn, mx) in [(600, 1000), (800, 1333), (300, 500)]:
        own = [oracle.transform_size(H, W, mn, mx)[2:] for H, W in sizes]
        want = []
        for g in groups:
            members = [own[i] for i in range(len(sizes)) if groups[i] == g]
            want.append((max(m[0] for m in members), max(m[1] for m in members)))
        assert ll_group_padding(sizes, groups, mn, mx) == want
        assert ll_group_padding(sizes, list(range(len(sizes))), mn, mx) == own
    # the mix really pads: a portrait and a landscape image in one group both grow
    pads = ll_group_padding(sizes, groups, 600, 1000)
    assert oracle.transform_size(375, 500, 600, 1000)[2:] == (608, 800) and oracle.transform_size(500, 375, 600, 1000)[2:] == (800, 608)
    assert pads[0] == pads[1] and pads[0][0] >= 800 and pads[0][1] >= 800


def test_ll_get_uncertainty_fails_loudly_without_gpu(golden):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cald_amd import baselines, detector, synth
    sd, _ = fixture_case(golden("lossnet"))
    model = detector.fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=300, max_size=500)
    model.load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0))
    loader = [([torch.zeros(3, 40, 50), torch.zeros(3, 50, 40)], [None, None])]
    with pytest.raises(RuntimeError):
        baselines.ll_get_uncertainty(model, sd, loader)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


BATCH_SIZES = [4, 4, 3]


def _batch_scores(b):
    return np.array([0.125 + b + 0.01 * i for i in range(BATCH_SIZES[b])], np.float32).astype(np.float64)


def _row_worker(rank, world, port, q):
    import torch.distributed as dist
    from cald_amd import baselines, sweep
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    mine = [b for b in range(len(BATCH_SIZES)) if b % world == rank]
    rows = baselines.ll_pack_rows([_batch_scores(b) for b in mine], max(BATCH_SIZES))
    first, rest = sweep.allgather_scores(mine, rows[:, 0], rows[:, 1:], len(BATCH_SIZES))
    q.put((rank, baselines.ll_unpack_rows(first, rest)))
    dist.destroy_process_group()


def test_batch_rows_survive_the_allgather():
    """Batches of 4, 4 and 3 images over two gloo ranks: one NaN-padded row per loader batch, first column as `cons`, the rest as `cls`."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_row_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    want = np.concatenate([_batch_scores(b) for b in range(len(BATCH_SIZES))])
    for _, got in res:
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
