"""The RetinaNet SSM tail on the CPU: the restatement (tests/_retina_ssm_restatement.py) against the executed reference
(tests/golden/retina_ssm.npz, tools/make_golden_retina_ssm.py), the fixture's power to tell plausible wrong statements apart, the library's
host-only draw cald_ssm_pick_mt19937 against random.shuffle, the ssm.py wrapper around a stubbed sweep, and box_loss with RetinaNet's
scalar score.  Nothing here needs a GPU (the library loads without one).
"""
import ctypes as C
import random

import numpy as np
import pytest

import _retina_ssm_restatement as R

F32 = np.float32
MIN_IOU_MARGIN, MIN_P_MARGIN = 1e-4, 1e-5


def _case(fx, c):
    K = int(fx["c%d_K" % c]); Hp, Wp, Hr, Wr = [int(v) for v in fx["c%d_sizes" % c]]
    return dict(K=K, sizes=(Hp, Wp, Hr, Wr), thr=float(fx["c%d_thr" % c]), per=int(fx["c%d_per" % c]), seed=int(fx["c%d_seed" % c]),
                scores=fx["c%d_ref_scores" % c], dec=fx["c%d_ref_boxes" % c], counts=fx["c%d_counts" % c],
                picks=R.unpack_picks(fx["c%d_picks" % c], fx["c%d_n_picks" % c]), al=int(fx["c%d_al" % c]),
                boxes=fx["c%d_boxes" % c], rows_scores=fx["c%d_scores" % c], labels=fx["c%d_labels" % c], margins=fx["c%d_margins" % c],
                name=str(fx["names"][c]))


def _restate(case, picks, mutate=None):
    Hp, Wp, Hr, Wr = case["sizes"]
    return R.tail(case["scores"], case["dec"], picks, Hr, Wr, Hr, Wr, score_thr=case["thr"], per_class=case["per"], mutate=mutate)


def _same(got, case):
    return (got["al"] == case["al"] and np.array_equal(got["counts"], case["counts"]) and got["boxes"].shape == case["boxes"].shape
            and got["boxes"].tobytes() == case["boxes"].tobytes() and got["scores"].tobytes() == case["rows_scores"].tobytes()
            and got["labels"].shape == case["labels"].shape and np.array_equal(got["labels"], case["labels"]))


def test_fixture_holds_the_cases_and_their_margins(golden):
    fx = golden("retina_ssm")
    cases = [_case(fx, c) for c in range(int(fx["n"]))]
    assert [c["name"] for c in cases] == ["few", "voc", "al1", "many", "class0"]
    for c in cases:
        iou, thr, half = c["margins"]
        assert iou > MIN_IOU_MARGIN and thr > MIN_P_MARGIN and half > MIN_P_MARGIN, (c["name"], c["margins"])
    by = {c["name"]: c for c in cases}
    assert by["voc"]["K"] == 21 and by["voc"]["al"] == 0 and len(by["voc"]["boxes"]) > 0
    assert by["al1"]["al"] == 1 and len(by["al1"]["boxes"]) == 0 and by["al1"]["counts"].sum() == 0
    assert by["many"]["counts"].max() > R.TAKE and max(len(p) for p in by["many"]["picks"]) == R.TAKE
    assert by["class0"]["al"] == 0 and len(by["class0"]["labels"]) > 0 and (by["class0"]["labels"] == -1).all()
    assert (by["few"]["scores"] == F32(by["few"]["thr"])).sum() >= 1        # a score of exactly the threshold


def test_restatement_equals_the_executed_reference(golden):
    """Recorded picks in, recorded rows out: al, counts and labels exactly, boxes and scores bit for bit (the restatement selects and
    scales by 1.0 the reference's own float32 scores and decoded boxes).  The margins it measures are the fixture's, the NMS's at least."""
    fx = golden("retina_ssm")
    for c in range(int(fx["n"])):
        case = _case(fx, c)
        got = _restate(case, case["picks"])
        assert _same(got, case), case["name"]
        m = got["margins"]
        assert (m["thr"], m["half"]) == (case["margins"][1], case["margins"][2])
        assert m["iou"] >= case["margins"][0]         # the tool's pass runs past the cut at per_class: it met every pair this one meets


def test_restatement_draws_the_recorded_picks_from_the_recorded_seed(golden):
    """shuffle_pick is the reference's three lines: from the case's seed it leaves the picks the reference's shuffles left."""
    fx = golden("retina_ssm")
    state = random.getstate()
    try:
        for c in range(int(fx["n"])):
            case = _case(fx, c)
            random.seed(case["seed"])
            got = _restate(case, R.shuffle_pick)
            assert _same(got, case), case["name"]
            if case["al"] == 0:
                assert all(np.array_equal(a, b) for a, b in zip(got["picks"], case["picks"]))
            else:                                                        # al = 1 draws nothing
                assert random.getstate() == random.Random(case["seed"]).getstate()
    finally:
        random.setstate(state)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_fixture_tells_each_mutation_apart(golden, mutation):
    fx = golden("retina_ssm")
    state = random.getstate()
    differs = []
    try:
        for c in range(int(fx["n"])):
            case = _case(fx, c)
            random.seed(case["seed"])
            if not _same(_restate(case, R.shuffle_pick, mutate=mutation), case):
                differs.append(case["name"])
    finally:
        random.setstate(state)
    assert differs, "no fixture case notices the mutation %s" % mutation


# ---------------------------------------------------------------------------------------------------------------------------
# cald_ssm_pick_mt19937 against random.shuffle
# ---------------------------------------------------------------------------------------------------------------------------
NS = [0, 1, 2, 3, 255, 256, 257, 499, 500, 501, 5000, 65537]


def _c_pick(state, counts):
    from cald_amd import ssm
    return ssm._c_pick(state, counts)


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("n", NS)
def test_c_pick_equals_random_shuffle(seed, n):
    rng = random.Random(seed * 1000 + n)
    ver, words, gauss = rng.getstate()
    state = np.array(words, np.uint32)
    picks, n_picks = _c_pick(state, [n])
    x = list(range(n)); rng.shuffle(x)
    assert n_picks[0] == min(n, R.TAKE) and picks[0, :n_picks[0]].tolist() == x[:R.TAKE]
    assert tuple(int(v) for v in state) == rng.getstate()[1]
    twin = random.Random(); twin.setstate((ver, tuple(int(v) for v in state), gauss))
    assert twin.random() == rng.random()


@pytest.mark.parametrize("index", [0, 623, 624])
def test_c_pick_regenerates_inside_a_shuffle(index):
    """States whose index sits at 0, 623 and 624 (setstate accepts all of them): the 624-word regeneration falls inside the shuffle, at
    its very start, or after one word."""
    rng = random.Random(77)
    for _ in range(1000):
        rng.getrandbits(32)
    ver, words, gauss = rng.getstate()
    words = words[:624] + (index,)
    rng.setstate((ver, words, gauss))
    state = np.array(words, np.uint32)
    counts = [700, 3, 0, 1, 501]                                            # more than 624 draws in the first class alone
    picks, n_picks = _c_pick(state, counts)
    for k, n in enumerate(counts):
        x = list(range(n)); rng.shuffle(x)
        assert n_picks[k] == min(n, R.TAKE) and picks[k, :n_picks[k]].tolist() == x[:R.TAKE], (index, k)
    assert tuple(int(v) for v in state) == rng.getstate()[1]
    twin = random.Random(); twin.setstate((ver, tuple(int(v) for v in state), gauss))
    assert twin.random() == rng.random()


def test_c_pick_chains_the_classes_of_one_call():
    rng = random.Random(5)
    ver, words, gauss = rng.getstate()
    state = np.array(words, np.uint32)
    picks, n_picks = _c_pick(state, NS)
    for k, n in enumerate(NS):
        x = list(range(n)); rng.shuffle(x)
        assert n_picks[k] == min(n, R.TAKE) and picks[k, :n_picks[k]].tolist() == x[:R.TAKE], n
    assert tuple(int(v) for v in state) == rng.getstate()[1]


def test_c_pick_refuses_a_bad_state_or_count():
    from cald_amd import _ffi
    L = _ffi.lib()
    state = np.array(random.Random(1).getstate()[1], np.uint32)
    counts = np.array([3], np.int32); picks = np.zeros((1, R.TAKE), np.int32); n_picks = np.zeros(1, np.int32)
    args = (_ffi.ptr(counts, _ffi.c_i), _ffi.ptr(picks, _ffi.c_i), _ffi.ptr(n_picks, _ffi.c_i))
    assert L.cald_ssm_pick_mt19937(None, 0, 1, *args) != 0
    bad = state.copy(); bad[624] = 625
    assert L.cald_ssm_pick_mt19937(bad.ctypes.data, 0, 1, *args) != 0
    counts[0] = -1
    assert L.cald_ssm_pick_mt19937(state.ctypes.data, 0, 1, *args) != 0
    assert tuple(int(v) for v in state) == random.Random(1).getstate()[1]     # a refused call draws nothing


# ---------------------------------------------------------------------------------------------------------------------------
# the ssm.py wrapper around a stubbed sweep
# ---------------------------------------------------------------------------------------------------------------------------
def _stub_sweep(counts_per_image, seen):
    """What cald_sweep_ssm_retina does with its pick argument, without a GPU: one call per image."""
    from cald_amd import _ffi

    def run(pick, user):
        fn = C.cast(pick, _ffi.PICK_FN)
        for i, counts in enumerate(counts_per_image):
            cn = np.array(counts, np.int32); K = len(cn)
            picks = np.full((K, R.TAKE), -1, np.int32); n_picks = np.zeros(K, np.int32)
            assert fn(user, i, K, _ffi.ptr(cn, _ffi.c_i), _ffi.ptr(picks, _ffi.c_i), _ffi.ptr(n_picks, _ffi.c_i)) == 0
            seen.append([picks[k, :n_picks[k]].tolist() for k in range(K)])
        return "done"
    return run


@pytest.mark.parametrize("mode", ["c", "python"])
def test_wrapper_draws_from_the_global_generator_and_keeps_gauss_next(monkeypatch, mode):
    from cald_amd import _ffi, ssm
    if mode == "python":
        monkeypatch.setenv("CALD_SSM_PICK", "python")
    else:
        monkeypatch.delenv("CALD_SSM_PICK", raising=False)
        assert ssm._c_pick_checked()
    images = [[0, 1, 5, 700], [3, 3, 3, 3], [501, 0, 2, 40]]
    saved = random.getstate()
    try:
        random.seed(99)
        random.gauss(0, 1)                                  # leaves a cached second value: gauss_next is not None
        before = random.getstate()
        assert before[2] is not None
        want = []
        for counts in images:
            row = []
            for n in counts:
                x = list(range(n)); random.shuffle(x); row.append(x[:R.TAKE])
            want.append(row)
        after = random.getstate()
        tail = [random.randint(0, 1000) for _ in range(4)] + [random.gauss(0, 1)]
        random.setstate(before)
        seen, used = [], []
        run = _stub_sweep(images, seen)
        assert ssm._with_pick(lambda pick, user: (used.append((pick, user)), run(pick, user))[1]) == "done"
        assert seen == want
        assert random.getstate() == after and random.getstate()[2] == before[2]
        assert [random.randint(0, 1000) for _ in range(4)] + [random.gauss(0, 1)] == tail
        py_ptr = C.cast(ssm._python_pick, C.c_void_p).value
        c_ptr = C.cast(_ffi.lib().cald_ssm_pick_mt19937, C.c_void_p).value
        assert used[0][0].value == (py_ptr if mode == "python" else c_ptr)
        assert (used[0][1] is None) == (mode == "python")
    finally:
        random.setstate(saved)


def test_wrapper_puts_the_advanced_state_back_when_the_sweep_raises(monkeypatch):
    from cald_amd import ssm
    monkeypatch.delenv("CALD_SSM_PICK", raising=False)
    saved = random.getstate()
    try:
        random.seed(3)
        x = list(range(40)); random.shuffle(x); after = random.getstate()
        random.seed(3)
        seen = []
        run = _stub_sweep([[40]], seen)

        def failing(pick, user):
            run(pick, user)
            raise RuntimeError("the sweep failed after the draw")
        with pytest.raises(RuntimeError):
            ssm._with_pick(failing)
        assert seen == [[x]] and random.getstate() == after
    finally:
        random.setstate(saved)


def test_a_failed_self_check_selects_the_python_callback(monkeypatch):
    from cald_amd import ssm
    monkeypatch.delenv("CALD_SSM_PICK", raising=False)
    monkeypatch.setattr(ssm, "_C_PICK_OK", False)
    got = []
    ssm._with_pick(lambda pick, user: got.append((pick.value, user)))
    assert got == [(C.cast(ssm._python_pick, C.c_void_p).value, None)]


def test_python_pick_turns_an_exception_into_a_refusal():
    from cald_amd import _ffi, ssm
    cn = np.array([2], np.int32); n_picks = np.zeros(1, np.int32)
    assert ssm._python_pick(None, 0, 1, _ffi.ptr(cn, _ffi.c_i), None, _ffi.ptr(n_picks, _ffi.c_i)) == 1      # no picks array to write to


def test_retinanet_factory_and_arch_dispatch():
    from cald_amd import ssm
    m = ssm.retinanet_resnet50_fpn_ssm(num_classes=21, min_size=300, max_size=500)
    assert m.arch == 1 and m.cfg.detections_per_img == 50 and m.num_classes == 21 and m.box_min_size == 0.0
    assert ssm.retinanet_resnet50_fpn_ssm(num_classes=4, detections_per_img=7).cfg.detections_per_img == 7
    f = ssm.fasterrcnn_resnet50_fpn_ssm(num_classes=21)
    assert f.arch == 0 and f.box_min_size == 1e-2
    with pytest.raises(ValueError):
        ssm.retinanet_resnet50_fpn_ssm(num_classes=1)


# ---------------------------------------------------------------------------------------------------------------------------
# stage 2 with RetinaNet's scalar score
# ---------------------------------------------------------------------------------------------------------------------------
def test_box_loss_broadcasts_a_scalar_score_as_the_reference_does():
    """ssm_train.py:228-229 on RetinaNet: `score` is a 0-d float32 (allScore[i][j].cpu().numpy()), `label` K - 1 entries."""
    from cald_amd.ssm import box_loss
    for s in (0.05000001, 0.3, 0.5, 0.93, 1.0):
        score = np.float32(s)
        for label in ([1, -1, -1], [-1, -1, -1, -1], [1]):
            y = np.array(label)
            with np.errstate(divide="ignore", invalid="ignore"):
                want = -((1 + y) / 2 * np.log(score) + (1 - y) / 2 * np.log(1 - score + 1e-30))
            got = box_loss(score, label)
            assert got.shape == (len(label),) and got.dtype == want.dtype
            assert np.array_equal(got, want, equal_nan=True), (s, label)


def test_from_torch_module_reads_a_retina_ssm_module():
    """detection/retina_ssm.py's module has an `ssm` attribute and 50 detections a class; a module that states its own number keeps it."""
    from cald_amd.detector import from_torch_module

    class Fake:
        ssm = True
        score_thresh, nms_thresh = 0.05, 0.5

        def state_dict(self):
            return {"head.classification_head.cls_logits.weight": np.zeros((9 * 21, 256, 3, 3), F32)}
    m = from_torch_module(Fake())
    assert m.arch == 1 and m.num_classes == 21 and m.cfg.detections_per_img == 50
    Fake.detections_per_img = 80
    assert from_torch_module(Fake()).cfg.detections_per_img == 80
    del Fake.ssm, Fake.detections_per_img
    assert from_torch_module(Fake()).cfg.detections_per_img == 300              # detection/retinanet_cal.py's default, as before
