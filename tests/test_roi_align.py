"""The CPU half of the RoIAlign tests: the numpy restatement (tests/_roi_restatement.py) is pinned to the oracle on the constructed
cases (tests/_roi_cases.py), the oracle to a float64 evaluation within a derived bound, the replayed row walk to the gather indices
over an exhaustive family of 1-D profiles, and the cases to the full census of what the walk can do.  test_gpu_roi_align.py then
compares the kernels with the oracle on the same cases, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import _roi_cases as K
import _roi_restatement as R

F32 = np.float32
NAMES = ("a", "b")


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert not len(bad), (what, len(bad), bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's rows of each case at 260 channels, computed once and read-only"""
    out = {}
    for n in NAMES:
        c = K.case(n)
        out[n] = oracle.roi_align(c["feats"], c["rois"])
        out[n].setflags(write=False)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_oracle(oracle, want, name):
    c = K.case(name)
    assert np.isfinite(want[name]).all()
    _same(R.evaluate(c["feats"], c["rois"]), want[name], name)
    # the replayed walk multiplies the same pixels (C = 16 is enough: the indices do not depend on C)
    f16 = K.feats_at(c, 16)
    _same(R.evaluate(f16, c["rois"], plan="walk"), np.ascontiguousarray(want[name][:, :, :16]), name + " walk")


def test_restatement_equals_oracle_on_the_views(oracle):
    """every eighth RoI of every view (and all of the short ones) at 16 channels, and the level of every RoI"""
    vc = K.views_case()
    lib = oracle.lib()
    lib.orc_roi_level.restype = C.c_int
    for v in range(vc["V"]):
        rois = vc["rois"][v]
        for b in rois:
            assert R.roi_level(b) == lib.orc_roi_level(b.ctypes.data_as(C.POINTER(C.c_float))), (v, b)
        sub = rois if len(rois) < 100 else rois[::8]
        if len(sub):
            f = [np.ascontiguousarray(x[:, :, :16]) for x in vc["feats"][v]]
            _same(R.evaluate(f, sub), oracle.roi_align(f, sub), v)


def test_levels_equal_the_oracle_at_the_boundaries(oracle):
    """roi_level with the emulated fused multiply-adds against the oracle's C, on squares of side b (1 + k 2^-24), k = -40 .. 40, around every
    boundary b, and on every RoI of the cases; every level occurs, and the epsilon decides some box"""
    lib = oracle.lib()
    lib.orc_roi_level.restype = C.c_int
    boxes = [np.array([0, 0, F32(b * (1.0 + k * 2.0 ** -24)), F32(b * (1.0 + k * 2.0 ** -24))], F32) for b in K.BOUNDARIES for k in range(-40, 41)]
    boxes += [r for n in NAMES for r in K.case(n)["rois"]]
    levels = [R.roi_level(b) for b in boxes]
    assert levels == [lib.orc_roi_level(np.ascontiguousarray(b).ctypes.data_as(C.POINTER(C.c_float))) for b in boxes]
    for n in NAMES:
        c = K.case(n)
        lv = [R.roi_level(b) for b in c["rois"]]
        assert set(lv) == {0, 1, 2, 3} and set(lv[:c["n_cross"]]) == {0}
        assert any(R.roi_level(b) != R.roi_level(b, wrong=("no_level_eps",)) for b in c["rois"])


# one output = sum over 16 terms of (wy * wx) * v, / 4.  Roundings a term passes through in float32: the weight product (1), the product with
# the pixel (1), the three additions inside its sample (3), the four additions into the accumulator (4): 9.  The division by 4 is exact.  The
# float64 evaluation starts from the same float32 lo / hi / l / h, so the positions and 1-D weights carry no error of their own.  (The first
# accumulator addition, 0 + x, is exact: 8 real roundings, the ninth covers the second-order terms and the float64 sum's own error.)
N_ROUNDINGS = 9


@pytest.mark.parametrize("name", NAMES)
def test_oracle_within_the_float64_bound(want, name):
    c = K.case(name)
    val, mag = R.evaluate_f64(c["feats"], c["rois"])
    err = np.abs(want[name].astype(np.float64) - val)
    bound = N_ROUNDINGS * 2.0 ** -24 * mag
    bad = np.argwhere(err > bound)
    assert not len(bad), (name, bad[:4], err[tuple(bad[0])], bound[tuple(bad[0])])
    assert (mag > 0).mean() > 0.2          # the bound is 0 exactly where every sample of a bin is outside (RoIs far larger than a 3 x 3 map: most bins)
    assert (err[mag > 0] > 0).mean() > 0.5 # and the float32 rows do carry rounding error: the comparison is not of a sum with itself


@pytest.fixture(scope="module")
def family():
    """the exhaustive 1-D family: (size, start, extent) -> the 14 samples"""
    return {k: R.axis_samples(k[1], k[2], k[0]) for k in K.family()}


def _walk_equals_gather_1d(s, what):
    """Along one axis: the column a slot holds (rows: the register a sample row reads) is the sample's own lo / hi wherever that corner can
    carry a non-zero weight (a valid sample; lo with h != 0, hi with l != 0).  Rows and columns of walk_plan are independent of each
    other, so this, over every row profile and every column profile, is the statement for their full cross."""
    _, held = R.column_walk(s)
    for pw in range(7):
        for k, (cl, ch) in enumerate(((held[pw][0], held[pw][1]), (held[pw][2], held[pw][3]))):
            lo, hi, l, h, valid = s[2 * pw + k]
            assert not valid or ((h == 0 or cl == lo) and (l == 0 or ch == hi)), (what, "column", pw, k)
        _, first, second = R.row_pattern(s[2 * pw], s[2 * pw + 1])
        for k, (rl, rh) in enumerate((first, second)):
            lo, hi, l, h, valid = s[2 * pw + k]
            assert not valid or ((h == 0 or rl == lo) and (l == 0 or rh == hi)), (what, "row", pw, k)


def test_walk_plan_equals_the_gather_indices(family):
    for k, s in family.items():
        _walk_equals_gather_1d(s, k)
    for n in NAMES:
        c = K.case(n)
        for box in c["rois"]:
            l, sy, sx = R.roi_setup(box, c["level_hw"])
            w = R.weights(sy, sx)
            (wr, wc), (gr, gc) = R.walk_plan(sy, sx), R.gather_plan(sy, sx)
            assert np.array_equal(wr[w != 0], gr[w != 0]) and np.array_equal(wc[w != 0], gc[w != 0]), (n, box)


def test_census_of_the_family(family):
    """what the walk can do at all: 81 (slot, decision, pw), 32 decision tuples, 3 x 7 (pattern, ph); the two dead decisions never occur; a
    map of 3 pixels reaches all 81"""
    triples, tuples, patterns, by_size = set(), set(), set(), {}
    for (size, _, _), s in family.items():
        for pw, d in enumerate(R.column_walk(s)[0]):
            tuples.add(d)
            for slot, dec in zip(R.SLOTS, d):
                triples.add((slot, dec, pw))
                by_size.setdefault(size, set()).add((slot, dec, pw))
        patterns |= {(R.row_pattern(s[2 * ph], s[2 * ph + 1])[0], ph) for ph in range(7)}
    assert not {(s, d) for s, d, _ in triples} & R.UNREACHABLE
    assert triples == R.reachable_triples() and len(triples) == 81
    assert by_size[3] == triples
    assert len(tuples) == 32
    assert patterns == {(p, ph) for p in range(3) for ph in range(7)}


def test_census_of_the_cases(family):
    """the cases reach everything the family shows reachable, and every column decision inside every pattern's instantiation"""
    tuples = {d for s in family.values() for d in R.column_walk(s)[0]}
    seen = dict(patterns=set(), triples=set(), tuples=set(), crossed=set(), levels=set())
    for n in NAMES:
        c = K.case(n)
        for k, v in R.census(c["rois"], c["level_hw"]).items():
            seen[k] |= v
        first = R.census(c["rois"][:c["n_cross"]], c["level_hw"])
        assert first["triples"] == R.reachable_triples(), n              # level 0 alone, on 3 x 3 as on 9 x 7
        assert first["crossed"] == {(p,) + t for p in range(3) for t in R.reachable_triples()}, n
        assert first["patterns"] == {(p, ph) for p in range(3) for ph in range(7)}, n
    assert seen["triples"] == R.reachable_triples() and len(seen["triples"]) == 81
    assert seen["tuples"] == tuples and len(tuples) == 32
    assert seen["levels"] == {0, 1, 2, 3}


def test_named_edges_are_present():
    for n in NAMES:
        c = K.case(n)
        H, W = c["level_hw"][0]
        found = set()
        for axis, (profiles, size) in enumerate(((c["py"], H), (c["px"], W))):
            for start, ext in profiles:
                start, ext = F32(start), F32(F32(F32(start) + F32(ext)) - F32(start))
                s = R.axis_samples(start, ext, size)
                b = F32(max(ext, F32(1.0)) / F32(7.0))
                t = [float(F32(F32(start + F32(F32(k >> 1) * b)) + F32(F32(F32(F32(k & 1) + F32(0.5)) * b) / F32(2.0)))) for k in range(14)]
                for k in range(14):
                    lo, hi, l, h, valid = s[k]
                    if -1.0 <= t[k] < 0.0:
                        assert valid and (lo, float(l), float(h)) == (0, 0.0, 1.0)
                        found.add((axis, "in [-1, 0): all weight on pixel 0"))
                    if t[k] == size:
                        assert valid and lo == hi == size - 1 and l == 0
                        found.add((axis, "t == size"))
                    if size < t[k] <= size + 2 * np.spacing(F32(size)):
                        assert not valid
                        found.add((axis, "one ulp beyond"))
                    if valid and lo == hi and size > 1:
                        found.add((axis, "clamp"))
                if not any(x[4] for x in s):
                    found.add((axis, "all outside"))
                if ext == 0:
                    found.add((axis, "zero extent"))
                if ext >= 7 * size:
                    found.add((axis, "far larger than the map"))
        need = {"in [-1, 0): all weight on pixel 0", "t == size", "clamp", "all outside", "zero extent"} | \
               ({"one ulp beyond"} if n == "b" else {"far larger than the map"})       # 7 times the 3 x 3 map; 3 + 1 ulp has no exact profile
        assert found >= {(a, e) for a in (0, 1) for e in need}, (n, found)
        assert [0.0, 0.0] in (c["rois"][:, 2:] - c["rois"][:, :2]).tolist()          # zero area: the cross of the two zero extents


def test_split_words_join_equals_the_oracle_requantize(oracle, want):
    """on the rows of the cases and on values around every edge of the two fp16 conversions: halves, subnormals, the smallest ones, ties"""
    rs = np.random.RandomState(3)
    x = ((1.0 + rs.rand(4096)) * 2.0 ** rs.randint(-40, 12, 4096) * rs.choice([-1.0, 1.0], 4096)).astype(F32)
    edge = np.array([0.0, -0.0, 2.0 ** -18, 2.0 ** -28, 2.0 ** -29, 3 * 2.0 ** -29, 2.0 ** -30, (1 + 2.0 ** -11) / 16, (1 + 3 * 2.0 ** -11) / 16, 4000.0, -4000.0,
                     2.0 ** -18 * (1 - 2.0 ** -12), 2.0 ** -19 * (1 + 2.0 ** -10)], F32)
    x = np.concatenate([x, edge, np.zeros(-(len(x) + len(edge)) % 16, F32)])
    for a in (x.reshape(-1, 16), want["a"][:, :, :256], want["b"][:, :, :256]):
        _same(R.join(R.split_words(a)), oracle.f16x3_requantize(a), "join(split)")
    w = R.split_words(np.arange(32, dtype=F32).reshape(1, 32) / 16)          # the layout: hi halves of 16 channels, then their lo halves
    assert w.view(np.uint16).reshape(2, 2, 16)[:, 0].view(np.float16).ravel().tolist() == list(range(32))
    assert not w.view(np.uint16).reshape(2, 2, 16)[:, 1].any()
    sub = want["a"][:, :, :256]
    assert ((np.abs(sub) * 16 < 2.0 ** -14) & (sub != 0)).any()              # 16 x an fp16 subnormal among the expected rows


@pytest.mark.parametrize("mistake", R.WRONG)
def test_each_mistake_changes_an_expected_output(want, mistake):
    """the cases notice every deliberate mistake of the restatement: some expected row differs (the walk's mistakes through walk_plan)"""
    if mistake == "split_lo_from_x":
        a = want["a"][:, :, :256]
        assert not np.array_equal(R.split_words(a, wrong=(mistake,)), R.split_words(a))
        return
    plan = "walk" if mistake in ("l0_ignores_phi", "l1_alias_l0", "h1_alias_l1", "pat1_rows01", "pat2_on_r0") else "gather"
    for n in NAMES:
        c = K.case(n)
        f = K.feats_at(c, 16)
        for r, box in enumerate(c["rois"]):
            if R.evaluate(f, box[None], wrong=(mistake,), plan=plan).tobytes() != want[n][r, :, :16].tobytes():
                return
    pytest.fail("no case notices " + mistake)


def test_roi_order_restatement():
    """ties by descending index, the clamps of the key"""
    vc = K.views_case()
    n = K.VIEW_COUNTS[K.TIE_VIEW]
    assert len({R.order_key(b) for b in vc["rois"][K.TIE_VIEW]}) == 1
    assert R.roi_order(vc["rois"][K.TIE_VIEW]).tolist() == list(range(n - 1, -1, -1))
    keys = [R.order_key(b) for b in vc["rois"][K.CLAMP_VIEW]]
    assert keys[:5] == [4095, 4095, (1023 << 12) | 2, (1023 << 12) | 2, 0] and keys[5] == keys[6] == 1
    assert R.roi_order(vc["rois"][K.CLAMP_VIEW]).tolist() == [4, 6, 5, 1, 0, 3, 2]
    for v in range(vc["V"]):
        assert sorted(R.roi_order(vc["rois"][v]).tolist()) == list(range(K.VIEW_COUNTS[v]))
