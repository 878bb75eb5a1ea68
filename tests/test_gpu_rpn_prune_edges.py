"""The DECISIONS of the certified RPN pruning (rpn_prune.hip: prune_select_kernel<1>, <2>, prune_scatter_kernel), outside any model, through
cald_op_rpn_prune, against tests/_prune_restatement.py -- and the sweep's ratio tripwire (sweep.hip sweep_checked), fired once.

Method.  Every value the three kernels compute is a short, fixed sequence of float32 operations (no contraction; sqrt and division are
correctly rounded), which numpy float32 restates operation by operation.  So every output is compared BYTE FOR BYTE, no tolerance:
pnorm, tau_key, nsel, both row_maps, the final head maps, check[2] and the profile counters.  Every in / out array is handed over filled
with sentinels (unused row_map slots, guard words past every array, channels 3.. of the look-ahead map) and must come back with the
sentinels in place.  The inputs are dyadic rationals of a few bits wherever a case's point is a tie or a threshold; what each case
assumes about its own data (rank k inside a tie, tau' above or below tau, the float32 patch norm against the float64 one, ...) is
asserted on the restatement's result first, in the CPU half that runs without a GPU as well.

One reading of the issue's list is fixed here: a look-ahead logit of -inf has the upper bound -inf and is parked like any anchor below the
threshold (rpn_prune.hip's header: a non-finite ACTIVATION is the range tripwire's business, through the patch norm); NaN and +inf logits
are kept by construction and the test asserts it.

What no case here can see: the scatter's `worst > 0.0f` guard.  With worst == +0.0 the word test behind it, `*ck < 0u`, is never true, so
the guard decides nothing for ratios >= 0 (it only keeps a -0.0 out, which would hang on fmaxf's choice between +0.0 and -0.0).
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import _prune_restatement as R

F32 = np.float32
GUARD = 5
S_F32 = F32(-7.0e33)            # sentinels of the in / out arrays: no case computes these values
S_I32 = np.int32(-77777)
S_U32 = np.uint32(0xDEADBEEF)


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from cald_amd import _ffi, detector
    return dict(L=_ffi.lib(), ffi=_ffi, ctx=detector.get_ctx(0), det=detector, torch=torch)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def _pix(hw):
    return [sum(h * w for h, w in lv) for lv in hw]


def _case(hw, pre_n, seed=0, c1=(2.0 ** -6,) * 3, c0=(2.0 ** -4,) * 3, ld=15, check=(0.0, 0.0), err=8):
    """A generic case: energies k / 4 (k < 64: every sum exact), look-ahead logits k / 256 in (-16, 16), exact logits = look + e / 4096
    (|e| <= err: ratios of a few percent), channels 3.. distinct values on both maps."""
    hw = [list(map(tuple, hw[0])), list(map(tuple, hw[1]))]
    assert len(hw[0]) == len(hw[1])
    rs = np.random.RandomState(seed)
    case = dict(V=len(hw[0]), hw=hw, pre_n=pre_n, ld=ld, c1=np.array(c1, F32), c0=np.array(c0, F32), check=np.array(check, F32),
                energy=[], look=[], exact=[])
    for l, n in enumerate(_pix(hw)):
        case["energy"].append((rs.randint(0, 64, (n, 4)) / 4.0).astype(F32))
        look = np.empty((n, ld), F32); exact = np.empty((n, ld), F32)
        look[:, :3] = rs.randint(-4095, 4096, (n, 3)) / 256.0
        exact[:, :3] = look[:, :3] + (rs.randint(-err, err + 1, (n, 3)) / 4096.0).astype(F32)
        look[:, 3:] = -(1000.0 + np.arange(n * (ld - 3)).reshape(n, ld - 3) % 4096 + l)         # the look-ahead's channels 3..: sentinels
        exact[:, 3:] = 0.25 + 0.5 * (np.arange(n * (ld - 3)).reshape(n, ld - 3) % 8192)
        case["look"].append(look); case["exact"].append(exact)
    return case


def _views(case, l):
    off = 0
    for v, (h, w) in enumerate(case["hw"][l]):
        yield v, off, h * w
        off += h * w


CASES = {}


def case(fn):
    CASES[fn.__name__[2:]] = fn
    return fn


# ---- geometry ----
@case
def c_geo_1x1():
    return _case([[(1, 1)], [(1, 1)]], 2), None


@case
def c_geo_1xW():
    return _case([[(1, 37)], [(1, 5)]], 10, seed=1), None


@case
def c_geo_Hx1():
    return _case([[(41, 1)], [(3, 1)]], 10, seed=2), None


def _npx_case(shape, seed):
    return _case([[shape], [(2, 3)]], 40, seed=seed)


@case
def c_geo_npx31():
    return _npx_case((1, 31), 3), None


@case
def c_geo_npx32():
    return _npx_case((4, 8), 4), None


@case
def c_geo_npx33():
    return _npx_case((3, 11), 5), None


@case
def c_geo_npx1023():
    return _npx_case((33, 31), 6), None


@case
def c_geo_npx1025():
    return _npx_case((25, 41), 7), None


def _rounds(words):
    def chk(c, r):
        npx = c["hw"][0][0][0] * c["hw"][0][0][1]
        assert (npx + 31) // 32 == words
        for s in range(2):          # selected pixels in the first and in the last compaction round of both stages
            idx = r["row_map"][s][0][0][1]
            assert idx.size and idx[0] < 32768 and idx[-1] >= ((words - 1) // 1024) * 32768, s
    return chk


@case
def c_geo_two_compaction_rounds():
    """150 x 221: 1036 mask words, a second round of 12 words."""
    return _case([[(150, 221)], [(7, 9)]], 3000, seed=8), _rounds(1036)


@case
def c_geo_three_compaction_rounds():
    """200 x 334: 2088 mask words, three rounds; enough rows that every thread of the scatter loops (checked below)."""
    c = _case([[(200, 334)], [(6, 5)]], 2000, seed=9)

    def chk(c, r):
        _rounds(2088)(c, r)
        assert r["nsel"][:, 0, 0].max() * c["ld"] > 64 * 256          # the scatter's grid is capped at 64 blocks of 256
    return c, chk


@case
def c_geo_ragged():
    """V = 3, the middle view 2 x 3 (all kept: 18 anchors <= pre_n) between larger ones."""
    c = _case([[(37, 53), (2, 3), (60, 70)], [(5, 5), (2, 3), (9, 4)]], 50, seed=10)

    def chk(c, r):
        assert r["nsel"][0, 0, 1] == 6 and r["nsel"][1, 0, 1] == 0 and r["tau_key"][0, 1] == 0
        assert 0 < r["nsel"][0, 0, 2] < 4200 and r["nsel"][1, 0, 2] > 0
    return c, chk


@case
def c_geo_level1_larger():
    return _case([[(5, 7)], [(40, 45)]], 30, seed=11), None


@case
def c_geo_distinct_neighbours():
    """3 x 4 pixels with total energies 2^i in quarters (1/2, 1/4, 1/8, 1/8): every subset sum of the nine neighbours is exact and distinct,
    a dropped or doubled term changes the bits."""
    c = _case([[(3, 4)], [(4, 3)]], 5, seed=12)
    for l in range(2):
        t = 2.0 ** np.arange(12)
        c["energy"][l] = np.stack([t / 2, t / 4, t / 8, t / 8], axis=1).astype(F32)

    def chk(c, r):
        H, W = c["hw"][0][0]
        t = 2.0 ** np.arange(12).reshape(H, W)
        for y in range(H):
            for x in range(W):
                s = sum(t[yy, xx] for yy in range(max(0, y - 1), min(H, y + 2)) for xx in range(max(0, x - 1), min(W, x + 2)))
                assert r["pnorm"][0][y * W + x] == F32(np.sqrt(F32(s)) * F32(1.0001))
    return c, chk


# ---- the k boundary ----
def _k_case(pre_n, seed=20):
    c = _case([[(6, 7)], [(7, 6)]], pre_n, seed=seed)          # 42 pixels, 126 anchors on both levels

    def chk(c, r):
        if pre_n >= 126:            # everything kept by stage 0: tau = 0, stage 1 selects nothing and parks nothing
            assert (r["tau_key"] == 0).all() and (r["nsel"][0] == 42).all() and (r["nsel"][1] == 0).all()
            assert not (r["head"][0][:, :3] == -R.FLT_MAX).any() and not (r["head"][1][:, :3] == -R.FLT_MAX).any()
        else:
            assert (r["tau_key"] != 0).all()
    return c, chk


@case
def c_k_n_minus_1():
    return _k_case(125)


@case
def c_k_n():
    return _k_case(126)


@case
def c_k_n_plus_1():
    return _k_case(127)


@case
def c_k_one():
    c, _ = _k_case(1)

    def chk(c, r):
        assert (r["nsel"][0] == 1).all()          # the one largest lower bound is unique in this data
    return c, chk


# ---- keys ----
@case
def c_key_ties_across_rank_k():
    """Integer logits, zero energy (constant norm 0, B = c0 = 1/2): 300 lower bounds in five groups of exact ties, rank k inside one."""
    c = _case([[(10, 10)], [(10, 10)]], 100, seed=30, c0=(0.5,) * 3)
    rs = np.random.RandomState(30)
    for l in range(2):
        c["energy"][l][:] = 0
        c["look"][l][:, :3] = rs.randint(-2, 3, (100, 3))
        c["exact"][l][:, :3] = c["look"][l][:, :3]

    def chk(c, r):
        for l in range(2):
            lb = (c["look"][l][:, :3] - F32(0.5)).reshape(-1)
            tau = np.sort(lb)[::-1][99]
            assert 1 < (lb > tau).sum() < 100 < (lb >= tau).sum() - 12          # dozens of ties straddle rank k
            assert r["tau_key"][l, 0] == R.orderable(np.array([tau], F32))[0]
            assert np.array_equal(r["keep"][0][l][0], (c["look"][l][:, :3] - F32(0.5) >= tau).any(axis=1))     # every tie is kept
    return c, chk


@case
def c_key_signed_zeros_at_rank_k():
    """B = 0 (c1 = c0 = 0): the lower bounds ARE the logits, +0.0 and -0.0 among them with rank k inside the zeros.  Unfolded, the k-th key
    would be -0.0's (0x7FFFFFFF) and the +0.0 / -0.0 pixels would part.  (B = 0 makes every ratio x / 0: check[0] = inf.)"""
    c = _case([[(8, 8)], [(8, 8)]], 60, seed=31, c1=(0.0,) * 3, c0=(0.0,) * 3)
    for l in range(2):
        lg = np.full(192, -1.0, F32)
        lg[:30] = 1.0; lg[30:50] = 0.0; lg[50:90] = -0.0           # descending: 30 ones, 20 x +0.0, 40 x -0.0, the rest -1: rank 60 is a -0.0
        c["look"][l][:, :3] = np.random.RandomState(31 + l).permutation(lg).reshape(64, 3)
        c["exact"][l][:, :3] = c["look"][l][:, :3]

    def chk(c, r):
        assert (r["tau_key"] == 0x80000000).all() and np.isinf(r["check"][0])
        for l in range(2):
            assert np.array_equal(r["keep"][0][l][0], (c["look"][l][:, :3] >= 0).any(axis=1))
    return c, chk


@case
def c_key_all_negative():
    c = _case([[(9, 11)], [(5, 6)]], 25, seed=32)
    for l in range(2):
        c["look"][l][:, :3] -= 100.0; c["exact"][l][:, :3] -= 100.0
    return c, None


def _bits_case(bits_of, seed):
    """logits with the given bit patterns, zero energy, B = c0."""
    def make(c0):
        c = _case([[(16, 16)], [(16, 16)]], 300, seed=seed, c0=(c0,) * 3)
        for l in range(2):
            c["energy"][l][:] = 0
            c["look"][l][:, :3] = bits_of(np.random.RandomState(seed + l)).astype(np.uint32).view(F32).reshape(256, 3)
            c["exact"][l][:, :3] = c["look"][l][:, :3]
        return c
    return make


@case
def c_key_lowest_byte():
    """logits 3 + r 2^-22, B = 2^-14 = 256 ulp: the keys of both bounds differ in their lowest byte only (passes 0..2 see one bin)."""
    c = _bits_case(lambda rs: 0x40400000 + rs.randint(0, 256, 768), 33)(2.0 ** -14)

    def chk(c, r):
        for l in range(2):
            lb = R.orderable((c["look"][l][:, :3] - F32(2.0 ** -14)).astype(F32)).reshape(-1)
            assert len(set(int(x) >> 8 for x in lb)) == 1 and len(set(int(x) & 255 for x in lb)) > 200
    return c, chk


@case
def c_key_highest_byte():
    """positive logits with the bit patterns (b << 24) | 0x400000, 0x3B <= b < 0x47, B = 0: the keys differ in their highest byte only."""
    tops = np.arange(0x3B, 0x47, dtype=np.int64)
    c = _bits_case(lambda rs: (tops[rs.randint(0, 12, 768)] << 24) | 0x400000, 34)(0.0)
    c["c1"][:] = 0

    def chk(c, r):
        for l in range(2):
            k = R.orderable(c["look"][l][:, :3]).reshape(-1)
            assert len(set(int(x) & 0xFFFFFF for x in k)) == 1 and len(set(int(x) >> 24 for x in k)) == 12
    return c, chk


@case
def c_key_bin_0():
    """the k-th largest lower bound is below -1.7e38 (key < 2^24: histogram bin 0 of the first pass)."""
    c = _case([[(12, 12)], [(12, 12)]], 100, seed=35)
    for l in range(2):
        rs = np.random.RandomState(35 + l)
        lg = -(2.0e38 + 1.0e34 * rs.permutation(432)).astype(F32)
        lg[rs.choice(432, 90, replace=False)] = rs.randint(-100, 100, 90)
        c["look"][l][:, :3] = lg.reshape(144, 3); c["exact"][l][:, :3] = c["look"][l][:, :3]

    def chk(c, r):
        assert (r["tau_key"] >> 24 == 0).all() and (r["tau_key"] != 0).all()
    return c, chk


@case
def c_key_bin_255():
    """the k-th largest lower bound is above 1.7e38 (bin 255); some are +inf."""
    c = _case([[(12, 12)], [(12, 12)]], 100, seed=36)
    for l in range(2):
        rs = np.random.RandomState(36 + l)
        lg = rs.randint(-100, 100, 432).astype(F32)
        big = rs.choice(432, 150, replace=False)
        lg[big] = (2.0e38 + 1.0e34 * rs.permutation(150)).astype(F32)
        lg[big[:20]] = np.inf
        c["look"][l][:, :3] = lg.reshape(144, 3); c["exact"][l][:, :3] = c["look"][l][:, :3]

    def chk(c, r):
        assert (r["tau_key"] >> 24 == 255).all()
        assert np.isinf(r["check"][0])             # inf - inf at the selected +inf anchors
    return c, chk


# ---- per-anchor constants ----
@case
def c_anchor_constants():
    c = _case([[(20, 20)], [(13, 17)]], 150, seed=40, c1=(2.0 ** -9, 2.0 ** -5, 2.0 ** -2), c0=(2.0 ** -7, 0.5, 3.0))

    def chk(c, r):
        for perm in itertools.permutations(range(3)):
            if perm == (0, 1, 2):
                continue
            c2 = dict(c, c1=c["c1"][list(perm)], c0=c["c0"][list(perm)])
            r2 = R.run(c2)
            for l in range(2):
                assert not np.array_equal(r2["keep"][0][l][0], r["keep"][0][l][0]), perm
                assert not np.array_equal(r2["keep"][0][l][0] | r2["keep"][1][l][0], r["keep"][0][l][0] | r["keep"][1][l][0]), perm
        c2 = dict(c, c1=np.repeat(c["c1"][:1], 3), c0=np.repeat(c["c0"][:1], 3))
        assert not np.array_equal(R.run(c2)["keep"][0][0][0], r["keep"][0][0][0])
    return c, chk


# ---- stage 1's threshold ----
@case
def c_stage1_tau_prime_wins():
    """exact ~ look: the k-th exact logit lies about one bound above the k-th lower bound; the band is one bound wide."""
    c = _case([[(30, 40), (20, 25)], [(15, 20), (16, 18)]], 200, seed=50, c0=(0.5,) * 3)

    def chk(c, r):
        assert (r["thr_key"] > r["tau_key"]).all()
        assert (r["nsel"][1] > 0).all()
        for l in range(2):
            for v in range(2):
                k0, k1 = r["keep"][0][l][v], r["keep"][1][l][v]
                assert (~k0 & ~k1).any()
                # with tau alone as stage 1's threshold more pixels would be selected: tau' is what the kept set shows
                off = sum(h * w for h, w in c["hw"][l][:v]); n = k0.size
                B = R.bound(r["pnorm"][l][off:off + n], c["c1"], c["c0"])
                wide = ~k0 & (R.orderable((c["look"][l][off:off + n, :3] + B).astype(F32)) >= r["tau_key"][l, v]).any(axis=1)
                assert wide.sum() > k1.sum()
    return c, chk


@case
def c_stage1_tau_wins_and_ratio_above_1():
    """exact = look - 50: tau' lies far below tau and stage 0's threshold must win; every ratio is far above 1."""
    c = _case([[(30, 40), (20, 25)], [(15, 20), (16, 18)]], 200, seed=51, c0=(0.5,) * 3)
    for l in range(2):
        c["exact"][l][:, :3] = c["look"][l][:, :3] - F32(50.0)

    def chk(c, r):
        assert (r["thr_key"] == r["tau_key"]).all() and (r["nsel"][1] > 0).all()
        assert 50.0 < r["check"][0] < np.inf
        for l in range(2):
            for v, off, n in _views(c, l):
                kex = R.orderable(c["exact"][l][off:off + n, :3][r["keep"][0][l][v]])
                assert R.kth_largest(kex, 200) < r["tau_key"][l, v]
    return c, chk


# ---- non-finite ----
@case
def c_nonfinite_look():
    """NaN, +inf and -inf look-ahead logits.  NaN and +inf are kept (stage 0); -inf has the upper bound -inf and is parked unless its pixel
    holds another anchor that stays (the module docstring)."""
    c = _case([[(14, 15)], [(8, 9)]], 60, seed=60)
    spots = {}
    for l in range(2):
        rs = np.random.RandomState(60 + l)
        px = rs.choice(c["look"][l].shape[0], 9, replace=False)
        for i, val in enumerate([np.nan, np.inf, -np.inf] * 3):
            c["look"][l][px[i], i % 3] = val
            c["look"][l][px[i], (i + 1) % 3] = -15.5              # the pixel's other anchors are hopeless: the special one decides
            c["look"][l][px[i], (i + 2) % 3] = -15.5
        spots[l] = px

    def chk(c, r):
        for l in range(2):
            k0, k1 = r["keep"][0][l][0], r["keep"][1][l][0]
            for i, p in enumerate(spots[l]):
                if i % 3 < 2:
                    assert k0[p], (l, i)                          # NaN, +inf: selected by stage 0, never parked
                else:
                    assert not k0[p] and not k1[p] and (r["head"][l][p, :3] == -R.FLT_MAX).all()
        assert np.isinf(r["check"][0])                            # look NaN against a finite exact value: NaN ratio -> inf
    return c, chk


@case
def c_nonfinite_exact_nan():
    """one exact NaN at a selected anchor (the largest look-ahead logit of level 1): check[0] == inf, nothing else non-finite."""
    c = _case([[(14, 15)], [(8, 9)]], 60, seed=61)
    p, a = np.unravel_index(np.argmax(c["look"][1][:, :3]), (72, 3))
    c["exact"][1][p, a] = np.nan

    def chk(c, r):
        assert r["keep"][0][1][0][p] and np.isinf(r["check"][0])
    return c, chk


@case
def c_nonfinite_inf_minus_inf():
    c = _case([[(14, 15)], [(8, 9)]], 60, seed=62)
    c["look"][0][17, 1] = np.inf; c["exact"][0][17, 1] = np.inf

    def chk(c, r):
        assert r["keep"][0][0][0][17] and np.isinf(r["check"][0])
    return c, chk


# ---- the range flag ----
RANGE_BELOW, RANGE_ABOVE = 16757482.0, 16757483.0       # energy sums whose float32 patch norm is 4093.9998 / 4094.0 (found with the restatement)


def _range_case(value, flagged, pre_n=20):
    c = _case([[(5, 6)], [(3, 3)]], pre_n, seed=70)
    for l in range(2):
        c["energy"][l][:] = 0
    c["energy"][1][4] = [value, 0, 0, 0]                   # the centre of level 1's 3 x 3 view: every pixel's patch holds it

    def chk(c, r):
        assert r["check"][1] == (1.0 if flagged else 0.0)
        assert not (r["pnorm"][0] != 0).any()
    return c, chk


@case
def c_range_just_below():
    c, chk = _range_case(RANGE_BELOW, False)

    def chk2(c, r):
        chk(c, r)
        assert (r["pnorm"][1] == F32(4093.9998)).all() and F32(4093.9998) < F32(4094.0)
    return c, chk2


@case
def c_range_just_above():
    c, chk = _range_case(RANGE_ABOVE, True)

    def chk2(c, r):
        chk(c, r)
        assert (r["pnorm"][1] == F32(4094.0)).all()
    return c, chk2


@case
def c_range_inf_energy():
    return _range_case(np.inf, True)


@case
def c_range_nan_energy():
    """Every bound of level 1 is NaN here, and the sign of a NaN that sqrt produces is the one thing numpy and the device need not agree on
    (a key of +NaN sorts above +inf, one of -NaN below -inf).  So the view keeps everything (27 anchors <= pre_n, tau = 0) and no output
    hangs on it: the case is about the flag and about NaN bounds being kept, not about where NaN sorts."""
    return _range_case(np.nan, True, pre_n=30)


# ---- the scatter ----
def _scatter_case(check0, zero=False, seed=80):
    c = _case([[(21, 23), (9, 9)], [(10, 12), (12, 13)]], 90, seed=seed, c0=(0.5,) * 3, check=(check0, 0.0))
    if zero:
        for l in range(2):
            c["exact"][l][:, :3] = c["look"][l][:, :3]
    return c


@case
def c_scatter_worst_in_last_element():
    """all ratios a few percent, but 1/2 at channel 2 of the last row selected by stage 1 on level 1 of the last view."""
    c = _scatter_case(0.0)
    r0 = R.run(c)
    off, idx = r0["row_map"][1][1][-1]
    assert idx.size and r0["worst"] < 0.1
    p = off + idx[-1]
    B = R.bound(r0["pnorm"][1][p:p + 1], c["c1"], c["c0"])[0, 2]
    c["exact"][1][p, 2] = c["look"][1][p, 2] + B * F32(0.5)

    def chk(c, r):
        assert np.array_equal(r["row_map"][1][1][-1][1], idx)            # a stage-1 pixel's exact logit decides nothing
        assert 0.49 < r["check"][0] < 0.51 and r["worst"] > 5 * r0["worst"]
    return c, chk


@case
def c_scatter_all_zero_initial_zero():
    c = _scatter_case(0.0, zero=True)
    return c, lambda c, r: np.testing.assert_array_equal(r["check"].view(np.uint32), [0, 0])


@case
def c_scatter_all_zero_initial_kept():
    c = _scatter_case(0.3, zero=True)
    return c, lambda c, r: np.testing.assert_array_equal(r["check"].view(np.uint32), np.array([0.3, 0], F32).view(np.uint32))


@case
def c_scatter_initial_larger():
    c = _scatter_case(0.75)
    return c, lambda c, r: np.testing.assert_array_equal(r["check"], np.array([0.75, 0], F32))


@case
def c_scatter_initial_smaller():
    c = _scatter_case(2.0 ** -20)

    def chk(c, r):
        assert 2.0 ** -12 < r["check"][0] < 0.1 and r["check"][0] == r["worst"]
    return c, chk


@case
def c_scatter_grid_stride():
    """half of all anchors wanted: stage 0 alone selects far more than a quarter of the pixels, the share at which each thread of the scatter's
    grid (a thread for four elements of the largest view) starts a second trip."""
    c = _case([[(40, 50)], [(20, 25)]], 3000, seed=81)

    def chk(c, r):
        bx = (2000 * c["ld"] + 1023) // 1024
        assert bx <= 64 and r["nsel"][0, 0, 0] * c["ld"] > 2 * bx * 256
    return c, chk


@case
def c_head_ld_other():
    """head_ld = 4 (and 3 on the ragged twin below): the row stride is no constant of the kernels."""
    return _case([[(17, 19), (3, 2)], [(8, 9), (4, 4)]], 70, seed=90, ld=4), None


@case
def c_head_ld_3():
    return _case([[(17, 19)], [(8, 9)]], 70, seed=91, ld=3), None


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name):
    """(case, restatement's result), computed once; the case's own assumptions checked on it."""
    c, chk = CASES[name]()
    r = R.run(c)
    for l in range(2):          # the certificate needs pnorm >= the true norm: the 1.0001 pays for float32's rounding of the sum
        ok = np.isfinite(r["pnorm64"][l])
        assert (r["pnorm"][l][ok].astype(np.float64) >= r["pnorm64"][l][ok]).all(), name
        assert not (r["pnorm"][l][~ok] < R.RANGE).any()
        for v in range(c["V"]):     # a pixel kept in stage 0 never reappears in stage 1
            assert not (r["keep"][0][l][v] & r["keep"][1][l][v]).any()
    if chk:
        chk(c, r)
    return c, r


@pytest.mark.parametrize("name", sorted(CASES))
def test_prune_restatement_assumptions_hold(name):
    """CPU half: what each case's docstring claims about its data holds on the restatement's own result."""
    _reference(name)


def test_range_pair_brackets_4094():
    lo, _ = R.patch_norm(np.array([[RANGE_BELOW, 0, 0, 0]], F32), 1, 1)
    hi, _ = R.patch_norm(np.array([[RANGE_ABOVE, 0, 0, 0]], F32), 1, 1)
    assert lo[0] < R.RANGE and not (hi[0] < R.RANGE) and F32(RANGE_ABOVE) == np.nextafter(F32(RANGE_BELOW), F32(np.inf))


def _run_gpu(hip, c):
    ffi, L = hip["ffi"], hip["L"]
    V, ld = c["V"], c["ld"]
    pix = _pix(c["hw"])
    p = ffi.RpnPruneProbe()
    p.V = V; p.guard = GUARD; p.pre_n = c["pre_n"]; p.head_ld = ld
    for l in range(2):
        for v, (h, w) in enumerate(c["hw"][l]):
            p.hw[l][v][0] = h; p.hw[l][v][1] = w
    for a in range(3):
        p.c1[a] = c["c1"][a]; p.c0[a] = c["c0"][a]
    p.check[0] = c["check"][0]; p.check[1] = c["check"][1]
    u32, i32 = C.POINTER(C.c_uint32), ffi.c_i
    keep = dict(energy=[np.ascontiguousarray(e, F32) for e in c["energy"]], exact=[np.ascontiguousarray(e, F32) for e in c["exact"]],
                head=[np.concatenate([c["look"][l], np.full((GUARD, ld), S_F32, F32)]) for l in range(2)],
                pnorm=[np.full(pix[l] + GUARD, S_F32, F32) for l in range(2)],
                tau_key=np.full(2 * V + GUARD, S_U32, np.uint32),
                row_map=[[np.full(pix[l] + GUARD, S_I32, np.int32) for l in range(2)] for _ in range(2)],
                nsel=[np.full(2 * V + GUARD, S_I32, np.int32) for _ in range(2)])
    for l in range(2):
        p.energy[l] = ffi.ptr(keep["energy"][l]); p.exact[l] = ffi.ptr(keep["exact"][l]); p.head[l] = ffi.ptr(keep["head"][l])
        p.pnorm[l] = ffi.ptr(keep["pnorm"][l])
        for s in range(2):
            p.row_map[s][l] = ffi.ptr(keep["row_map"][s][l], i32)
    for s in range(2):
        p.nsel[s] = ffi.ptr(keep["nsel"][s], i32)
    p.tau_key = ffi.ptr(keep["tau_key"], u32)
    ffi.check(L.cald_op_rpn_prune(hip["ctx"], C.byref(p)))
    keep["check"] = np.array([p.check[0], p.check[1]], F32)
    keep["stat"] = np.array(list(p.stat), np.uint64)
    return keep


def _expected(c, r):
    """the restatement's result in the layout of the in / out arrays, sentinels where nothing may be written."""
    V, ld = c["V"], c["ld"]
    pix = _pix(c["hw"])
    want = dict(head=[np.concatenate([r["head"][l], np.full((GUARD, ld), S_F32, F32)]) for l in range(2)],
                pnorm=[np.concatenate([r["pnorm"][l], np.full(GUARD, S_F32, F32)]) for l in range(2)],
                tau_key=np.concatenate([r["tau_key"].reshape(-1), np.full(GUARD, S_U32, np.uint32)]),
                nsel=[np.concatenate([r["nsel"][s].reshape(-1), np.full(GUARD, S_I32, np.int32)]) for s in range(2)],
                row_map=[[np.full(pix[l] + GUARD, S_I32, np.int32) for l in range(2)] for _ in range(2)],
                check=r["check"], stat=r["stat"])
    for s in range(2):
        for l in range(2):
            for off, idx in r["row_map"][s][l]:
                want["row_map"][s][l][off:off + idx.size] = idx
    return want


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32)) if got.itemsize == 4 else []
        raise AssertionError("%s: %d words differ, first at %s: got %r, want %r" % (what, len(bad), bad[:4], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_prune_kernels_equal_their_restatement_bit_for_bit(hip, name):
    """select stage 0, select stage 1 and the scatter on one case: every output byte-equal to tests/_prune_restatement.py, every sentinel
    in place."""
    c, r = _reference(name)
    got, want = _run_gpu(hip, c), _expected(c, r)
    for l in range(2):
        _same(got["pnorm"][l], want["pnorm"][l], "pnorm[%d]" % l)
        ok = np.isfinite(r["pnorm64"][l])
        assert (got["pnorm"][l][:-GUARD][ok].astype(np.float64) >= r["pnorm64"][l][ok]).all()
    _same(got["tau_key"], want["tau_key"], "tau_key")
    for s in range(2):
        _same(got["nsel"][s], want["nsel"][s], "nsel[%d]" % s)
    for s in range(2):
        for l in range(2):
            _same(got["row_map"][s][l], want["row_map"][s][l], "row_map[%d][%d]" % (s, l))
    for l in range(2):
        _same(got["head"][l], want["head"][l], "head[%d]" % l)
    _same(got["check"], want["check"], "check")
    assert np.array_equal(got["stat"], want["stat"]), (got["stat"], want["stat"])


@pytest.mark.gpu
def test_prune_hook_refuses_malformed_arguments(hip):
    ffi, L = hip["ffi"], hip["L"]
    c, _ = _reference("geo_1x1")
    for field, bad in (("V", 0), ("V", ffi.PRUNE_PROBE_MAX_VIEWS + 1), ("head_ld", 2), ("pre_n", 0), ("guard", -1)):
        p = ffi.RpnPruneProbe(); p.V = 1; p.head_ld = 15; p.pre_n = 1
        p.hw[0][0][0] = p.hw[0][0][1] = p.hw[1][0][0] = p.hw[1][0][1] = 1
        setattr(p, field, bad)
        assert L.cald_op_rpn_prune(hip["ctx"], C.byref(p)) == -1, field          # CALD_ERR_INVALID
    p = ffi.RpnPruneProbe(); p.V = 1; p.head_ld = 15; p.pre_n = 1
    p.hw[0][0][0] = p.hw[0][0][1] = p.hw[1][0][0] = 1                            # level 1: W = 0
    assert L.cald_op_rpn_prune(hip["ctx"], C.byref(p)) == -1
    p.hw[1][0][1] = 1                                                            # sizes fine, arrays null
    assert L.cald_op_rpn_prune(hip["ctx"], C.byref(p)) == -1
    assert L.cald_op_rpn_prune(hip["ctx"], None) == -1


# ---------------------------------------------------------------------------------------------------------------------------
# the ratio tripwire of sweep_checked
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sweep_falls_back_to_the_dense_head_when_the_bound_is_exceeded(hip):
    """sweep_checked's `!(chk[0] <= 1.0f)`, which no data has ever reached: with the bound's constants scaled by 2^-24
    (cald_model_set_rpn_prune_bound; the measured worst ratio is ~4e-5 = 2^-14.6, so the ratio exceeds 1 by a factor of ~2^9) the sweep
    must count one fallback and return the dense head's results; with a NaN constant (NaN ratio -> inf) again.  Neither sweep's ratio
    may enter cald_profile_prune's worst_bound_ratio, which speaks about the certified bound."""
    torch, ffi, L = hip["torch"], hip["ffi"], hip["L"]
    from cald_amd import synth, sweep
    m = hip["det"].fasterrcnn_resnet50_fpn_feature(num_classes=21, min_size=300, max_size=500).to("cuda")
    m.load_state_dict(synth.pseudo_trained_frcnn(21, 50, seed=0)); m.eval()
    dev = [torch.from_numpy(im).cuda() for im in synth.make_pool(5, "voc", 1, scale=0.5)]

    def run():
        return sweep.sweep_device_images(m, dev, list(range(5)), ["flip", "cut_out"], bp=1.3, base_seed=1, batch_images=3)

    def counters():
        n = C.c_int64(); w = C.c_double()
        ffi.check(L.cald_profile_prune_fallbacks(hip["ctx"], C.byref(n)))
        ffi.check(L.cald_profile_prune(hip["ctx"], None, None, None, C.byref(w), None))
        return n.value, w.value

    assert m.set_rpn_prune(False) is True
    dense = run()
    assert m.set_rpn_prune(True) is False
    n0, _ = counters()
    pruned = run()
    n1, w1 = counters()
    print("certified sweep: worst ratio %.3g" % w1)
    assert n1 == n0 and 0.0 < w1 <= 2.0 ** -9            # the certified bound holds with the margin the scaled one is to lose
    assert pruned[0].tobytes() == dense[0].tobytes() and pruned[1].tobytes() == dense[1].tobytes()
    c1, c0 = m.rpn_prune_bound()
    m.set_rpn_prune_bound(c1 * F32(2.0 ** -24), c0 * F32(2.0 ** -24))
    g1, g0 = m.rpn_prune_bound()
    assert g1.tobytes() == (c1 * F32(2.0 ** -24)).tobytes() and g0.tobytes() == (c0 * F32(2.0 ** -24)).tobytes()
    got = run()
    n2, w2 = counters()
    assert n2 == n1 + 1                                   # exactly one fallback
    assert got[0].tobytes() == dense[0].tobytes() and got[1].tobytes() == dense[1].tobytes()
    assert w2 == w1                                       # the voided bound's ratio is not the certificate's
    bad = c1.copy(); bad[1] = np.nan
    m.set_rpn_prune_bound(bad, c0)
    got = run()
    n3, w3 = counters()
    assert n3 == n2 + 1 and w3 == w1
    assert got[0].tobytes() == dense[0].tobytes() and got[1].tobytes() == dense[1].tobytes()
    assert m.set_rpn_prune(True) is True                  # the fallbacks left the switch as it was
