"""Every variant of the training kernels (cald_amd/csrc/train_*.hip) run directly: the weight-gradient plan pinned by a host query and
driven through every kernel / split / reduction edge with EXACT-INTEGER operands, RoIAlign forward and backward at the production
channel count with every merge pattern named, the code behind the environment switches in child processes, and the small backward
kernels at the sizes where a vector grid has a tail block.

Exact integers: fp32 products and sums of small integers are exact in ANY order while every partial sum stays below 2^24, on the
matrix pipe as on the vector ALU.  With x in {-1, 0, 1} and g in {-2 .. 2} a weight / bias / data gradient or a forward has ONE
correct float32 answer whatever the split count, tile order or reduction order, and an int64 / float64 numpy sum gives it: those
comparisons are array_equal, no tolerance.  Each case asserts its bound (2 * terms < 2^24) from its own shape.  One gaussian /
float64 comparison per variant stays (2e-5 of the largest magnitude, the rule of test_gpu_train.py), because integers cannot see a
wrong rounding or a misplaced fractional weight."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1 << 24          # integers of magnitude below 2^24 are exact in float32


@pytest.fixture(scope="module")
def T():
    import torch
    from cald_amd import train_ops
    if not torch.cuda.is_available():      # module-scoped: runs before conftest's function-scoped auto-skip
        pytest.skip("needs an MI355X")
    return torch, train_ops


def _close(got, want, tol, what):
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-30, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err <= tol, "%s: max err / max|ref| = %.3g > %.3g" % (what, err, tol)


def _exact(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == np.float32, (what, got.dtype)
    bad = np.flatnonzero(got.astype(np.float64).ravel() != want.astype(np.float64).ravel())
    assert bad.size == 0, "%s: %d of %d elements differ from the exact sum; first at %s: got %r, exact %r" % (
        what, bad.size, got.size, np.unravel_index(bad[0], got.shape), got.ravel()[bad[0]], want.ravel()[bad[0]])


def _cpu(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the weight gradient: case table, plan coverage, exact sums
# ---------------------------------------------------------------------------------------------------------------------
POINTWISE, TABLE, GENERAL, GENERAL32, WIDE = 0, 1, 2, 3, 4       # CALD_WGRAD_* of include/cald_hip.h
REDUCE_FLAT, REDUCE_TAPS = 0, 1
KERNEL_NAMES = {POINTWISE: b"wgrad_kernel<true,16,1>", TABLE: b"wgrad_kernel<true,16,2>", GENERAL: b"wgrad_kernel<true,16>",
                GENERAL32: b"wgrad_kernel<true,32>", WIDE: b"wgrad_kernel<false,16>"}


def _case(name, N, H, W, Cin, Cout, K, s, p, variant, ldx=None, ldg=None, bias=False, row_scale=False):
    return dict(name=name, N=N, H=H, W=W, Cin=Cin, ldx=ldx or Cin, Cout=Cout, ldg=ldg or (Cout + 3) // 4 * 4, K=K, s=s, p=p,
                variant=variant, bias=bias, row_scale=row_scale)


# name, N, H, W, Cin, Cout, K, stride, pad, the kernel the shape is MEANT to reach (asserted against the plan)
WGRAD_CASES = [
    # pointwise kernel (1 x 1, stride 1), flat reduction
    _case("pw_q1_cout1", 1, 1, 1, 4, 1, 1, 1, 0, POINTWISE, bias=True),                      # Q == 1, Cin = 4, Cout = 1
    _case("pw_q20", 2, 2, 5, 64, 15, 1, 1, 0, POINTWISE, bias=True),                         # Q < 32, the 15-column RPN head
    _case("pw_ragged", 3, 16, 20, 128, 64, 1, 1, 0, POINTWISE, row_scale=True),              # 960 pixels: 4 splits of 256, last one 192
    _case("pw_q1023", 1, 11, 93, 64, 129, 1, 1, 0, POINTWISE, bias=True),                    # one below 4 x chunk; Cout = 129: a second row tile
    _case("pw_q1024", 1, 32, 32, 64, 128, 1, 1, 0, POINTWISE, ldg=132),                      # Q == S x chunk; pad channels past a full tile
    _case("pw_q1025", 1, 25, 41, 64, 256, 1, 1, 0, POINTWISE, ldx=72, bias=True),            # ldx > Cin
    _case("pw_q1793", 1, 11, 163, 32, 105, 1, 1, 0, POINTWISE, bias=True),                   # 1 793 = 7 x 256 + 1: one above a multiple of chunk
    _case("pw_seam", 3, 19, 23, 256, 105, 1, 1, 0, POINTWISE, ldx=260, bias=True),           # seams inside images 1 and 2
    # offset-table kernel (Cin % 128 == 0, not pointwise)
    _case("tab_1x1_map", 1, 1, 1, 128, 15, 3, 1, 1, TABLE, bias=True),                       # map smaller than its filter, Q == 1
    _case("tab_1x2_map", 2, 1, 2, 256, 1, 3, 1, 1, TABLE, bias=True),
    _case("tab_2x3_map", 2, 2, 3, 256, 256, 3, 1, 1, TABLE, row_scale=True),
    _case("tab_s2_even", 2, 18, 22, 128, 64, 3, 2, 1, TABLE, row_scale=True),
    _case("tab_s2_odd", 2, 17, 23, 128, 105, 3, 2, 1, TABLE, bias=True),
    _case("tab_1x1_s2_odd", 2, 17, 23, 256, 64, 1, 2, 0, TABLE, ldx=264, bias=True),         # the downsample shape, ldx > Cin
    _case("tab_ragged_seam", 2, 75, 70, 128, 128, 3, 1, 1, TABLE),                           # 10 500 pixels, 42 splits, seams inside image 1
    _case("tab_fills_seam", 2, 200, 200, 128, 129, 3, 1, 1, TABLE, bias=True),               # chunk > 1 024: several table fills per split
    _case("tab_q1023", 1, 11, 93, 1024, 1024, 3, 1, 1, TABLE),                               # ONE split around the 1 024-entry table
    _case("tab_q1024", 1, 32, 32, 1024, 1024, 3, 1, 1, TABLE),
    _case("tab_q1025", 1, 25, 41, 1024, 1024, 3, 1, 1, TABLE),
    # general kernel (filters with an extent, Cin % 128 != 0)
    _case("gen_1x1_map", 1, 1, 1, 64, 15, 3, 1, 1, GENERAL, bias=True),
    _case("gen_1x2_map", 2, 1, 2, 64, 105, 3, 1, 1, GENERAL, bias=True),
    _case("gen_2x3_map", 2, 2, 3, 48, 128, 3, 1, 1, GENERAL, row_scale=True),
    _case("gen_j_tail", 2, 9, 11, 48, 105, 3, 1, 1, GENERAL, bias=True),                     # J = 432: a ragged column tile
    _case("gen_cin4_7x7", 2, 20, 25, 4, 15, 7, 2, 3, GENERAL, bias=True),                    # the stem's shape: 49 taps of 4 channels
    _case("gen_s2_even", 2, 18, 22, 64, 64, 3, 2, 1, GENERAL, row_scale=True),
    _case("gen_s2_odd", 2, 17, 23, 64, 129, 3, 2, 1, GENERAL, ldx=68, bias=True),
    _case("gen_1x1_s2", 2, 18, 21, 64, 256, 1, 2, 0, GENERAL, bias=True),
    _case("gen_ragged_seam", 3, 37, 41, 64, 1, 3, 1, 1, GENERAL, ldx=72, bias=True),         # 4 551 pixels, seams inside images 1 and 2
    _case("gen_q_mult", 1, 32, 64, 32, 128, 3, 1, 1, GENERAL, row_scale=True),               # 2 048 = 8 x 256
]
# x [R][K], g [R][ldg]: R, K, Cout, taps
LINEAR_CASES = [(1, 64, 15, 1), (31, 128, 105, 1), (200, 256, 129, 1), (513, 64, 256, 1), (1, 49 * 8, 1, 49), (31, 49 * 16, 128, 49),
                (200, 49 * 64, 128, 49), (513, 49 * 4, 15, 49), (200, 12544, 1024, 49)]       # the last one: fc6 at its real size


def _conv_plan(ops, cs):
    return ops.conv_wgrad_plan(cs["N"], cs["H"], cs["W"], cs["Cin"], cs["ldx"], cs["Cout"], cs["ldg"], cs["K"], cs["K"], cs["s"], cs["p"])


def _out_hw(cs):
    return (cs["H"] + 2 * cs["p"] - cs["K"]) // cs["s"] + 1, (cs["W"] + 2 * cs["p"] - cs["K"]) // cs["s"] + 1


def _int_operands(cs, seed):
    """x in {-1, 0, 1} (unused channels Cin..ldx: garbage), g in {-2 .. 2} (pad channels Cout..ldg: garbage), as float32 NHWC."""
    rs = np.random.RandomState(seed)
    Ho, Wo = _out_hw(cs)
    x = rs.randint(-1, 2, (cs["N"], cs["H"], cs["W"], cs["ldx"])).astype(np.float32)
    g = rs.randint(-2, 3, (cs["N"], Ho, Wo, cs["ldg"])).astype(np.float32)
    x[..., cs["Cin"]:] = rs.randint(-1000, 1000, x[..., cs["Cin"]:].shape) + 0.37      # must never reach dw
    g[..., cs["Cout"]:] = rs.randint(-1000, 1000, g[..., cs["Cout"]:].shape) + 0.37     # must never reach dw / db
    return x, g


def _wgrad_reference(x, g, Cin, Cout, K, s, p):
    """dw[co][ci][ky][kx] = sum over output pixels of g[q][co] * x[q @ (ky, kx)][ci], db[co] = sum of g[q][co], in float64."""
    N, H, W, _ = x.shape
    _, Ho, Wo, _ = g.shape
    xp = np.zeros((N, H + 2 * p, W + 2 * p, Cin), np.float64)
    xp[:, p:p + H, p:p + W] = x[..., :Cin]
    g2 = g[..., :Cout].reshape(-1, Cout).astype(np.float64)
    dw = np.empty((Cout, Cin, K, K), np.float64)
    for ky in range(K):
        for kx in range(K):
            xs = xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s].reshape(-1, Cin)
            dw[:, :, ky, kx] = g2.T @ xs
    return dw, g2.sum(0)


def _pow2(rs, n):
    return (2.0 ** rs.randint(-2, 3, n)).astype(np.float32)


def run_conv_wgrad_case(torch, ops, cs):
    """One row of WGRAD_CASES through ops.conv_wgrad with exact-integer operands: plain, then accumulated onto non-zero dw / db (with
    row_scale where the row asks for it).  Returns the four results (float32 numpy) after asserting each against the exact sum."""
    Ho, Wo = _out_hw(cs)
    Q = cs["N"] * Ho * Wo
    # every product is an integer of magnitude <= 2 and an output element sums Q of them: partial sums stay below 2 Q in any order.
    # row_scale (2^-2 .. 2^2) turns the sum into a multiple of 1/4 of magnitude <= 8 Q; the accumulate target adds an integer <= 3.
    assert 2 * Q < EXACT and 4 * (8 * Q + 3) < EXACT, "case %s leaves the exact range" % cs["name"]
    rs = np.random.RandomState(len(cs["name"]) * 131 + Q)
    x, g = _int_operands(cs, Q % 9973 + 17)
    want_dw, want_db = _wgrad_reference(x, g, cs["Cin"], cs["Cout"], cs["K"], cs["s"], cs["p"])
    xc, gc = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    shape = (cs["Cout"], cs["Cin"], cs["K"], cs["K"])
    scale = _pow2(rs, cs["Cout"]) if cs["row_scale"] else None
    sc = torch.from_numpy(scale).cuda() if scale is not None else None
    sref = scale.astype(np.float64)[:, None, None, None] if scale is not None else 1.0
    dw = torch.full(shape, float("nan"), device="cuda"); db = torch.full((cs["Cout"],), float("nan"), device="cuda") if cs["bias"] else None
    ops.conv_wgrad(xc, gc, cs["Cin"], cs["Cout"], cs["K"], cs["K"], cs["s"], cs["p"], dw, db, row_scale=sc)
    _exact(_cpu(dw), want_dw * sref, cs["name"] + ": dw")
    if db is not None:
        _exact(_cpu(db), want_db, cs["name"] + ": db")
    dw0 = rs.randint(-3, 4, shape).astype(np.float32); db0 = rs.randint(-3, 4, cs["Cout"]).astype(np.float32)
    dw2 = torch.from_numpy(dw0).cuda(); db2 = torch.from_numpy(db0).cuda() if cs["bias"] else None
    ops.conv_wgrad(xc, gc, cs["Cin"], cs["Cout"], cs["K"], cs["K"], cs["s"], cs["p"], dw2, db2, accumulate=True, row_scale=sc)
    _exact(_cpu(dw2), dw0 + want_dw * sref, cs["name"] + ": dw accumulated")
    if db2 is not None:
        _exact(_cpu(db2), db0 + want_db, cs["name"] + ": db accumulated")
    return [_cpu(t) for t in (dw, dw2)] + ([_cpu(db), _cpu(db2)] if cs["bias"] else [])


def run_linear_wgrad_case(torch, ops, case):
    R, K, Cout, taps = case
    assert 2 * R + 3 < EXACT
    ldg = (Cout + 3) // 4 * 4
    rs = np.random.RandomState(R * 7 + K + Cout)
    x = rs.randint(-1, 2, (R, K)).astype(np.float32)
    g = rs.randint(-2, 3, (R, ldg)).astype(np.float32)
    g[:, Cout:] = rs.randint(-1000, 1000, (R, ldg - Cout)) + 0.37
    flat = g[:, :Cout].astype(np.float64).T @ x.astype(np.float64)                       # [Cout][tap * Cin + ci], rows are [tap][K / taps]
    want_dw = flat.reshape(Cout, taps, K // taps).transpose(0, 2, 1).reshape(Cout, K)     # torch layout [Cout][K / taps][taps]
    want_db = g[:, :Cout].astype(np.float64).sum(0)
    xc, gc = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    dw = torch.full((Cout, K), float("nan"), device="cuda"); db = torch.full((Cout,), float("nan"), device="cuda")
    ops.linear_wgrad(xc, gc, Cout, dw, db, taps=taps)
    _exact(_cpu(dw), want_dw, "linear %s: dw" % (case,)); _exact(_cpu(db), want_db, "linear %s: db" % (case,))
    dw0 = rs.randint(-3, 4, (Cout, K)).astype(np.float32); db0 = rs.randint(-3, 4, Cout).astype(np.float32)
    dw2, db2 = torch.from_numpy(dw0).cuda(), torch.from_numpy(db0).cuda()
    ops.linear_wgrad(xc, gc, Cout, dw2, db2, taps=taps, accumulate=True)
    _exact(_cpu(dw2), dw0 + want_dw, "linear %s: dw accumulated" % (case,)); _exact(_cpu(db2), db0 + want_db, "linear %s: db accumulated" % (case,))
    return [_cpu(t) for t in (dw, db, dw2, db2)]


@pytest.mark.parametrize("cs", WGRAD_CASES, ids=lambda c: c["name"])
def test_conv_wgrad_exact_integer_sums(T, cs):
    """Every row of the case table: the kernel the plan names is the one the row is meant to reach, and dw / db (plain, with
    row_scale, accumulated onto non-zero tensors, with garbage in every pad channel) equal the integer sums exactly."""
    torch, ops = T
    pl = _conv_plan(ops, cs)
    assert pl.variant == cs["variant"] and pl.kernel == KERNEL_NAMES[cs["variant"]], (cs["name"], pl.variant, pl.kernel)
    run_conv_wgrad_case(torch, ops, cs)


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "R%d_K%d_Co%d_t%d" % c)
def test_linear_wgrad_exact_integer_sums(T, case):
    """linear_wgrad at row counts around the stage / split sizes, plain and tap-major (fc6) rows, bias gradient, accumulate."""
    torch, ops = T
    R, K, Cout, taps = case
    pl = ops.linear_wgrad_plan(R, K, Cout, (Cout + 3) // 4 * 4, taps)
    assert pl.variant == POINTWISE and pl.reduce == (REDUCE_TAPS if taps > 1 else REDUCE_FLAT)
    run_linear_wgrad_case(torch, ops, case)


def test_wgrad_case_table_reaches_every_kernel_split_shape_and_edge(T):
    """The coverage the table above is there for, asserted from the plan the library answers (a later change to the plan or to a
    row that makes a case stop reaching its variant or its edge fails here, not silently)."""
    torch, ops = T
    plans = [(cs, _conv_plan(ops, cs)) for cs in WGRAD_CASES]
    Qs = {cs["name"]: cs["N"] * _out_hw(cs)[0] * _out_hw(cs)[1] for cs in WGRAD_CASES}
    for cs, pl in plans:
        Q = Qs[cs["name"]]
        assert pl.chunk % 32 == 0 and (pl.S - 1) * pl.chunk < Q <= pl.S * pl.chunk, (cs["name"], pl.S, pl.chunk)
        assert pl.csplit * pl.rows_per_block >= Q and pl.JT == (cs["K"] ** 2 * cs["Cin"] + 127) // 128 and pl.MT == (cs["Cout"] + 127) // 128
    big = ops.conv_wgrad_plan(*WIDE_X, 4, 4, 3, 3, 1, 1)
    assert big.variant == WIDE and big.kernel == KERNEL_NAMES[WIDE]
    assert {pl.variant for _, pl in plans} | {big.variant} == {POINTWISE, TABLE, GENERAL, WIDE}, "the four kernels a default run can reach"
    for v in (POINTWISE, TABLE, GENERAL):
        sel = [(cs, pl) for cs, pl in plans if pl.variant == v]
        assert any(pl.S == 1 for _, pl in sel), v
        assert any(pl.S > 1 and Qs[cs["name"]] % pl.chunk for cs, pl in sel), "ragged last split, variant %d" % v
        assert any(pl.S > 1 and cs["N"] > 1 and any((k * pl.chunk) % (Qs[cs["name"]] // cs["N"]) and k * pl.chunk > Qs[cs["name"]] // cs["N"]
                                                    for k in range(1, pl.S)) for cs, pl in sel), "a split seam inside an image n > 0, variant %d" % v
        assert any(cs["ldx"] > cs["Cin"] for cs, _ in sel), "ldx > Cin, variant %d" % v
        assert any(cs["ldg"] > cs["Cout"] for cs, _ in sel), "pad channels in g, variant %d" % v
        assert any(cs["row_scale"] for cs, _ in sel) and any(cs["bias"] for cs, _ in sel), v
    assert {pl.reduce for _, pl in plans} == {REDUCE_FLAT, REDUCE_TAPS}
    assert any(pl.S > 1 and Qs[cs["name"]] == pl.S * pl.chunk for cs, pl in plans), "Q equal to a multiple of chunk"
    assert any(pl.S > 1 and Qs[cs["name"]] == pl.S * pl.chunk - 1 for cs, pl in plans), "Q one below a multiple of chunk"
    assert any(pl.S > 1 and Qs[cs["name"]] == (pl.S - 1) * pl.chunk + 1 for cs, pl in plans), "Q one above a multiple of chunk"
    tab1 = {Qs[cs["name"]]: pl for cs, pl in plans if pl.variant == TABLE and pl.S == 1}
    assert {1023, 1024, 1025} <= set(tab1), "the offset-table kernel around its 1 024-pixel table, in ONE split"
    assert any(pl.variant == TABLE and pl.S > 1 and pl.chunk > 1024 for _, pl in plans), "several table fills inside a split of several"
    assert any(Q == 1 for Q in Qs.values()) and any(1 < Q < 32 for Q in Qs.values())
    for v in (TABLE, GENERAL):
        small = {(cs["H"], cs["W"]) for cs, pl in plans if pl.variant == v and cs["K"] == 3 and cs["p"] == 1}
        assert {(1, 1), (1, 2), (2, 3)} <= small, "maps smaller than the 3 x 3 filter, variant %d" % v
        s2 = [(cs["H"] % 2, cs["W"] % 2) for cs, pl in plans if pl.variant == v and cs["s"] == 2]
        assert {0, 1} <= {h for h, _ in s2} and {0, 1} <= {w for _, w in s2}, "stride 2 on odd and even sizes, variant %d" % v
    assert {1, 15, 105, 128, 129, 256} <= {cs["Cout"] for cs in WGRAD_CASES}
    assert any(cs["Cin"] == 4 for cs in WGRAD_CASES) and any((cs["K"] ** 2 * cs["Cin"]) % 128 for cs in WGRAD_CASES)
    assert {1, 31, 200, 513} <= {c[0] for c in LINEAR_CASES if c[3] == 1} and {1, 31, 200, 513} <= {c[0] for c in LINEAR_CASES if c[3] == 49}
    assert (200, 12544, 1024, 49) in LINEAR_CASES
    # the refusals: a row stride below the channel count, strides that are not multiples of 4
    for bad in ((8, 4, 4, 4), (8, 8, 5, 4), (6, 6, 4, 4), (8, 8, 4, 6)):
        with pytest.raises(RuntimeError):
            ops.conv_wgrad_plan(1, 4, 4, bad[0], bad[1], bad[2], bad[3], 1, 1, 1, 0)
    x = torch.zeros(1, 4, 4, 4, device="cuda"); g = torch.zeros(1, 4, 4, 4, device="cuda"); dw = torch.zeros(8, 8, 1, 1, device="cuda")
    with pytest.raises(RuntimeError):
        ops.conv_wgrad(x, g, 8, 4, 1, 1, 1, 0, dw)            # Cin = 8 channels claimed of rows that hold 4


GAUSS_CASES = ["pw_seam", "tab_ragged_seam", "tab_s2_odd", "gen_j_tail", "gen_s2_odd", "gen_cin4_7x7"]


@pytest.mark.parametrize("name", GAUSS_CASES)
def test_conv_wgrad_gaussian_vs_float64(T, name):
    """One gaussian comparison per variant (float64 sums, 2e-5 of the largest magnitude): a wrong rounding or a fractional weight
    in the wrong place is invisible to integers.  row_scale is an arbitrary positive vector here."""
    torch, ops = T
    cs = [c for c in WGRAD_CASES if c["name"] == name][0]
    rs = np.random.RandomState(len(name))
    Ho, Wo = _out_hw(cs)
    x = rs.randn(cs["N"], cs["H"], cs["W"], cs["ldx"]).astype(np.float32); g = rs.randn(cs["N"], Ho, Wo, cs["ldg"]).astype(np.float32)
    scale = (rs.rand(cs["Cout"]) + 0.5).astype(np.float32)
    want_dw, want_db = _wgrad_reference(x, g, cs["Cin"], cs["Cout"], cs["K"], cs["s"], cs["p"])
    xc, gc = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    dw = torch.empty((cs["Cout"], cs["Cin"], cs["K"], cs["K"]), device="cuda"); db = torch.empty(cs["Cout"], device="cuda")
    ops.conv_wgrad(xc, gc, cs["Cin"], cs["Cout"], cs["K"], cs["K"], cs["s"], cs["p"], dw, db)
    _close(_cpu(dw), want_dw, 2e-5, name + ": dw"); _close(_cpu(db), want_db, 2e-5, name + ": db")
    ops.conv_wgrad(xc, gc, cs["Cin"], cs["Cout"], cs["K"], cs["K"], cs["s"], cs["p"], dw, None, row_scale=torch.from_numpy(scale).cuda())
    _close(_cpu(dw), want_dw * scale.astype(np.float64)[:, None, None, None], 2e-5, name + ": dw with row_scale")


# N, H, W, Cin (= ldx): x is N * H * W * Cin * 4 = 2 153 216 000 bytes >= 0x7FFE0000, so the plan leaves the 32-bit buffer addressing
WIDE_X = (2, 1450, 1450, 128, 128)
# a 1 x 1 layer whose g is the wide tensor: Q * ldg * 4 = 2 151 680 000 bytes, x only 34 MB
WIDE_G = (2, 1025, 1025, 4, 256)


def test_wgrad_wide_x_exact(T):
    """wgrad_kernel<false,16> (64-bit addressing), reached only by a tensor of 2 GB or more: a 3 x 3 layer on 2 x 1450 x 1450 x 128
    activations with 4 outputs, exact-integer operands.  x is drawn as int8 on the host and widened on the device; the reference goes
    tap by tap over row chunks so that host memory stays near the int8 copy of x.  2 Q = 8.4 M < 2^24."""
    torch, ops = T
    N, H, W, Cin, ldx = WIDE_X
    Cout, ldg = 4, 4
    Q = N * H * W
    assert 2 * Q < EXACT and N * H * W * ldx * 4 >= 0x7FFE0000
    pl = ops.conv_wgrad_plan(N, H, W, Cin, ldx, Cout, ldg, 3, 3, 1, 1)
    assert pl.variant == WIDE and pl.S > 1
    torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    rng = np.random.default_rng(11)
    x8 = rng.integers(-1, 2, (N, H, W, Cin), dtype=np.int8)
    g = rng.integers(-2, 3, (N, H, W, ldg), dtype=np.int8)
    x8t = torch.from_numpy(x8); gt = torch.from_numpy(g).float()
    xc = x8t.cuda().float(); gc = gt.cuda()
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda"); db = torch.full((Cout,), float("nan"), device="cuda")
    ops.conv_wgrad(xc, gc, Cin, Cout, 3, 3, 1, 1, dw, db)
    torch.cuda.synchronize()
    got_dw, got_db = _cpu(dw), _cpu(db)
    print("wide-x case: device memory high-water mark %.2f GB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))
    del xc, gc, dw, db
    torch.cuda.empty_cache()
    # reference: dw[:, :, ky, kx] = sum over row chunks of g[rows].T @ x[rows + ky - 1, cols + kx - 1]; a chunk's float32 product is
    # exact (2 * 64 * 1450 < 2^24) and the chunks are added in float64
    rows = 64
    assert 2 * rows * W < EXACT
    want = np.zeros((Cout, Cin, 3, 3), np.float64)
    for n in range(N):
        for ky in range(3):
            for y0 in range(0, H, rows):
                oy0, oy1 = max(y0, 1 - ky), min(y0 + rows, H, H + 1 - ky)          # output rows whose input row oy + ky - 1 is inside
                if oy1 <= oy0:
                    continue
                xs = x8t[n, oy0 + ky - 1:oy1 + ky - 1].float()                   # [r][W][Cin]
                gs = gt[n, oy0:oy1]                                              # [r][W][4]
                for kx in range(3):
                    ox0, ox1 = max(0, 1 - kx), min(W, W + 1 - kx)
                    a = gs[:, ox0:ox1].reshape(-1, ldg); b = xs[:, ox0 + kx - 1:ox1 + kx - 1].reshape(-1, Cin)
                    want[:, :, ky, kx] += (a.t() @ b).double().numpy()
    _exact(got_dw, want, "wide x: dw")
    _exact(got_db, g.reshape(-1, ldg).astype(np.int64).sum(0), "wide x: db")
    del x8, x8t, g, gt


def test_wgrad_wide_g_exact(T):
    """The same kernel reached through g: a 1 x 1 layer with 4 inputs and 256 outputs on 2 x 1025 x 1025 pixels (g is 2.15 GB, x 34 MB;
    the shape would be the pointwise kernel's if it fitted 32-bit offsets).  Exact-integer operands, 2 Q = 4.2 M < 2^24."""
    torch, ops = T
    N, H, W, Cin, Cout = WIDE_G
    Q = N * H * W
    assert 2 * Q < EXACT and Q * Cout * 4 >= 0x7FFE0000
    pl = ops.conv_wgrad_plan(N, H, W, Cin, Cin, Cout, Cout, 1, 1, 1, 0)
    assert pl.variant == WIDE and pl.reduce == REDUCE_FLAT
    torch.cuda.empty_cache()
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.integers(-1, 2, (Q, Cin), dtype=np.int8))
    g8 = torch.from_numpy(rng.integers(-2, 3, (Q, Cout), dtype=np.int8))
    xc = x.cuda().float().view(N, H, W, Cin); gc = g8.cuda().float().view(N, H, W, Cout)
    dw = torch.full((Cout, Cin, 1, 1), float("nan"), device="cuda"); db = torch.full((Cout,), float("nan"), device="cuda")
    ops.conv_wgrad(xc, gc, Cin, Cout, 1, 1, 1, 0, dw, db)
    got_dw, got_db = _cpu(dw), _cpu(db)
    del xc, gc, dw, db
    torch.cuda.empty_cache()
    want = np.zeros((Cout, Cin), np.float64); wdb = np.zeros(Cout, np.float64)
    step = 1 << 18
    assert 2 * step < EXACT
    for q0 in range(0, Q, step):
        a = g8[q0:q0 + step].float()
        want += (a.t() @ x[q0:q0 + step].float()).double().numpy(); wdb += a.sum(0).double().numpy()
    _exact(got_dw, want.reshape(Cout, Cin, 1, 1), "wide g: dw"); _exact(got_db, wdb, "wide g: db")


SMALL_MAPS = [(1, 1), (1, 2), (2, 3)]


def test_conv_entry_points_exact_on_the_smallest_maps(T):
    """ops.conv (forward with a power-of-two FrozenBN scale and bias), ops.conv_dgrad (stride 1 and 2) and ops.conv_group with
    masks, each once per map smaller than its 3 x 3 filter, on exact-integer operands: |sum| <= 2 * 9 * 256 * 4, far inside 2^24."""
    torch, ops = T
    import torch.nn.functional as F
    rs = np.random.RandomState(5)
    N, Cin, Cout = 2, 64, 128
    assert 2 * 9 * max(Cin, Cout) * 4 + 4 < EXACT
    ti = lambda lo, hi, *shape: torch.from_numpy(rs.randint(lo, hi + 1, shape).astype(np.float32))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()
    w = ti(-1, 1, Cout, Cin, 3, 3); b = ti(-3, 3, Cout); sc = torch.from_numpy(_pow2(rs, Cout)); sh = ti(-2, 2, Cout)
    pk = ops.PackedConv(w.cuda(), scale=sc.cuda(), shift=sh.cuda())
    pkb = ops.PackedConv(w.cuda(), bias=b.cuda())
    pkd = ops.PackedConv(w.cuda(), CinK=Cout, mode=1)
    pkd2 = ops.PackedConv(w.cuda(), scale=sc.cuda(), CinK=Cout, mode=1)
    gys, acts = [], []
    for H, W in SMALL_MAPS:
        x = ti(-1, 1, N, Cin, H, W)
        y = F.conv2d(x.double(), w.double(), padding=1)
        _exact(_cpu(ops.conv(nhwc(x), pk, pad=1).permute(0, 3, 1, 2)), (y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).numpy(), "forward + BN %dx%d" % (H, W))
        _exact(_cpu(ops.conv(nhwc(x), pkb, pad=1, relu=True).permute(0, 3, 1, 2)), torch.relu(y + b.double().view(1, -1, 1, 1)).numpy(), "forward + bias + ReLU %dx%d" % (H, W))
        gy = ti(-2, 2, N, Cout, H, W); act = ti(-1, 1, N, Cin, H, W)
        dx = F.conv_transpose2d(gy.double(), w.double(), padding=1)
        _exact(_cpu(ops.conv_dgrad(nhwc(gy), pkd, H, W, 1, 1).permute(0, 3, 1, 2)), dx.numpy(), "data gradient %dx%d" % (H, W))
        _exact(_cpu(ops.conv_dgrad(nhwc(gy), pkd, H, W, 1, 1, mask=nhwc(act)).permute(0, 3, 1, 2)), (dx * (act > 0)).numpy(), "data gradient + mask %dx%d" % (H, W))
        gys.append(gy); acts.append(act)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        g2 = ti(-2, 2, N, Cout, Ho, Wo)
        xd = torch.zeros(N, Cin, H, W, dtype=torch.float64, requires_grad=True)
        (F.conv2d(xd, w.double(), stride=2, padding=1) * sc.double().view(1, -1, 1, 1)).backward(g2.double())
        _exact(_cpu(ops.conv_dgrad(nhwc(g2), pkd2, H, W, 2, 1).permute(0, 3, 1, 2)), xd.grad.numpy(), "stride-2 data gradient %dx%d" % (H, W))
        _exact(_cpu(ops.conv_dgrad(nhwc(g2), pkd2, H, W, 2, 1, mask=nhwc(act)).permute(0, 3, 1, 2)), (xd.grad * (act > 0)).numpy(), "stride-2 data gradient + mask %dx%d" % (H, W))
    outs = ops.conv_group([nhwc(t) for t in gys], pkd, pad=1, masks=[nhwc(t) for t in acts])
    for o, gy, act, hw in zip(outs, gys, acts, SMALL_MAPS):
        _exact(_cpu(o.permute(0, 3, 1, 2)), (F.conv_transpose2d(gy.double(), w.double(), padding=1) * (act > 0)).numpy(), "grouped data gradient + mask %dx%d" % hw)


# ---------------------------------------------------------------------------------------------------------------------
# 3. RoIAlign forward and backward at C = 256 (the channel count of every real model: roi_align_bwd_fixed_merge_kernel)
# ---------------------------------------------------------------------------------------------------------------------
ROI_DIMS = [(50, 68), (25, 34), (13, 17), (7, 9)]       # a 200 x 272 image's pyramid
F32 = np.float32


def roi_level_np(box):
    """kernels.h:roi_level in float32 (the product's det_log2f is replaced by numpy's log2: the test boxes stay clear of the level
    boundaries, which roi_set asserts)."""
    area = F32(F32(box[2] - box[0]) * F32(box[3] - box[1]))
    k = F32(4.0) + np.log2(np.sqrt(area, dtype=F32) / F32(224.0), dtype=F32)
    assert abs(float(k) - round(float(k))) > 1e-3 or float(k) < 1.5 or float(k) > 5.5, "box on a pyramid-level boundary"
    k = np.floor(F32(k + F32(1e-6)))
    return int(min(max(k, 2.0), 5.0)) - 2


def roi_sample_np(start, bin_, p, i, size):
    """kernels.h:roi_sample, operation by operation in float32: (lo, hi, l, h, valid, t)."""
    t = F32(F32(start + F32(F32(p) * bin_)) + F32(F32(F32(F32(i) + F32(0.5)) * bin_) / F32(2.0)))
    valid = not (t < F32(-1.0) or t > F32(size))
    tt = F32(0.0) if t <= F32(0.0) else t
    lo = int(tt)
    if lo >= size - 1:
        hi = lo = size - 1; tt = F32(lo)
    else:
        hi = lo + 1
    l = F32(tt - F32(lo)); h = F32(F32(1.0) - l)
    if not valid:
        lo = hi = 0
    return lo, hi, l, h, valid, float(t)


def roi_setup_np(box, dims):
    """train_roi.hip:roi_setup: level, the 14 row samples and the 14 column samples of one box, and whether rw / rh were raised to 1."""
    box = [F32(v) for v in box]
    l = roi_level_np(box)
    scale = F32(1.0) / F32(4 << l)
    x1, y1, x2, y2 = [F32(v * scale) for v in box]
    rw, rh = F32(x2 - x1), F32(y2 - y1)
    thin = (not rw >= F32(1.0), not rh >= F32(1.0))
    rw = rw if rw >= F32(1.0) else F32(1.0); rh = rh if rh >= F32(1.0) else F32(1.0)
    bw, bh = F32(rw / F32(7.0)), F32(rh / F32(7.0))
    sy = [roi_sample_np(y1, bh, k >> 1, k & 1, dims[l][0]) for k in range(14)]
    sx = [roi_sample_np(x1, bw, k >> 1, k & 1, dims[l][1]) for k in range(14)]
    return l, sy, sx, thin


def merge_pattern(s0, s1):
    """The sharing pattern roi_align_bwd_fixed_merge_kernel derives from the two samples of a bin along one axis."""
    return 2 if (s1[0] == s0[0] and s1[1] == s0[1]) else (1 if s1[0] == s0[1] else 0)


def roi_set():
    """The RoIs of the section: ordinary boxes of every pyramid level and aspect ratio (a fixed seed), plus the named edges."""
    rs = np.random.RandomState(7)
    boxes = []
    for s in (10, 25, 45, 70, 100, 130, 170, 200, 260, 320, 400, 520, 700):       # square roots of the areas: every level, off the boundaries
        for ar in (0.25, 0.6, 1.0, 1.7, 4.0):
            w, h = s * ar ** 0.5, s / ar ** 0.5
            x, y = rs.rand() * 230 - 10, rs.rand() * 170 - 10
            boxes.append([x, y, x + w, y + h])
    boxes += [[30.3, 40.7, 32.1, 90.2],          # narrower than one feature pixel (rw < 1)
              [50.5, 20.1, 120.9, 21.3],         # flatter than one feature pixel (rh < 1)
              [230.0, 150.0, 271.9, 199.9],      # into the bottom-right corner: border clamps on both axes
              [-30.0, -25.0, 40.0, 35.0],        # samples left of / above -1: invalid on the low side
              [240.0, 170.0, 330.0, 260.0],      # samples past the map: invalid on the high side
              [400.0, 50.0, 460.0, 110.0],       # fully outside, to the right
              [20.0, -120.0, 80.0, -60.0],       # fully outside, above
              [-90.0, -70.0, 350.0, 300.0]]      # larger than the image on every side (level 2)
    img = np.arange(len(boxes)) % 2
    return np.concatenate([img[:, None], np.array(boxes)], axis=1).astype(np.float32)


def roi_census(rois, dims):
    """What the RoI set reaches: merge patterns (all four samples valid), clamps, invalid sides, thin boxes, levels."""
    seen = dict(patterns=set(), clamp=set(), invalid=set(), thin=set(), levels=set(), outside=0, invalid_patterns=set())
    for r in rois:
        l, sy, sx, thin = roi_setup_np(r[1:], dims)
        seen["levels"].add(l)
        for axis, (ss, size, th) in enumerate(((sy, dims[l][0], thin[1]), (sx, dims[l][1], thin[0]))):
            if th:
                seen["thin"].add(axis)
            for s in ss:
                if s[4] and s[0] == s[1] == size - 1 and size > 1:
                    seen["clamp"].add(axis)
                if not s[4]:
                    seen["invalid"].add((axis, "low" if s[5] < -1.0 else "high"))
        if not any(a[4] and b[4] for a in sy for b in sx):
            seen["outside"] += 1
        for ph in range(7):
            for pw in range(7):
                pat = (merge_pattern(sy[2 * ph], sy[2 * ph + 1]), merge_pattern(sx[2 * pw], sx[2 * pw + 1]))
                ok = [sy[2 * ph][4], sy[2 * ph + 1][4], sx[2 * pw][4], sx[2 * pw + 1][4]]
                if all(ok):
                    seen["patterns"].add(pat)
                elif any(ok):
                    seen["invalid_patterns"].add(pat)
    return seen


def roi_scatter_f64(rois, gout, dims, N):
    """The backward as a float64 scatter that places the samples with the FLOAT32 weights of the restatement above (float64 autograd
    places them in double precision, about 1e-5 of a weight away at coordinates near 100).  Returns per level the sums, the sums of
    |terms| and the term counts, [N][H][W][C]."""
    C = gout.shape[2]
    sums = [np.zeros((N, h, w, C)) for h, w in dims]; mags = [np.zeros((N, h, w, C)) for h, w in dims]; cnts = [np.zeros((N, h, w, C)) for h, w in dims]
    for r, roi in enumerate(rois):
        n = int(roi[0])
        l, sy, sx, _ = roi_setup_np(roi[1:], dims)
        for a, Y in enumerate(sy):
            for b, X in enumerate(sx):
                if not (Y[4] and X[4]):
                    continue
                go = gout[r, (a >> 1) * 7 + (b >> 1)].astype(np.float64) * 0.25
                for (yy, wy) in ((Y[0], Y[3]), (Y[1], Y[2])):
                    for (xx, wx) in ((X[0], X[3]), (X[1], X[2])):
                        w = float(F32(wy * wx))                  # the kernel's first rounding is part of the operand
                        sums[l][n, yy, xx] += w * go; mags[l][n, yy, xx] += abs(w) * np.abs(go); cnts[l][n, yy, xx] += 1
    return sums, mags, cnts


def _roi_bwd(torch, ops, rois, gout, start=None, dims=ROI_DIMS, N=2):
    """ops.roi_align_bwd_ on numpy operands; start: the tensors gfeats holds before the call (default zeros).  Returns numpy levels."""
    C = gout.shape[2]
    gf = [torch.from_numpy(s.astype(np.float32)).cuda() if start is not None else torch.zeros(N, h, w, C, device="cuda")
          for s, (h, w) in zip(start if start is not None else dims, dims)]
    ops.roi_align_bwd_(gf, torch.from_numpy(rois).cuda(), torch.from_numpy(np.ascontiguousarray(gout, dtype=np.float32)).cuda())
    return [_cpu(t) for t in gf]


def _roi_autograd(torch, rois, feats, gout):
    """oracle/torch_train.py:roi_align + autograd in float64.  feats: numpy [N][H][W][C] per level; gout [R][49][C].
    Returns the forward [R][49][C] and the gradients [N][H][W][C]."""
    from oracle import torch_train as tt
    fd = [torch.from_numpy(f).double().permute(0, 3, 1, 2).contiguous().requires_grad_() for f in feats]
    R, C = len(rois), feats[0].shape[3]
    out = tt.roi_align(fd, torch.from_numpy(rois[:, 0]).long(), torch.from_numpy(rois[:, 1:]))        # [R, C, 7, 7]
    out.backward(torch.from_numpy(gout).double().view(R, 7, 7, C).permute(0, 3, 1, 2))
    grads = [f.grad.permute(0, 2, 3, 1).numpy() if f.grad is not None else np.zeros(f.permute(0, 2, 3, 1).shape) for f in fd]
    return out.detach().permute(0, 2, 3, 1).reshape(R, 49, C).numpy(), grads


def test_roi_set_reaches_all_nine_merge_patterns_and_every_edge():
    """The census of the section's RoIs by the numpy restatement of roi_sample / roi_level: all nine (row, column) sharing patterns
    of the merge kernel with all four samples valid, border clamps and invalid samples on each side of each axis, boxes thinner
    than a feature pixel on each axis, boxes fully outside, all four levels."""
    seen = roi_census(roi_set(), ROI_DIMS)
    assert seen["patterns"] == {(r, c) for r in range(3) for c in range(3)}, seen["patterns"]
    assert seen["clamp"] == {0, 1} and seen["thin"] == {0, 1} and seen["levels"] == {0, 1, 2, 3}
    assert seen["invalid"] == {(0, "low"), (0, "high"), (1, "low"), (1, "high")}
    assert seen["outside"] >= 2 and len(seen["invalid_patterns"]) >= 3


@pytest.fixture(scope="module")
def roi_case(T):
    """The RoI set on gaussian features / gradients at C = 256 with its float64 autograd reference (computed once)."""
    torch, ops = T
    rois = roi_set()
    rs = np.random.RandomState(21)
    feats = [rs.randn(2, h, w, 256).astype(np.float32) for h, w in ROI_DIMS]
    gout = rs.randn(len(rois), 49, 256).astype(np.float32)
    fwd, grads = _roi_autograd(torch, rois, feats, gout)
    return rois, feats, gout, fwd, grads


def test_roi_align_c256_forward_backward_vs_autograd(T, roi_case):
    """roi_align_train_kernel and the merge kernel at C = 256 == float64 autograd to 1e-5 of the largest magnitude (the rule of
    test_roi_align_forward_backward_vs_autograd, which runs C = 16 and so the other backward kernel); gfeats is ADDED to."""
    torch, ops = T
    rois, feats, gout, fwd, grads = roi_case
    got = ops.roi_align([torch.from_numpy(f).cuda() for f in feats], torch.from_numpy(rois).cuda())
    _close(_cpu(got), fwd, 1e-5, "RoIAlign forward, C = 256")
    outside = [r for r, roi in enumerate(rois) if not np.abs(fwd[r]).any()]
    assert len(outside) >= 2 and all(not _cpu(got)[r].any() for r in outside), "boxes outside the map pool zeros"
    back = _roi_bwd(torch, ops, rois, gout)
    for l in range(4):
        _close(back[l], grads[l], 1e-5, "RoIAlign backward level %d, C = 256" % l)
    rs = np.random.RandomState(22)
    start = [rs.randn(*g.shape).astype(np.float32) for g in grads]
    back2 = _roi_bwd(torch, ops, rois, gout, start=start)
    for l in range(4):
        _close(back2[l], grads[l] + start[l], 1e-5, "RoIAlign backward onto a non-zero gfeats, level %d" % l)
        assert np.array_equal(back2[l], start[l] + back[l]), "the scatter is summed first and added once"


def test_roi_backward_merge_kernel_equals_the_plain_kernel_bit_for_bit(T, roi_case):
    """C = 256 (one atomic per distinct pixel of a bin, nine instantiations) against the C != 256 kernel (one atomic per term) run
    on the two 128-channel halves: both accumulate the same integers, so every bit agrees.  The fixed-point scale comes from
    max|gout| of a CALL, so the same largest value is planted in both halves."""
    torch, ops = T
    rois, _, gout, _, _ = roi_case
    gout = gout.copy(); gout[3, 5, 7] = gout[3, 5, 128 + 7] = 7.5          # |randn| stays below 7.5
    assert np.abs(gout).max() == 7.5
    whole = _roi_bwd(torch, ops, rois, gout)
    for half in (0, 1):
        part = _roi_bwd(torch, ops, rois, np.ascontiguousarray(gout[:, :, 128 * half:128 * half + 128]))
        for l in range(4):
            assert np.array_equal(whole[l][..., 128 * half:128 * half + 128], part[l]), "level %d, channels %d.." % (l, 128 * half)
    assert all(np.abs(w).max() > 0 for w in whole)


def test_roi_backward_is_order_independent_and_reproducible(T, roi_case):
    """What the fixed-point accumulation promises: the same bits on a second run and under any permutation of the RoI rows; a few
    hundred RoIs on the same pixels still match float64; an all-zero gout leaves gfeats untouched."""
    torch, ops = T
    rois, _, gout, _, grads = roi_case
    a = _roi_bwd(torch, ops, rois, gout); b = _roi_bwd(torch, ops, rois, gout)
    perm = np.random.RandomState(3).permutation(len(rois))
    c = _roi_bwd(torch, ops, np.ascontiguousarray(rois[perm]), np.ascontiguousarray(gout[perm]))
    for l in range(4):
        assert np.array_equal(a[l], b[l]), "two runs differ, level %d" % l
        assert np.array_equal(a[l], c[l]), "permuted RoIs differ, level %d" % l
    rs = np.random.RandomState(23)
    same = np.repeat(np.array([[1, 41.3, 33.9, 118.2, 102.4], [0, 10.2, 80.7, 150.1, 170.6]], np.float32), 150, axis=0)
    g2 = rs.randn(len(same), 49, 256).astype(np.float32)
    _, want = _roi_autograd(torch, same, [np.zeros((2, h, w, 256), np.float32) for h, w in ROI_DIMS], g2)
    got = _roi_bwd(torch, ops, same, g2)
    touched = 0
    for l in range(4):
        if np.abs(want[l]).max() > 0:
            _close(got[l], want[l], 1e-5, "300 RoIs on two boxes, level %d" % l); touched += 1
        else:
            assert not got[l].any()
    assert touched >= 1
    start = [rs.randn(2, h, w, 256).astype(np.float32) for h, w in ROI_DIMS]
    kept = _roi_bwd(torch, ops, rois, np.zeros_like(gout), start=start)
    for l in range(4):
        assert kept[l].tobytes() == start[l].tobytes(), "an all-zero gout changed gfeats, level %d" % l


def test_roi_backward_fixed_point_scale_keeps_small_gradients(T):
    """One element of 2^20 among values near 1.  Bound per element of gfeats, from the float64 scatter's own sum of |terms| (A), term
    count (n) and value (v), with the float32 sample weights as operands: each term carries two float32 roundings (the weight
    product and its product with gout / 4; relative 2^-24 each), at most half a fixed-point quantum (the quantum is at most
    2^-39 of max|gout|), and the sum is rounded to float32 once when it is added to the zero gfeats:
        |got - v| <= A (2^-23 + 2^-48) + n 2^-40 max|gout| + (|v| + the two terms before) 2^-24.
    The small gradients far from the large one must survive: non-zero wherever the reference exceeds twice its bound."""
    torch, ops = T
    rois = roi_set()
    rs = np.random.RandomState(31)
    gout = ((rs.rand(len(rois), 49, 256) + 0.5) * rs.choice([-1.0, 1.0], (len(rois), 49, 256))).astype(np.float32)
    big = 27                                                        # a level-1 box of the random part
    assert roi_setup_np(rois[big, 1:], ROI_DIMS)[0] == 1
    gout[big, 24, 100] = 2.0 ** 20
    sums, mags, cnts = roi_scatter_f64(rois, gout, ROI_DIMS, 2)
    got = _roi_bwd(torch, ops, rois, gout)
    gmax = float(np.abs(gout).max())
    checked = 0
    for l in range(4):
        pre = mags[l] * (2.0 ** -23 + 2.0 ** -48) + cnts[l] * 2.0 ** -40 * gmax
        bound = pre + (np.abs(sums[l]) + pre) * 2.0 ** -24
        err = np.abs(got[l].astype(np.float64) - sums[l])
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        assert (err <= bound).all(), "level %d: |got - ref| = %.3g > bound %.3g at %s" % (l, err[worst], bound[worst], worst)
        must = np.abs(sums[l]) > 2 * bound
        assert (got[l][must] != 0).all(), "level %d: small gradients were quantised away" % l
        checked += int(must.sum())
        if l != 1:
            assert must.sum() > 0.5 * (cnts[l] > 0).sum(), "the bound is loose enough to hide the small gradients at level %d" % l
    assert checked > 100000


def test_roi_backward_drops_non_finite_gradients(T, roi_case):
    """NaN and +-Inf in a few places of gout give the result of those places set to zero, bit for bit (non-finite gradients are
    reported by the loss check, not spread, and they must not set the fixed-point scale), on both backward kernels."""
    torch, ops = T
    rois, _, gout, _, _ = roi_case
    for C in (256, 128):
        clean = np.ascontiguousarray(gout[:, :, :C]); dirty = clean.copy()
        for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf)):
            clean[3 + 11 * k, 7 * k, 5 + 40 * k % C] = 0.0; dirty[3 + 11 * k, 7 * k, 5 + 40 * k % C] = v
        want = _roi_bwd(torch, ops, rois, clean); got = _roi_bwd(torch, ops, rois, dirty)
        for l in range(4):
            assert np.isfinite(got[l]).all(), "C = %d level %d: a non-finite gradient was spread" % (C, l)
            assert np.array_equal(got[l], want[l]), "C = %d level %d: differs from the run with zeros in those places" % (C, l)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the paths behind the environment switches (read once per process): one fresh child process per setting
# ---------------------------------------------------------------------------------------------------------------------
SWITCH_ENV = ("CALD_WGRAD_PW", "CALD_WGRAD_TAB", "CALD_WGRAD_BK", "CALD_WGRAD_TARGET", "CALD_ROI_BWD_MERGE")
SWITCH_SETTINGS = [{}, {"CALD_WGRAD_PW": "0"}, {"CALD_WGRAD_TAB": "0"}, {"CALD_WGRAD_BK": "32"}, {"CALD_WGRAD_TARGET": "64"},
                   {"CALD_WGRAD_TARGET": "4096"}, {"CALD_ROI_BWD_MERGE": "0"}]
CHILD_CONV = ["pw_q1_cout1", "pw_ragged", "pw_q1793", "pw_seam", "tab_2x3_map", "tab_s2_odd", "tab_1x1_s2_odd", "tab_ragged_seam",
              "tab_fills_seam", "gen_1x2_map", "gen_j_tail", "gen_cin4_7x7", "gen_s2_odd", "gen_ragged_seam"]
CHILD_LINEAR = [(513, 64, 256, 1), (200, 49 * 64, 128, 49)]


def child_main(out_prefix):
    """Run by tests/_train_variant_child.py in a process of its own: the fixed subset of the exact-integer cases (each asserted
    against its integer sums there) and the section-3 RoI backward at C = 256; results to <prefix>_exact.npy, <prefix>_roi.npy, and
    the plans the library answered to <prefix>_plan.json."""
    import torch
    from cald_amd import train_ops as ops
    exact, plans = [], {}
    for name in CHILD_CONV:
        cs = [c for c in WGRAD_CASES if c["name"] == name][0]
        pl = _conv_plan(ops, cs)
        plans[name] = [pl.kernel.decode(), pl.reduce_kernel.decode(), int(pl.S), int(pl.chunk)]
        exact += [a.ravel() for a in run_conv_wgrad_case(torch, ops, cs)]
    for case in CHILD_LINEAR:
        pl = ops.linear_wgrad_plan(case[0], case[1], case[2], (case[2] + 3) // 4 * 4, case[3])
        plans["linear_%d_%d_%d_%d" % case] = [pl.kernel.decode(), pl.reduce_kernel.decode(), int(pl.S), int(pl.chunk)]
        exact += [a.ravel() for a in run_linear_wgrad_case(torch, ops, case)]
    rois = roi_set()
    gout = np.random.RandomState(21).randn(len(rois), 49, 256).astype(np.float32)
    back = _roi_bwd(torch, ops, rois, gout)
    np.save(out_prefix + "_exact.npy", np.concatenate(exact))
    np.save(out_prefix + "_roi.npy", np.concatenate([b.ravel() for b in back]))
    with open(out_prefix + "_plan.json", "w") as f:
        json.dump(plans, f)


def test_environment_switch_paths_in_child_processes(T, tmp_path):
    """CALD_WGRAD_PW=0, CALD_WGRAD_TAB=0, CALD_WGRAD_BK=32, CALD_WGRAD_TARGET=64 / 4096, CALD_ROI_BWD_MERGE=0:
    the library reads each once per process, so each setting gets a fresh child (one after another, stopping at the first failure).
    Every child asserts its exact-integer cases against the integer sums; here the results of every setting must be IDENTICAL to the
    default run's, the plans must show that the switch took effect, the un-merged fixed-point RoI backward must equal the merged one
    bit for bit, and the default backward is held to float64 at the 1e-5 rule."""
    torch, ops = T
    base = {k: v for k, v in os.environ.items() if k not in SWITCH_ENV}
    res = []
    for i, setting in enumerate(SWITCH_SETTINGS):
        prefix = str(tmp_path / ("run%d" % i))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_train_variant_child.py"), prefix, ROOT], env=dict(base, **setting),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, "child with %s failed:\n%s" % (setting, (r.stdout + r.stderr)[-3000:])
        res.append((np.load(prefix + "_exact.npy"), np.load(prefix + "_roi.npy"), json.load(open(prefix + "_plan.json"))))
    exact0, roi0, plan0 = res[0]
    assert exact0.size > 1000000 and np.isfinite(exact0).all()
    for setting, (exact, roi, plan) in zip(SWITCH_SETTINGS, res):
        assert exact.tobytes() == exact0.tobytes(), "exact-integer results moved under %s" % setting
    kernels = lambda plan: {v[0] for v in plan.values()}
    assert kernels(plan0) == {"wgrad_kernel<true,16,1>", "wgrad_kernel<true,16,2>", "wgrad_kernel<true,16>"}
    assert kernels(res[1][2]) == {"wgrad_kernel<true,16,2>", "wgrad_kernel<true,16>"}, "CALD_WGRAD_PW=0: pointwise shapes take the other kernels"
    assert kernels(res[2][2]) == {"wgrad_kernel<true,16,1>", "wgrad_kernel<true,16>"}, "CALD_WGRAD_TAB=0: no offset table"
    assert kernels(res[3][2]) == {"wgrad_kernel<true,16,1>", "wgrad_kernel<true,16,2>", "wgrad_kernel<true,32>"}, "CALD_WGRAD_BK=32"
    for k in (4, 5):
        assert kernels(res[k][2]) == kernels(plan0)
    assert any(res[4][2][n][2] < plan0[n][2] for n in plan0) and all(res[4][2][n][2] <= plan0[n][2] for n in plan0), "CALD_WGRAD_TARGET=64: fewer splits"
    assert any(res[5][2][n][2] > plan0[n][2] for n in plan0) and all(res[5][2][n][2] >= plan0[n][2] for n in plan0), "CALD_WGRAD_TARGET=4096: more splits"
    for k in (1, 2, 3, 4, 5, 6):
        assert res[k][1].tobytes() == roi0.tobytes(), "the fixed-point RoI backward moved under %s" % SWITCH_SETTINGS[k]
    rois = roi_set()
    gout = np.random.RandomState(21).randn(len(rois), 49, 256).astype(np.float32)
    _, grads = _roi_autograd(torch, rois, [np.zeros((2, h, w, 256), np.float32) for h, w in ROI_DIMS], gout)
    off = 0
    for l, g in enumerate(grads):
        _close(roi0[off:off + g.size].reshape(g.shape), g, 1e-5, "default RoI backward in the child, level %d" % l)
        off += g.size


# ---------------------------------------------------------------------------------------------------------------------
# 5. the small backward kernels, exact on integer data, at sizes with and without a tail block in the float4 grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hh,ww", [((13, 7), (14, 7)), ((14, 7), (13, 7)), ((1, 1), (2, 1)), ((2, 1), (3, 2)), ((3, 2), (1, 1)),
                                   ((13, 7), (3, 2)), ((3, 2), (14, 7))], ids=str)
def test_upsample_backward_exact_at_uneven_ratios(T, hh, ww):
    """upsample_bwd_kernel == autograd of F.interpolate(size=fine, mode="nearest") where the fine size is not twice the coarse one
    (real pyramids: Hf = 2 Hc - 1, Hc = 1), added onto a non-zero coarse tensor; integer data, exact."""
    torch, ops = T
    import torch.nn.functional as F
    (Hf, Hc), (Wf, Wc) = hh, ww
    rs = np.random.RandomState(Hf * 100 + Wf)
    N, C = 2, 8
    fine = torch.from_numpy(rs.randint(-4, 5, (N, Hf, Wf, C)).astype(np.float32)); c0 = torch.from_numpy(rs.randint(-4, 5, (N, Hc, Wc, C)).astype(np.float32))
    cd = torch.zeros(N, C, Hc, Wc, dtype=torch.float64, requires_grad=True)
    F.interpolate(cd, size=(Hf, Wf), mode="nearest").backward(fine.permute(0, 3, 1, 2).double())
    got = ops.upsample_bwd_(fine.cuda(), c0.cuda().clone())
    _exact(_cpu(got), (cd.grad.permute(0, 2, 3, 1) + c0.double()).numpy(), "upsample backward %s x %s" % (hh, ww))


VEC_SIZES = [(1, 1), (15, 17), (16, 16), (1, 257)]         # H x W with C = 4, N = 1: 1, 255, 256, 257 float4 -- no tail, a full last block, one over


@pytest.mark.parametrize("hw", VEC_SIZES, ids=str)
def test_dilate_exact(T, hw):
    """dilate_kernel (stride-2 scatter onto the stride-1 grid, including the extra rows / columns of an even input size) against its
    index rule in numpy, at float4 counts of 1, 255, 256, 257 and at odd and even H, W."""
    torch, ops = T
    for (H, W) in (hw, (hw[1], hw[0]), (hw[0] + 1, hw[1]), (6, 5)):
        rs = np.random.RandomState(H * 1000 + W)
        N, Cc = (1, 4) if (H, W) != (6, 5) else (2, 12)
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        g = rs.randint(-9, 10, (N, Ho, Wo, Cc)).astype(np.float32)
        want = np.zeros((N, H, W, Cc), np.float32)
        want[:, ::2, ::2] = g[:, :(H + 1) // 2, :(W + 1) // 2]
        _exact(_cpu(ops.dilate(torch.from_numpy(g).cuda(), 2, H, W)), want, "dilate to %dx%d" % (H, W))


@pytest.mark.parametrize("n4", [1, 255, 256, 257])
def test_relu_backward_and_add_exact(T, n4):
    """relu_bwd_kernel with act, scale, both, neither (power-of-two scales: exact) and add_kernel with and without b, at float4
    counts of 1, 255, 256, 257; and relu_bwd with C = 12, where the scale index wraps inside a block."""
    torch, ops = T
    rs = np.random.RandomState(n4)
    for rows, Cc in ((n4, 4), (n4, 12)):
        g = rs.randint(-9, 10, (rows, Cc)).astype(np.float32); act = rs.randint(-1, 2, (rows, Cc)).astype(np.float32); sc = _pow2(rs, Cc)
        for use_act in (False, True):
            for use_sc in (False, True):
                got = ops.relu_bwd_(torch.from_numpy(g).cuda(), torch.from_numpy(act).cuda() if use_act else None, torch.from_numpy(sc).cuda() if use_sc else None)
                want = g * ((act > 0) if use_act else 1) * (sc[None, :] if use_sc else 1)
                _exact(_cpu(got), want.astype(np.float32), "relu_bwd rows %d C %d act %s scale %s" % (rows, Cc, use_act, use_sc))
    a = rs.randint(-99, 100, 4 * n4).astype(np.float32); b = rs.randint(-99, 100, 4 * n4).astype(np.float32)
    _exact(_cpu(ops.add(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())), a + b, "add")
    _exact(_cpu(ops.add(torch.from_numpy(a).cuda())), a, "add without b (copy)")
