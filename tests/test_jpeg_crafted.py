"""Input side: the JPEG decoder on crafted streams no libjpeg encoder writes.

Every JPEG of tests/test_jpeg.py and tests/test_jpeg_progressive.py comes from Pillow's encoder: one scan script, table
ids 0 and 1, 8-bit DQT, one DRI, coefficients a forward DCT of 8-bit pixels produces.  The files here come from
tests/_jpeg_writer.py, which codes chosen quantised coefficients under a chosen script, tables and marker layout.

Chain of evidence: the writer is checked first (Pillow decodes every encoding of one coefficient set to the same pixels,
different sets to different pixels, and gray files to the float64 inverse DCT of their coefficients within IEEE 1180's
peak error of 1) -> live Pillow == cald_jpeg_decode_host (and the C oracle for baseline files) -> the HIP decoder, bit
for bit, in one shuffled batch whose outputs are views of a guarded arena.

In range: every crafted case but the over-range one keeps its float64 IDCT + 128 inside [-384, 639] and every
|coef * q| <= 1023 + q/2.  The over-range case (tests/golden/jpeg_crafted.npz, tools/make_golden_jpeg_crafted.py) is
where a wrapping range limit and libjpeg-turbo's saturating one part: it pins the decoder to saturation.  Dequantised
values beyond int16 are outside the promise (turbo's SIMD saturates its intermediates) and are not tested.
"""
import functools
import io

import numpy as np
import pytest

import _jpeg_writer as jw

try:
    from PIL import Image
except Exception:  # pragma: no cover
    Image = None

needs_pillow = pytest.mark.skipif(Image is None, reason="Pillow not importable")

SIZES = [(1, 1), (2, 3), (9, 9), (17, 23), (33, 39), (40, 56)]                  # (H, W)
SAMPLINGS = {"gray": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}         # luma (h, v)
ZZ = np.array(jw.ZIGZAG)


def _pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ------------------------------------------------------------------------------------------------ float64 reference
_M = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _float_idct(coef_zz, q_zz):
    """[bh][bw][64] zigzag coefficients x zigzag table -> float64 plane [bh*8][bw*8] (no level shift)."""
    bh, bw, _ = coef_zz.shape
    nat = np.zeros((bh, bw, 64))
    nat[:, :, ZZ] = coef_zz * np.asarray(q_zz, np.float64)
    px = np.einsum("ux,abuv,vy->abxy", _M, nat.reshape(bh, bw, 8, 8), _M)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


# ------------------------------------------------------------------------------------------------ coefficient sets
def _fit_block(blk, q):
    """Halves a block's AC coefficients until its float IDCT + 128 is inside [-380, 635]."""
    while True:
        f = _float_idct(blk.reshape(1, 1, 64), q)
        if f.min() >= -508 and f.max() <= 507:
            return blk
        assert blk[1:].any()
        blk[1:] = np.trunc(blk[1:] / 2).astype(np.int64)


def _coefs(rng, bh, bw, uh, uw, q):
    """Blocks of six kinds: DC only; one large coefficient; three far-apart ones of mixed magnitude (zero runs past 15 in
    first and refinement scans); dense small; a dozen medium; only k = 1 and k = 63.  Blocks outside the component's own
    uh x uw grid (MCU padding) carry a DC value only: interleaved scans code them, single-component scans do not."""
    q = np.asarray(q, np.int64)
    lim = 1023 // q
    coef = np.zeros((bh, bw, 64), np.int64)
    for by in range(bh):
        for bx in range(bw):
            blk = coef[by, bx]
            blk[0] = rng.integers(-lim[0], lim[0] + 1) if rng.integers(0, 4) else rng.integers(-3, 4)
            if by >= uh or bx >= uw:
                continue
            kind = int(rng.integers(0, 6))
            if kind == 1:
                k = int(rng.integers(1, 64))
                blk[k] = rng.choice([-1, 1]) * lim[k]
            elif kind == 2:
                for k, m in zip((int(rng.integers(1, 4)), int(rng.integers(28, 34)), int(rng.integers(58, 64))), rng.permutation([9, 1, 2])):
                    blk[k] = rng.choice([-1, 1]) * min(int(m), lim[k])
            elif kind == 3:
                on = rng.random(63) < 0.6
                blk[1:] = np.where(on, rng.integers(-4, 5, 63), 0)
            elif kind == 4:
                for k in rng.choice(np.arange(1, 64), 12, replace=False):
                    blk[k] = rng.integers(-40, 41)
            elif kind == 5:
                blk[1] = rng.integers(-20, 21)
                blk[63] = rng.choice([-1, 1]) * int(rng.integers(1, 12))
            np.clip(blk, -lim, lim, out=blk)
            _fit_block(blk, q)
    return coef


def _qtab(rng, lo, hi):
    return [int(v) for v in rng.integers(lo, hi + 1, 64)]


def _geometry(H, W, samp):
    """[(h, v, bh, bw, uh, uw)] per component."""
    if samp is None:
        return [(1, 1, -(-H // 8), -(-W // 8), -(-H // 8), -(-W // 8))]
    h, v = samp
    mcux, mcuy = -(-W // (8 * h)), -(-H // (8 * v))
    out = [(h, v, mcuy * v, mcux * h, -(-H // 8), -(-W // 8))]
    dw, dh = -(-W // h), -(-H // v)
    out += [(1, 1, mcuy, mcux, -(-dh // 8), -(-dw // 8))] * 2
    return out


def _frame(rng, H, W, samp, qtabs, tq=(0, 1, 1), cids=(1, 2, 3)):
    """A frame with fresh in-range coefficients.  qtabs = {id: (zigzag values, sixteen_bit)}."""
    comps = []
    for i, (h, v, bh, bw, uh, uw) in enumerate(_geometry(H, W, samp)):
        comps.append(jw.Component(cids[i], h, v, tq[i], _coefs(rng, bh, bw, uh, uw, qtabs[tq[i]][0])))
    return jw.Frame(W, H, comps, qtabs)


def _reframe(frame, qtabs=None, tq=None, **kw):
    """The same coefficients under other tables / table selectors / frame parameters."""
    comps = [jw.Component(c.cid, c.h, c.v, c.tq if tq is None else tq[i], c.coef) for i, c in enumerate(frame.comps)]
    return jw.Frame(frame.W, frame.H, comps, frame.qtabs if qtabs is None else qtabs, **kw)


# ------------------------------------------------------------------------------------------------ scan scripts
def script_libjpeg(nc):
    if nc == 1:
        return [([0], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([0], 6, 63, 0, 2), ([0], 1, 63, 2, 1), ([0], 0, 0, 1, 0), ([0], 1, 63, 1, 0)]
    return [([0, 1, 2], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([2], 1, 63, 0, 1), ([1], 1, 63, 0, 1), ([0], 6, 63, 0, 2), ([0], 1, 63, 2, 1),
            ([0, 1, 2], 0, 0, 1, 0), ([2], 1, 63, 1, 0), ([1], 1, 63, 1, 0), ([0], 1, 63, 1, 0)]


def script_bands(nc):
    """Non-interleaved DC, last component first, DC and every band from Al = 3 down to 0, bands 63..63 / 1..1 / 2..62."""
    s = []
    for c in reversed(range(nc)):
        for ss, se in ((0, 0), (63, 63), (1, 1), (2, 62)):
            s.append(([c], ss, se, 0, 3))
            s += [([c], ss, se, al + 1, al) for al in (2, 1, 0)]
    return s


def script_single(nc):
    return [(list(range(nc)), 0, 0, 0, 0)] + [([c], 1, 63, 0, 0) for c in range(nc)]


SCRIPTS = {"libjpeg": script_libjpeg, "bands": script_bands, "single": script_single}
DRI_CYCLE = [2, 0, 1, 3, 0, 5, 1]          # per scan: changes, includes 0; interval 1 runs the RSTn index past RST7


# ------------------------------------------------------------------------------------------------ case table
class Case:
    def __init__(self, name, blob, stats, group, progressive, frame):
        self.name, self.blob, self.stats, self.group, self.progressive = name, blob, stats, group, progressive
        self.frame = frame             # the coefficients, with the quantisation tables that are in effect at decode time


def _encodings(name, frame, k):
    """The eight standard encodings of one coefficient set: baseline x 2, three scripts x (no restarts, per-scan DRI)."""
    nc = len(frame.comps)
    out = []
    blob, st = jw.write_sequential(frame, jfif=bool(k & 1))
    out.append(Case(name + "/base", blob, st, name, False, frame))
    blob, st = jw.write_sequential(frame, sof=0xC1, tables=jw.skewed, merged_dht=False, merged_dqt=False, restart=1 + k % 3,
                                   table_ids=[(0, 0), (1, 1), (2, 2)][:nc], jfif=not (k & 1))
    out.append(Case(name + "/base_rst", blob, st, name, False, frame))
    for j, (sn, sf) in enumerate(SCRIPTS.items()):
        pol = {"libjpeg": jw.flat, "bands": jw.skewed, "single": jw.long_codes if k & 1 else jw.flat}[sn]
        for dri in (None, DRI_CYCLE[(k + j) % 7:] + DRI_CYCLE[:(k + j) % 7]):
            blob, st = jw.write_progressive(frame, sf(nc), tables=pol, dri=dri, merged_dht=bool((k + j) & 1), jfif=bool(k & 2),
                                            ac_id=(k + j) % 4)
            out.append(Case("%s/%s%s" % (name, sn, "_dri" if dri else ""), blob, st, name, True, frame))
    return out


def _sparse_large():
    """Gray 1024 x 2048 = 32768 blocks, three AC bands, each sent at Al = 1 and refined to Al = 0.
    Band 1..2 is empty everywhere: each of its scans is one EOB run of 32768, which must split at 0x7FFF.
    Band 3..5 is empty but for the last block, which has a coefficient with history (magnitude 3: new at Al = 1, correction
    bit 1 at Al = 0) and one that is new at Al = 0 (magnitude 1): a run of exactly 0x7FFF, category 14, ends at it.
    Band 6..63: block P_r has the same two kinds of coefficient, and P_r+1 follows it 2^r + r blocks on, r = 0..13, so in
    the refinement scan an EOB run of every category 0..13 ends at a block where a mis-read run length misplaces a new
    coefficient.  From r = 2 on the block after P_r has history only: it stays inside the run and its correction bits are
    carried behind the EOBn symbol, across the whole run."""
    rng = np.random.default_rng(77)
    H, W = 1024, 2048
    coef = np.zeros((128 * 256, 64), np.int64)
    coef[:, 0] = rng.integers(-60, 61, len(coef))
    coef[-1, 3], coef[-1, 5] = -3, 1
    at = 0
    for r in range(15):
        coef[at, 6 + r] = (2 + (r & 1)) * (-1 if r & 2 else 1)          # history: correction bit 0 or 1
        coef[at, 30 + r] = -1 if r & 1 else 1                           # new in the refinement scan
        if r >= 2:
            coef[at + 1, 40], coef[at + 1, 41] = (3 if r & 2 else -3), 2
        at += (1 << r) + r                                              # + P_r's own end of block: a run of 2^r + r
    q = {0: ([2] * 64, False)}
    frame = jw.Frame(W, H, [jw.Component(1, 1, 1, 0, coef.reshape(128, 256, 64))], q)
    script = [([0], 0, 0, 0, 1), ([0], 1, 2, 0, 1), ([0], 3, 5, 0, 1), ([0], 6, 63, 0, 1), ([0], 1, 2, 1, 0), ([0], 0, 0, 1, 0),
              ([0], 6, 63, 1, 0), ([0], 3, 5, 1, 0)]
    blob, st = jw.write_progressive(frame, script, tables=jw.flat)
    base, st0 = jw.write_sequential(frame)
    return [Case("large/prog", blob, st, "large", True, frame), Case("large/base", base, st0, "large", False, frame)]


@functools.lru_cache(maxsize=None)
def _cases():
    """Every in-range crafted file, deterministic."""
    rng = np.random.default_rng(20240229)
    out, k = [], 0
    qy = {0: (_qtab(rng, 1, 12), False), 1: (_qtab(rng, 2, 20), False), 2: (_qtab(rng, 1, 6), False)}
    for sname, samp in SAMPLINGS.items():
        for H, W in SIZES:
            frame = _frame(rng, H, W, samp, qy, tq=(0, 1, 2))
            out += _encodings("%s_%dx%d" % (sname, H, W), frame, k)
            k += 1

    # SOF1 with table ids 3, 1, 2 in one merged DHT; three distinct table pairs; arbitrary component ids
    f = _frame(rng, 17, 23, (2, 2), qy, cids=(7, 200, 9))
    blob, st = jw.write_sequential(f, sof=0xC1, table_ids=[(3, 3), (1, 1), (2, 2)], tables=jw.skewed, jfif=False)
    out.append(Case("sof1_ids", blob, st, "sof1_ids", False, f))
    blob, st = jw.write_progressive(f, script_libjpeg(3), dc_ids=[3, 1, 2], ac_id=3, tables=jw.skewed)
    out.append(Case("sof1_ids/prog", blob, st, "sof1_ids", True, f))

    # every code word longer than the 9-bit lookahead; fill bytes; trailing bytes with RST0 and SOS in them
    trailing = b"\xff\xd0tail\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00\xff\xd9\xff"
    for sname, samp, (H, W) in (("gray", None, (33, 39)), ("420", (2, 2), (17, 23)), ("422", (2, 1), (33, 39))):
        f = _frame(rng, H, W, samp, qy)
        name = "edges_" + sname
        for tag, kw in (("long", dict(tables=jw.long_codes)), ("fill", dict(fill=2)), ("trail", dict(trailing=trailing)),
                        ("all", dict(tables=jw.long_codes, fill=1, trailing=trailing))):
            blob, st = jw.write_sequential(f, restart=2, **kw)
            out.append(Case("%s/base_%s" % (name, tag), blob, st, name, False, f))
            blob, st = jw.write_progressive(f, script_bands(len(f.comps)), dri=DRI_CYCLE, **kw)
            out.append(Case("%s/prog_%s" % (name, tag), blob, st, name, True, f))

    # 16-bit DQT
    q16 = {0: (_qtab(rng, 200, 340), True), 1: (_qtab(rng, 256, 511), True)}
    for sname, samp in (("gray", None), ("420", (2, 2))):
        f = _frame(rng, 17, 23, samp, q16)
        out += _encodings("dqt16_" + sname, f, k)
        k += 1

    # a DQT redefined before a component's first scan takes effect; after it, it does not
    qa, qb, qc = (_qtab(rng, 1, 9), False), (_qtab(rng, 3, 14), False), (_qtab(rng, 20, 90), False)
    eff = _frame(rng, 33, 39, None, {0: qb})
    com = jw.segment(0xFE, b"between scans") + jw.segment(0xE5, b"app5")
    blob, st = jw.write_progressive(_reframe(eff, {0: qa}), script_libjpeg(1), tables=jw.skewed,
                                    between={0: jw.dqt_segment({0: qb}), 1: jw.dqt_segment({0: qc}), 3: com + jw.dqt_segment({0: qa, 1: qc})})
    out.append(Case("dqt_redefined_gray/prog", blob, st, "dqt_redefined_gray", True, eff))
    blob, st = jw.write_sequential(eff)
    out.append(Case("dqt_redefined_gray/base", blob, st, "dqt_redefined_gray", False, eff))
    # colour, chroma first: Cr latches table 1 at its first scan, the table is then redefined, Cb latches the new one
    qy_a, qy_b, qc_a, qc_b = ((_qtab(rng, 1, 9), False) for _ in range(4))
    eff = _frame(rng, 17, 23, (2, 2), {0: qy_b, 1: qc_b, 2: qc_a}, tq=(0, 1, 2))
    prog = _reframe(eff, {0: qy_a, 1: qc_a}, tq=(0, 1, 1))
    s = script_bands(3)                                  # scans 0..15 component 2, 16..31 component 1, 32..47 component 0
    blob, st = jw.write_progressive(prog, s, tables=jw.skewed, dri=DRI_CYCLE,
                                    between={5: jw.dqt_segment({1: qc_b}), 16: com, 20: jw.dqt_segment({0: qy_b, 1: qc}),
                                             33: jw.dqt_segment({0: qc, 1: qc, 2: qc}, merged=False)})
    out.append(Case("dqt_redefined_420/prog", blob, st, "dqt_redefined_420", True, eff))
    blob, st = jw.write_sequential(eff, table_ids=[(0, 0), (1, 1), (2, 2)])
    out.append(Case("dqt_redefined_420/base", blob, st, "dqt_redefined_420", False, eff))

    return tuple(out + _sparse_large())


@functools.lru_cache(maxsize=None)
def _refusals():
    """name -> (file, Pillow decodes it).  Files the parser must sort HOST_ONLY; none of them ever goes to a GPU."""
    rng = np.random.default_rng(5)
    q = {0: (_qtab(rng, 1, 12), False), 1: (_qtab(rng, 2, 20), False)}
    f = _frame(rng, 17, 23, (1, 1), q)
    g = _frame(rng, 17, 23, None, q)

    def odd(h, v):
        mcux, mcuy = -(-23 // (8 * h)), -(-17 // (8 * v))
        comps = [jw.Component(1, h, v, 0, _coefs(rng, mcuy * v, mcux * h, 3, 3, q[0][0]))]
        comps += [jw.Component(i, 1, 1, 1, _coefs(rng, mcuy, mcux, 1, 1, q[1][0])) for i in (2, 3)]
        return jw.Frame(23, 17, comps, q)
    ac = [([c], 1, 63, 0, 0) for c in range(3)]
    out = {
        "multi_scan_baseline": (jw.write_sequential(f, scans=[[0], [1], [2]])[0], True),
        "two_component_scan": (jw.write_progressive(f, [([0, 1], 0, 0, 0, 0), ([2], 0, 0, 0, 0)] + ac, dc_ids=[0, 1, 0])[0], True),
        "sampling_1x2": (jw.write_sequential(odd(1, 2))[0], True),
        "sampling_4x1": (jw.write_sequential(odd(4, 1))[0], True),
        "swapped_sos_baseline": (jw.write_sequential(f, sos_order=[0, 2, 1])[0], False),      # Pillow raises on it
        "ah_not_previous_al": (jw.write_progressive(g, [([0], 0, 0, 0, 2), ([0], 0, 0, 1, 0), ([0], 1, 63, 0, 0)])[0], True),
        "ac_before_dc": (jw.write_progressive(g, [([0], 1, 63, 0, 0), ([0], 0, 0, 0, 0)])[0], True),
        "incomplete_missing_band": (jw.write_progressive(g, [([0], 0, 0, 0, 0), ([0], 1, 5, 0, 0), ([0], 7, 63, 0, 0)])[0], True),
        "incomplete_al_left": (jw.write_progressive(f, [([0, 1, 2], 0, 0, 0, 1)] + ac)[0], True),
        "precision_12": (jw.write_sequential(_reframe(g, precision=12), sof=0xC1)[0], False),
    }
    return out


# ------------------------------------------------------------------------------------------------ CPU: the writer
@needs_pillow
def test_writer_pillow_sees_one_image_per_coefficient_set():
    """Pillow tolerates corrupt data silently, so the writer is not taken on faith: every encoding of a coefficient set
    decodes to the same pixels, and no two sets decode to the same pixels."""
    groups = {}
    for c in _cases():
        groups.setdefault(c.group, []).append((c.name, _pil_decode(c.blob)))
    assert len(groups) > 30
    for g, members in groups.items():
        assert len(members) >= 2, g
        for name, px in members[1:]:
            assert np.array_equal(px, members[0][1]), name
    seen = {}
    for g, members in groups.items():
        key = members[0][1].shape, members[0][1].tobytes()
        assert key not in seen, (g, seen.get(key))
        seen[key] = g


@needs_pillow
def test_writer_gray_files_decode_to_the_float_idct_of_their_coefficients():
    """|Pillow - round(float64 IDCT + 128)| <= 1 (IEEE 1180's peak error for the ISLOW IDCT) wherever the float value lies
    in [0.5, 254.5].  Checks the writer (coefficient placement, tables in effect), not the decoder."""
    n = 0
    for c in _cases():
        if len(c.frame.comps) != 1:
            continue
        comp = c.frame.comps[0]
        f = _float_idct(comp.coef, c.frame.qtabs[comp.tq][0])[:c.frame.H, :c.frame.W] + 128
        px = _pil_decode(c.blob)[:, :, 0].astype(np.float64)
        inside = (f >= 0.5) & (f <= 254.5)
        assert inside.any() or f.size < 8, c.name
        assert np.abs(px - np.round(f))[inside].max(initial=0) <= 1, c.name
        n += 1
    assert n > 60


def test_in_range_precondition_holds_for_every_case():
    frames = {id(c.frame): c.frame for c in _cases()}
    assert len(frames) > 30
    for fr in frames.values():
        for comp in fr.comps:
            q = np.asarray(fr.qtabs[comp.tq][0], np.float64)
            assert np.all(np.abs(comp.coef * q) <= 1023 + q / 2)
            f = _float_idct(comp.coef, q) + 128
            assert f.min() >= -384 and f.max() <= 639


def test_case_table_reaches_every_claimed_edge():
    """From the writer's own statistics: a claimed edge that is not in the bytes fails here."""
    cases = {c.name: c for c in _cases()}
    prog = [c for c in cases.values() if c.progressive]
    base = [c for c in cases.values() if not c.progressive]

    def total(cs, f):
        return sum(f(c.stats) for c in cs)
    for cs in (prog, base):
        lengths = set()
        for c in cs:
            lengths |= set(c.stats.code_lengths)
        assert lengths >= set(range(1, 17)), sorted(lengths)                 # the 9-bit lookahead and every maxcode length
    for l in range(10, 17):
        assert cases["edges_420/prog_long"].stats.code_lengths[l] > 0 and cases["edges_420/base_long"].stats.code_lengths[l] > 0
    assert not any(k < 10 for k in cases["edges_gray/base_long"].stats.code_lengths)
    assert total(prog, lambda s: s.zrl_first) > 0 and total(prog, lambda s: s.zrl_refine) > 0 and total(base, lambda s: s.zrl_first) > 0
    assert any(c.stats.restart_inside_eobrun for c in prog)
    assert max(c.stats.max_restarts_in_scan for c in prog) > 16 and max(c.stats.max_restarts_in_scan for c in base) > 8     # past RST7
    assert max(c.stats.max_carried_bits for c in prog) >= 8                  # correction bits carried across an EOB run
    assert max(c.stats.max_dc_category for c in cases.values()) >= 10 and max(c.stats.max_ac_size for c in cases.values()) == 10
    assert max(c.stats.dht_tables_max for c in base) == 6 and max(c.stats.dht_tables_max for c in prog) == 3
    large = cases["large/prog"].stats
    assert large.max_eobrun == 0x7FFF and large.eobrun_categories >= set(range(15))
    # refinement scans: a run of every category ends at a block with history and a new coefficient, where a mis-read run
    # length shows; runs of every category from 2 on carry correction bits behind their EOBn symbol
    assert large.refine_eobrun_before_history >= set(range(15)) and large.eobrun_carrying >= set(range(2, 14))
    assert max(c.stats.scans for c in prog) == 48
    # marker-level edges, read from the bytes
    for kind in ("base", "prog"):
        fill, trail = cases["edges_420/%s_fill" % kind].blob, cases["edges_420/%s_trail" % kind].blob
        assert b"\xff\xff\xff\xd0" in fill and fill.endswith(b"\xff\xff\xff\xd9")
        assert trail.endswith(b"\xff\xd9\xff") and b"\xff\xd9\xff\xd0tail\xff\xda" in trail
    assert b"\xff\xdb\x00\x83\x10" in cases["dqt16_gray/base_rst"].blob and b"\xff\xdb\x01\x04\x10" in cases["dqt16_420/libjpeg"].blob
    assert cases["dqt_redefined_gray/prog"].blob.count(b"\xff\xdb") == 4 and b"\xff\xfe\x00\x0fbetween scans" in cases["dqt_redefined_420/prog"].blob
    assert cases["sof1_ids"].blob.count(b"\xff\xc4") == 1 and b"\xff\xc1" in cases["sof1_ids"].blob
    dri = [c.blob.count(b"\xff\xdd\x00\x04") for c in prog if c.name.endswith("_dri")]
    assert min(dri) >= 1 and max(dri) >= 30                                  # the interval changes from scan to scan ...
    assert sum(b"\xff\xdd\x00\x04\x00\x00" in c.blob for c in prog) >= 40      # ... and goes back to 0
    # DC from Al = 3 with three refinements is the bands script
    assert [s[3:] for s in script_bands(1)[:4]] == [(0, 3), (3, 2), (2, 1), (1, 0)]
    # a luma block row and column shorter than the MCU-padded one
    for H, W, samp in ((17, 23, (2, 2)), (33, 39, (2, 1))):
        _, _, bh, bw, uh, uw = _geometry(H, W, samp)[0]
        assert uw < bw and (uh < bh or samp[1] == 1)


# ------------------------------------------------------------------------------------------------ CPU: the decoder
@needs_pillow
def test_host_decode_of_crafted_files_equals_live_pillow(oracle):
    from cald_amd import pool
    bad = []
    for c in _cases():
        H, W, _, kind = pool.jpeg_probe(c.blob)
        assert kind == (pool.JPEG_GPU_EXTENDED if c.progressive else pool.JPEG_BASELINE), c.name   # never HOST_ONLY
        want = _pil_decode(c.blob)
        assert (H, W) == want.shape[:2], c.name
        if not np.array_equal(pool.decode_jpeg_host(c.blob), want):
            bad.append(c.name)
        if not c.progressive:
            assert pool.jpeg_info(c.blob)[:2] == (H, W), c.name
            if not np.array_equal(oracle.jpeg_decode(c.blob), want):
                bad.append("oracle:" + c.name)
    assert not bad, bad


def _overrange_golden(golden):
    g = golden("jpeg_crafted")
    return [(str(g["name_%d" % i]), g["file_%d" % i].tobytes(), g["rgb_%d" % i]) for i in range(int(g["n"]))]


def test_overrange_blocks_saturate_as_recorded_pillow_does(oracle, golden):
    """IDCT outputs beyond the 10-bit range-limit table: libjpeg-turbo saturates where libjpeg's C table wraps.  The
    fixture is the record; where the installed Pillow and libjpeg-turbo are the recorded versions, live Pillow must
    reproduce it (another build may run another IDCT on such files, and then only the record holds)."""
    from cald_amd import pool
    cases = _overrange_golden(golden)
    recorded_build_is_installed = False
    if Image is not None:
        import PIL
        from PIL import features
        g = golden("jpeg_crafted")
        recorded_build_is_installed = (str(g["pillow_version"]), str(g["libjpeg_turbo_version"])) == (PIL.__version__, str(features.version("libjpeg_turbo")))
    assert [n for n, _, _ in cases] == [n for n, _ in jw.overrange_blobs()]
    over_range_files = 0
    for (name, blob, ref), (_, again) in zip(cases, jw.overrange_blobs()):
        assert blob == again, name                                         # the fixture's files are the writer's
        assert pool.jpeg_probe(blob)[3] == pool.JPEG_BASELINE
        assert np.array_equal(pool.decode_jpeg_host(blob), ref), name
        assert np.array_equal(oracle.jpeg_decode(blob), ref), name
        if recorded_build_is_installed:                                    # then live Pillow must reproduce the record
            assert np.array_equal(_pil_decode(blob), ref), name
        # where the float IDCT leaves [-384, 639] a 10-bit table index wraps; the record saturates there
        f = _overrange_float(name)
        out = (f < -384 - 2) | (f > 639 + 2)                               # clear of the fixed-point IDCT's error of 1
        assert np.array_equal(ref[:, :, 0][out], np.where(f[out] > 0, 255, 0)), name
        over_range_files += int(out.any())
    assert over_range_files == 5                                           # 600x6, 900x3, 900x6, 1023x3, 1023x6


def _overrange_float(name):
    """float64 IDCT + 128 of an over-range file, [8][32]."""
    f = dict(jw.overrange_frames())[name]
    c = f.comps[0]
    return _float_idct(c.coef, f.qtabs[c.tq][0]) + 128


def test_refusal_table_is_sorted_host_only():
    from cald_amd import pool
    for name, (blob, _) in _refusals().items():
        assert pool.jpeg_probe(blob)[3] == pool.JPEG_HOST_ONLY, name
        with pytest.raises(NotImplementedError):
            pool.jpeg_info(blob)
        with pytest.raises(NotImplementedError):
            pool.decode_jpeg_host(blob)


@needs_pillow
def test_refusal_table_files_are_jpegs_pillow_decodes():
    for name, (blob, decodable) in _refusals().items():
        if decodable:
            assert _pil_decode(blob).shape == (17, 23, 3), name


# ------------------------------------------------------------------------------------------------ GPU
def _arena(shapes, guard=256):
    """One uint8 arena of 0xA5 with `guard` bytes before, between and after the images; views into it."""
    import torch
    offs, at = [], guard
    for H, W in shapes:
        offs.append(at)
        at += H * W * 3 + guard
    arena = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    return arena, [arena[o:o + H * W * 3].view(H, W, 3) for o, (H, W) in zip(offs, shapes)], offs


def _guards_intact(arena, shapes, offs, guard=256):
    a = arena.cpu().numpy()
    keep = np.ones(a.size, bool)
    for o, (H, W) in zip(offs, shapes):
        keep[o:o + H * W * 3] = False
    return keep.sum() == guard * (len(shapes) + 1) and bool(np.all(a[keep] == 0xA5))


@pytest.mark.gpu
@needs_pillow
def test_gpu_crafted_batch_is_bit_exact_inside_a_guarded_arena(golden):
    import torch
    from cald_amd import pool
    cases = list(_cases())
    blobs = [c.blob for c in cases] + [b for _, b, _ in _overrange_golden(golden)]
    names = [c.name for c in cases] + [n for n, _, _ in _overrange_golden(golden)]
    want = [_pil_decode(c.blob) for c in cases] + [r for _, _, r in _overrange_golden(golden)]
    order = np.random.default_rng(3).permutation(len(blobs))             # baseline and progressive files interleave
    blobs, names, want = [blobs[i] for i in order], [names[i] for i in order], [want[i] for i in order]
    shapes = [w.shape[:2] for w in want]
    arena, outs, offs = _arena(shapes)
    pool.decode_images(blobs, outs=outs, fallback=None)
    torch.cuda.synchronize()
    assert _guards_intact(arena, shapes, offs)
    bad = [n for n, b, o, w in zip(names, blobs, outs, want)
           if not (np.array_equal(o.cpu().numpy(), w) and np.array_equal(w, pool.decode_jpeg_host(b)))]
    assert not bad, bad
    # the baseline subset through the strict entry point: the same bits
    base = [i for i, b in enumerate(blobs) if pool.jpeg_probe(b)[3] == pool.JPEG_BASELINE]
    assert 60 < len(base) < len(blobs) - 60
    arena2, outs2, offs2 = _arena([shapes[i] for i in base])
    pool.decode_jpeg_batch([blobs[i] for i in base], outs=outs2)
    torch.cuda.synchronize()
    assert _guards_intact(arena2, [shapes[i] for i in base], offs2)
    assert all(torch.equal(o, outs[i]) for i, o in zip(base, outs2))


@pytest.mark.gpu
@needs_pillow
def test_gpu_refusal_files_take_the_host_route_or_raise_before_any_launch():
    import torch
    from cald_amd import pool
    gpu = [c for c in _cases() if c.group in ("420_17x23", "gray_9x9")]
    refused = [b for b, ok in _refusals().values() if ok]
    blobs = []
    for i, c in enumerate(gpu):                                             # refused files between GPU files
        blobs.append(c.blob)
        if i < len(refused):
            blobs.append(refused[i])
    assert len(blobs) == len(gpu) + len(refused)
    want = [_pil_decode(b) for b in blobs]
    shapes = [w.shape[:2] for w in want]
    arena, outs, offs = _arena(shapes)
    pool.decode_images(blobs, outs=outs, fallback="pillow")
    torch.cuda.synchronize()
    assert _guards_intact(arena, shapes, offs)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert np.array_equal(o.cpu().numpy(), w), i
    arena.fill_(0xA5)
    with pytest.raises(NotImplementedError):
        pool.decode_images(blobs, outs=outs, fallback=None)
    torch.cuda.synchronize()
    assert bool((arena == 0xA5).all())                                      # raised before any launch: nothing was written
    with pytest.raises(NotImplementedError):
        pool.decode_jpeg_batch([gpu[0].blob, _refusals()["multi_scan_baseline"][0]], outs=outs[:2])
    assert bool((arena == 0xA5).all())
