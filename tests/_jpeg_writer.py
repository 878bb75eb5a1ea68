"""Test-only JPEG entropy coder in plain Python (ITU T.81 annexes B, C, F and G), for streams no libjpeg encoder writes.

It takes QUANTISED coefficients, not pixels: per component an integer array [bh][bw][64] in zigzag order, MCU-padded
(bw = mcux * h, bh = mcuy * v), so a test chooses every coefficient, table, marker and scan boundary of the file.  It
writes baseline / extended-sequential files (SOF0 / SOF1, any scan partition, table ids 0..3) and progressive files
(SOF2) under any scan script, and reports what the stream really contains (`Stats`), so that a test can assert that a
claimed edge is in the bytes.

A stream is made in two steps.  `*_tokens` turns a scan into a list of tokens -- ("H", slot, symbol) a Huffman-coded
symbol of the scan's table `slot`, ("B", value, nbits) raw bits, ("R", n) restart marker n -- and `_emit` turns tokens
into bytes once the scan's tables are known.  Tables are (symbol, length) lists with canonical code assignment, given
explicitly or made from the scan's own symbol counts by a policy (`flat`, `skewed`, `long_codes`).
"""
import collections
import struct

import numpy as np


def _zigzag():
    zz, k = [0] * 64, 0
    for s in range(15):
        for a in range(8):
            r, c = (a, s - a) if s & 1 else (s - a, a)
            if 0 <= r < 8 and 0 <= c < 8:
                zz[k] = r * 8 + c
                k += 1
    return zz


ZIGZAG = _zigzag()        # zigzag index -> natural position (row * 8 + column), T.81 figure A.6


# ------------------------------------------------------------------------------------------------ Huffman tables
def flat(counts):
    """Every symbol the scan uses gets the same length."""
    syms = sorted(counts)
    n = max(1, (len(syms)).bit_length())          # 2^n > len(syms): Kraft sum < 1
    return [(s, n) for s in syms]


def skewed(counts):
    """Most frequent symbol first: lengths 1, 2, 3, 4, 6, 7, ..., 16, every further symbol 14 bits.  Kraft sum:
    15/16 + (2^-5 - 2^-9) + (2^-9 - 2^-16) + rest * 2^-14 < 1 for rest < 512."""
    syms = sorted(counts, key=lambda s: (-counts[s], s))
    prof = [1, 2, 3, 4] + list(range(6, 17))
    return [(s, prof[i] if i < len(prof) else 14) for i, s in enumerate(syms)]


def long_codes(counts):
    """Only lengths 10..16, in turn by frequency: every symbol is decoded past the 9-bit lookahead."""
    syms = sorted(counts, key=lambda s: (-counts[s], s))
    return [(s, 10 + i % 7) for i, s in enumerate(syms)]


class HuffTable:
    """(symbol, length) pairs -> canonical codes (T.81 annex C).  Symbols of equal length keep the order given."""

    def __init__(self, pairs):
        pairs = list(pairs)
        assert pairs and len({s for s, _ in pairs}) == len(pairs), "duplicate symbol"
        assert all(0 <= s <= 255 and 1 <= l <= 16 for s, l in pairs)
        kraft = sum(1 << (16 - l) for _, l in pairs)
        assert kraft < 1 << 16, "Kraft sum must stay below 1: a complete code has an all-ones code word"
        self.bits = [0] * 17
        self.vals = []
        self.code = {}
        code = 0
        for l in range(1, 17):
            for s, sl in pairs:
                if sl == l:
                    self.code[s] = (code, l)
                    assert code != (1 << l) - 1
                    self.vals.append(s)
                    self.bits[l] += 1
                    code += 1
            code <<= 1

    def dht_payload(self, tc, th):
        assert tc in (0, 1) and 0 <= th <= 3
        return bytes([(tc << 4) | th]) + bytes(self.bits[1:]) + bytes(self.vals)


def _make_table(spec, counts):
    if isinstance(spec, HuffTable):
        t = spec
    elif callable(spec):
        t = HuffTable(spec(counts if counts else {0: 1}))
    else:
        t = HuffTable(spec)
    missing = [s for s in counts if s not in t.code]
    assert not missing, "table lacks symbols the scan emits: %r" % missing
    return t


# ------------------------------------------------------------------------------------------------ frame description
class Component:
    def __init__(self, cid, h, v, tq, coef):
        self.cid, self.h, self.v, self.tq = cid, h, v, tq
        self.coef = np.asarray(coef, np.int64)
        assert self.coef.ndim == 3 and self.coef.shape[2] == 64


class Frame:
    """W x H samples, components in SOF order, qtabs = {id: (64 values in zigzag order, sixteen_bit)}."""

    def __init__(self, W, H, comps, qtabs, precision=8):
        self.W, self.H, self.comps, self.qtabs, self.precision = W, H, list(comps), dict(qtabs), precision
        self.hmax = max(c.h for c in comps)
        self.vmax = max(c.v for c in comps)
        self.mcux = -(-W // (8 * self.hmax))
        self.mcuy = -(-H // (8 * self.vmax))
        for c in self.comps:
            # a frame with one component is never interleaved: its MCU is one block whatever h and v say
            ch, cv = (1, 1) if len(self.comps) == 1 else (c.h, c.v)
            hm, vm = (1, 1) if len(self.comps) == 1 else (self.hmax, self.vmax)
            c.dw = -(-W * ch // hm)
            c.dh = -(-H * cv // vm)
            c.uw, c.uh = -(-c.dw // 8), -(-c.dh // 8)            # blocks a single-component scan walks
            c.eh, c.ev = ch, cv
            want = (self.mcuy * cv, self.mcux * ch, 64) if len(self.comps) > 1 else (-(-H // 8), -(-W // 8), 64)
            assert c.coef.shape == want, (c.coef.shape, want)

    def walk(self, ci_list):
        """Yields restart units of a scan over the components `ci_list` (indices into comps): lists of
        (scan slot, component, block row, block column).  One component: its own ceil(dw/8) x ceil(dh/8) blocks in
        raster order; several: MCUs."""
        if len(ci_list) == 1:
            c = self.comps[ci_list[0]]
            for y in range(c.uh):
                for x in range(c.uw):
                    yield [(0, c, y, x)]
            return
        for my in range(self.mcuy):
            for mx in range(self.mcux):
                unit = []
                for slot, ci in enumerate(ci_list):
                    c = self.comps[ci]
                    for v in range(c.ev):
                        for h in range(c.eh):
                            unit.append((slot, c, my * c.ev + v, mx * c.eh + h))
                yield unit


class Stats:
    def __init__(self):
        self.code_lengths = collections.Counter()     # length -> Huffman code words emitted with it
        self.eobrun_categories = set()                # r of every EOBn symbol emitted
        self.max_eobrun = 0
        self.zrl_first = 0                            # ZRL symbols in AC first scans (and sequential scans)
        self.zrl_refine = 0
        self.restart_inside_eobrun = False            # a restart interval ended while an EOB run was pending
        self.max_restarts_in_scan = 0                 # > 8: the RSTn index wrapped
        self.max_carried_bits = 0                     # correction bits buffered behind one EOBn symbol
        self.eobrun_carrying = set()                  # r of the EOBn symbols that had correction bits behind them
        self.refine_eobrun_before_history = set()     # r of the EOBn symbols of refinement scans whose run ends at a block
                                                      # that has both coefficients with history and a newly non-zero one
        self.max_dc_category = 0
        self.max_ac_size = 0
        self.scans = 0
        self.dht_tables_max = 0                       # tables in the largest DHT segment

    def merge_lengths(self, c):
        self.code_lengths.update(c)


# ------------------------------------------------------------------------------------------------ tokens
def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, n):
    """T.81 F.1.2.1: the low n bits of v, or of v - 1 if v is negative."""
    v = int(v)
    return (v if v >= 0 else v - 1) & ((1 << n) - 1)


class _Restarts:
    """Counts restart units; `due` says whether a restart marker goes in front of the next unit."""

    def __init__(self, interval):
        self.interval, self.left, self.n = interval, interval, 0

    def due(self):
        if not self.interval:
            return False
        if self.left == 0:
            self.left = self.interval
            return True
        return False

    def done_unit(self):
        if self.interval:
            self.left -= 1


def sequential_tokens(frame, ci_list, restart, stats):
    """One scan of a sequential (SOF0 / SOF1) file.  Table slots: 2 * i for the DC, 2 * i + 1 for the AC table of the
    scan's i-th component."""
    out, pred, rs = [], [0] * len(ci_list), _Restarts(restart)
    for unit in frame.walk(ci_list):
        if rs.due():
            out.append(("R", rs.n & 7))
            rs.n += 1
            pred = [0] * len(ci_list)
        for slot, c, by, bx in unit:
            blk = c.coef[by, bx]
            d = int(blk[0]) - pred[slot]
            pred[slot] = int(blk[0])
            n = _category(d)
            assert n <= 11
            stats.max_dc_category = max(stats.max_dc_category, n)
            out.append(("H", 2 * slot, n))
            if n:
                out.append(("B", _value_bits(d, n), n))
            r = 0
            nz = np.flatnonzero(blk[1:]) + 1
            last = 0
            for k in nz:
                r = int(k) - last - 1
                last = int(k)
                while r > 15:
                    out.append(("H", 2 * slot + 1, 0xF0))
                    stats.zrl_first += 1
                    r -= 16
                n = _category(blk[k])
                assert n <= 10
                stats.max_ac_size = max(stats.max_ac_size, n)
                out.append(("H", 2 * slot + 1, (r << 4) | n))
                out.append(("B", _value_bits(blk[k], n), n))
            if last < 63:
                out.append(("H", 2 * slot + 1, 0x00))
        rs.done_unit()
    stats.max_restarts_in_scan = max(stats.max_restarts_in_scan, rs.n)
    return out


def progressive_tokens(frame, ci_list, Ss, Se, Ah, Al, restart, stats):
    """One scan of a progressive file (T.81 annex G).  Table slots: DC first scan: i for the scan's i-th component;
    AC scans: 0; DC refinement scans use no table."""
    out, rs = [], _Restarts(restart)
    if Ss == 0:
        assert Se == 0
        pred = [0] * len(ci_list)
        for unit in frame.walk(ci_list):
            if rs.due():
                out.append(("R", rs.n & 7))
                rs.n += 1
                pred = [0] * len(ci_list)
            for slot, c, by, bx in unit:
                v = int(c.coef[by, bx, 0]) >> Al               # point transform of DC: arithmetic shift
                if Ah:
                    out.append(("B", v & 1, 1))
                    continue
                d = v - pred[slot]
                pred[slot] = v
                n = _category(d)
                stats.max_dc_category = max(stats.max_dc_category, n)
                out.append(("H", slot, n))
                if n:
                    out.append(("B", _value_bits(d, n), n))
            rs.done_unit()
        stats.max_restarts_in_scan = max(stats.max_restarts_in_scan, rs.n)
        return out

    assert len(ci_list) == 1 and 1 <= Ss <= Se <= 63
    c = frame.comps[ci_list[0]]
    band = np.abs(c.coef[:c.uh, :c.uw, Ss:Se + 1]) >> Al            # point transform of AC: magnitude shift
    neg = c.coef[:c.uh, :c.uw, Ss:Se + 1] < 0
    busy = band.reshape(c.uh, c.uw, -1).any(axis=2)                 # False: the block adds one to the EOB run, no more
    eobrun, carried = 0, []                                         # carried: correction bits behind the pending EOBn
    last_eob = None                                                 # r of the EOBn symbol if it is the latest symbol out

    def flush_eobrun():
        nonlocal eobrun, carried, last_eob
        if eobrun:
            n = eobrun.bit_length() - 1
            last_eob = n
            stats.eobrun_categories.add(n)
            if carried:
                stats.eobrun_carrying.add(n)
            stats.max_eobrun = max(stats.max_eobrun, eobrun)
            out.append(("H", 0, n << 4))
            if n:
                out.append(("B", eobrun & ((1 << n) - 1), n))
            eobrun = 0
        stats.max_carried_bits = max(stats.max_carried_bits, len(carried))
        out.extend(("B", b, 1) for b in carried)
        carried = []

    for by in range(c.uh):
        for bx in range(c.uw):
            if rs.due():
                if eobrun:
                    stats.restart_inside_eobrun = True
                flush_eobrun()
                out.append(("R", rs.n & 7))
                rs.n += 1
                last_eob = None
            rs.done_unit()
            if not busy[by, bx]:
                eobrun += 1
                if eobrun == 0x7FFF:
                    flush_eobrun()
                continue
            t, ng = band[by, bx], neg[by, bx]
            n = Se - Ss + 1
            if Ah == 0:
                r = 0
                for k in range(n):
                    a = int(t[k])
                    if a == 0:
                        r += 1
                        continue
                    flush_eobrun()
                    while r > 15:
                        out.append(("H", 0, 0xF0))
                        stats.zrl_first += 1
                        r -= 16
                    nb = a.bit_length()
                    assert nb <= 10
                    stats.max_ac_size = max(stats.max_ac_size, nb)
                    out.append(("H", 0, (r << 4) | nb))
                    out.append(("B", _value_bits(-a if ng[k] else a, nb), nb))
                    r = 0
                if r:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        flush_eobrun()
                continue
            # refinement (G.1.2.3): coefficients already non-zero send one correction bit each, buffered until the next
            # symbol is out; newly non-zero ones (magnitude exactly 1 at this Al) send run/size with size 1 and a sign
            ones = np.flatnonzero(t == 1)
            last_new = int(ones[-1]) if len(ones) else -1
            r, br = 0, []
            if last_new < 0 or not (t > 1).any():
                last_eob = None                                     # only a block with history and a new coefficient counts
            for k in range(n):
                a = int(t[k])
                if a == 0:
                    r += 1
                    continue
                while r > 15 and k <= last_new:
                    flush_eobrun()
                    if last_eob is not None:
                        stats.refine_eobrun_before_history.add(last_eob)
                        last_eob = None
                    out.append(("H", 0, 0xF0))
                    stats.zrl_refine += 1
                    r -= 16
                    out.extend(("B", b, 1) for b in br)
                    br = []
                if a > 1:
                    br.append(a & 1)
                    continue
                flush_eobrun()
                if last_eob is not None:
                    stats.refine_eobrun_before_history.add(last_eob)
                    last_eob = None
                out.append(("H", 0, (r << 4) | 1))
                out.append(("B", 0 if ng[k] else 1, 1))
                out.extend(("B", b, 1) for b in br)
                br = []
                r = 0
            if r or br:
                eobrun += 1
                carried.extend(br)
                if eobrun == 0x7FFF:
                    flush_eobrun()
    flush_eobrun()
    stats.max_restarts_in_scan = max(stats.max_restarts_in_scan, rs.n)
    return out


def _symbol_counts(tokens):
    counts = collections.defaultdict(collections.Counter)
    for t in tokens:
        if t[0] == "H":
            counts[t[1]][t[2]] += 1
    return counts


def _emit(tokens, tables, stats, fill=0):
    """Tokens -> entropy-coded bytes: byte stuffing, 1-padding before every marker and at the end, `fill` extra FF bytes
    in front of each RSTn."""
    out = bytearray()
    acc = nacc = 0

    def put(v, n):
        nonlocal acc, nacc
        acc = (acc << n) | v
        nacc += n
        while nacc >= 8:
            b = (acc >> (nacc - 8)) & 0xFF
            out.append(b)
            if b == 0xFF:
                out.append(0)
            nacc -= 8
        acc &= (1 << nacc) - 1

    def pad():
        if nacc:
            put((1 << (8 - nacc)) - 1, 8 - nacc)

    lengths = collections.Counter()
    for t in tokens:
        if t[0] == "H":
            code, l = tables[t[1]].code[t[2]]
            lengths[l] += 1
            put(code, l)
        elif t[0] == "B":
            put(t[1], t[2])
        else:
            pad()
            out += b"\xff" * fill + bytes([0xFF, 0xD0 + t[1]])
    pad()
    stats.merge_lengths(lengths)
    return bytes(out)


# ------------------------------------------------------------------------------------------------ segments
def segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def dqt_payload(tq, values, sixteen=False):
    v = [int(x) for x in values]
    assert len(v) == 64 and all(1 <= x <= (65535 if sixteen else 255) for x in v)
    return bytes([(16 if sixteen else 0) | tq]) + (struct.pack(">64H", *v) if sixteen else bytes(v))


def dqt_segment(tabs, merged=True):
    """tabs = {id: (zigzag values, sixteen_bit)}: one DQT segment holding them all, or one each."""
    parts = [dqt_payload(tq, v, s) for tq, (v, s) in sorted(tabs.items())]
    return segment(0xDB, b"".join(parts)) if merged else b"".join(segment(0xDB, p) for p in parts)


def _dht(parts, merged, stats):
    if not parts:
        return b""
    stats.dht_tables_max = max(stats.dht_tables_max, len(parts) if merged else 1)
    return segment(0xC4, b"".join(parts)) if merged else b"".join(segment(0xC4, p) for p in parts)


def _head(frame, sof, jfif, merged_dqt):
    out = b"\xff\xd8"
    if jfif:
        out += segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += dqt_segment(frame.qtabs, merged_dqt)
    body = struct.pack(">BHHB", frame.precision, frame.H, frame.W, len(frame.comps))
    for c in frame.comps:
        body += bytes([c.cid, (c.h << 4) | c.v, c.tq])
    return out + segment(sof, body)


def _sos(frame, ci_list, tsel, Ss, Se, Ah, Al):
    body = bytes([len(ci_list)])
    for ci, (td, ta) in zip(ci_list, tsel):
        body += bytes([frame.comps[ci].cid, (td << 4) | ta])
    return segment(0xDA, body + bytes([Ss, Se, (Ah << 4) | Al]))


def _tail(fill, trailing):
    return b"\xff" * fill + b"\xff\xd9" + bytes(trailing)


# ------------------------------------------------------------------------------------------------ files
def write_sequential(frame, sof=0xC0, scans=None, table_ids=None, tables=flat, merged_dht=True, merged_dqt=True,
                     restart=0, fill=0, trailing=b"", jfif=True, sos_order=None):
    """A baseline (sof = 0xC0) or extended-sequential (0xC1) file.  scans: component index lists (default: one
    interleaved scan of all).  table_ids[ci] = (DC id, AC id) (default: 0, 0 for the first component, 1, 1 for the others).
    tables: a policy, or {(class, id): policy or (symbol, length) list}; components that share an id share the table.
    sos_order: permutation applied to the components of an interleaved scan (the MCU follows it).  Returns (bytes, Stats)."""
    assert sof in (0xC0, 0xC1)
    stats = Stats()
    n = len(frame.comps)
    scans = [list(range(n))] if scans is None else scans
    table_ids = table_ids or [(0, 0)] + [(1, 1)] * (n - 1)
    out = _head(frame, sof, jfif, merged_dqt)
    current_restart = 0
    for ci_list in scans:
        if sos_order is not None and len(ci_list) > 1:
            ci_list = [ci_list[i] for i in sos_order]
        toks = sequential_tokens(frame, ci_list, restart, stats)
        counts = _symbol_counts(toks)
        by_id = collections.defaultdict(collections.Counter)         # (class, id) -> symbols of every slot that uses it
        for slot, ci in enumerate(ci_list):
            by_id[(0, table_ids[ci][0])].update(counts[2 * slot])
            by_id[(1, table_ids[ci][1])].update(counts[2 * slot + 1])
        built = {key: _make_table(tables[key] if isinstance(tables, dict) else tables, cnt) for key, cnt in sorted(by_id.items())}
        out += _dht([t.dht_payload(tc, th) for (tc, th), t in sorted(built.items())], merged_dht, stats)
        if restart != current_restart:
            out += segment(0xDD, struct.pack(">H", restart))
            current_restart = restart
        slot_tabs = {}
        for slot, ci in enumerate(ci_list):
            slot_tabs[2 * slot] = built[(0, table_ids[ci][0])]
            slot_tabs[2 * slot + 1] = built[(1, table_ids[ci][1])]
        out += _sos(frame, ci_list, [table_ids[ci] for ci in ci_list], 0, 63, 0, 0)
        out += _emit(toks, slot_tabs, stats, fill)
        stats.scans += 1
    return out + _tail(fill, trailing), stats


def write_progressive(frame, script, tables=flat, dri=None, between=None, dc_ids=None, ac_id=0, merged_dht=True,
                      merged_dqt=True, fill=0, trailing=b"", jfif=True):
    """A progressive (SOF2) file.  script: (component indices, Ss, Se, Ah, Al) per scan, written as given -- the script's
    validity is the caller's business.  tables: a policy for every scan, or a list with one entry per scan (a policy, or
    {slot: policy or (symbol, length) list}).  dri: restart interval per scan (0 = off; a DRI segment is written whenever
    the interval changes).  between: {scan index: raw bytes written in front of that scan's tables} (COM, APPn, DQT ...).
    dc_ids[ci]: the DC table id of a component (default: its index); ac_id: int, or list per scan.  Returns (bytes, Stats)."""
    stats = Stats()
    n = len(frame.comps)
    dc_ids = dc_ids or list(range(n))
    out = _head(frame, 0xC2, jfif, merged_dqt)
    current_restart = 0
    for si, (ci_list, Ss, Se, Ah, Al) in enumerate(script):
        ci_list = list(ci_list)
        restart = dri[si % len(dri)] if dri else 0
        toks = progressive_tokens(frame, ci_list, Ss, Se, Ah, Al, restart, stats)
        counts = _symbol_counts(toks)
        pol = tables[si] if isinstance(tables, list) else tables
        aid = ac_id[si] if isinstance(ac_id, list) else ac_id
        if between and si in between:
            out += between[si]
        slot_tabs, parts, tsel = {}, [], [(0, 0)] * len(ci_list)
        if Ss == 0 and Ah == 0:
            by_id = collections.defaultdict(collections.Counter)
            for slot, ci in enumerate(ci_list):
                by_id[dc_ids[ci]].update(counts[slot])
            spec = {}
            for slot, ci in enumerate(ci_list):
                spec.setdefault(dc_ids[ci], pol[slot] if isinstance(pol, dict) else pol)
            built = {th: _make_table(spec[th], cnt) for th, cnt in by_id.items()}
            parts = [built[th].dht_payload(0, th) for th in sorted(built)]
            slot_tabs = {slot: built[dc_ids[ci]] for slot, ci in enumerate(ci_list)}
            tsel = [(dc_ids[ci], 0) for ci in ci_list]
        elif Ss > 0:
            t = _make_table(pol[0] if isinstance(pol, dict) else pol, counts[0])
            parts = [t.dht_payload(1, aid)]
            slot_tabs = {0: t}
            tsel = [(0, aid)]
        out += _dht(parts, merged_dht, stats)
        if restart != current_restart:
            out += segment(0xDD, struct.pack(">H", restart))
            current_restart = restart
        out += _sos(frame, ci_list, tsel, Ss, Se, Ah, Al)
        out += _emit(toks, slot_tabs, stats, fill)
        stats.scans += 1
    return out + _tail(fill, trailing), stats


# ------------------------------------------------------------------------------------------------ the over-range files
def overrange_frames():
    """[(name, Frame)]: 12 gray 8 x 32 files, q = 1, DC = +-1000, the first 1, 3 or 6 AC coefficients at +-m.  Their inverse
    DCT leaves the sample range by hundreds: shared by tests/test_jpeg_crafted.py and tools/make_golden_jpeg_crafted.py."""
    out = []
    for m in (300, 600, 900, 1023):
        for n in (1, 3, 6):
            coef = np.zeros((1, 4, 64), np.int64)
            for b, (sd, sa) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
                coef[0, b, 0] = sd * 1000
                coef[0, b, 1:1 + n] = sa * m
            out.append(("over_%dx%d" % (m, n), Frame(32, 8, [Component(1, 1, 1, 0, coef)], {0: ([1] * 64, False)})))
    return out


def overrange_blobs():
    return [(name, write_sequential(f)[0]) for name, f in overrange_frames()]
