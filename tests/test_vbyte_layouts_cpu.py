"""The layout families of tests/vbyte_layouts.py, held to their own claims
without a device: every class in R units or more per case and UNREACHED exactly
as stated, with the directed draws that missed; the restated parses agree with
the serial definition on every unit and every wrong variant (MUTANTS) parses 3
units or more of each full-width 32-bit family differently; the older inputs
(vbyte_case, v32_case, wide_vbyte_gaps, the lists tail families) miss the classes
and let through the variants recorded here; the host framing
(tpf_block_size, tpf_scan_offsets, tpf_lists_scan_offsets) sizes every unit,
decode-only ones included, as the oracle does; and the oracle's bytes and
decodes are the reference's where oracle/_ref is built."""
import ctypes
import os

import numpy as np
import pytest

import h64_inputs
import lists_ref
import lists_tails
import oracle_lib as orc
import ref_lib
import v32_inputs
import vbyte_layouts as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
FMT = {"32": 0, "128v32": 1, "256v32": 2, "64": 3, "128v64": 4, "256v64": 5}
CASES32 = [c for c in vl.CASES if vl.WBITS[c[0]] == 32]


# ---- the census ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n", vl.CASES)
def test_census(fmt, n):
    """every class of the case in R units or more, by the bytes of the plain and of the delta-1 stream; the classes
    of UNREACHED in none, and in none of their directed draws"""
    f, c, cd = vl.family(fmt, n), vl.layout_case(fmt, n, False), vl.layout_case(fmt, n, True)
    assert f.nu <= vl.MAX_UNITS
    assert np.array_equal(c.packed, cd.packed) and np.array_equal(c.off, cd.off)  # the same gaps: the same units
    cen = vl.stream_census(fmt, n, c.packed, c.off)
    assert all(vl.unit_facts(fmt, c.packed, int(c.off[i]), n) == f.tags[i] for i in range(f.nu))
    low = {t: cen[t] for t in vl.required_classes(fmt, n) if cen[t] < vl.R}
    assert not low, low
    assert sorted(vl.UNREACHED[(fmt, n)], key=str) == sorted((t for t in vl.all_classes(fmt, n) if cen[t] == 0), key=str)
    for t, (draws, units) in vl.directed_misses(fmt, n).items():
        assert draws >= vl.tries(t) + (1000 if t[0] in ("W", "short", "xn") else 0) and units == 0, (t, draws, units)
    print(fmt, n, f.nu, "units;", len(vl.required_classes(fmt, n)), "classes; most windows", max(t[1] for t in cen if t[0] == "W" and cen[t]))


def test_the_chained_form_wraps():
    for fmt, n in vl.CASES:
        c = vl.layout_case(fmt, n, True)
        flat = c.vals.ravel().astype(object)
        assert (np.diff(flat) < 0).any() and int(c.starts[0]) == c.start0, (fmt, n)


@pytest.mark.parametrize("fmt,n", vl.DECODE_ONLY_CASES)
def test_decode_only_family(fmt, n):
    """xn in {128, 200, 255}, all-2, all-3, all-4 and mixed lengths, up to 16 windows, V canonical, positions distinct and
    ascending; nothing the encoder writes: re-encoding the values gives other bytes"""
    d = vl.decode_only(fmt, n)
    assert {(x, k) for x, k, _ in d.label} == {(x, k) for x in vl.DO_XN for k in vl.DO_KINDS}
    assert max(w for _, _, w in d.label) == 16 and min(w for _, _, w in d.label) <= 4
    for i in range(d.nu):
        blk = vl.blocks_of_unit(fmt, d.packed, int(d.off[i]), n)[0]
        assert blk.mode == "vb_comp" and blk.end == int(d.off[i + 1]) and blk.xn == d.label[i][0]
        pos = d.packed[blk.v0 + blk.vlen: blk.end]
        assert len(pos) == blk.xn and (np.diff(pos.astype(int)) > 0).all() and int(pos[-1]) < n
        vals, _ = vl.serial_parse(bytes(d.packed[blk.v0: blk.end]), blk.xn)
        assert np.array_equal(np.concatenate([vl._vbput32(v) for v in vals]), d.packed[blk.v0: blk.v0 + blk.vlen])
        assert orc.encode(fmt, d.gaps[i]) != bytes(d.packed[int(d.off[i]): int(d.off[i + 1])])
    if fmt == "256v32":
        assert sum(("v1024",) in t for t in d.tags) >= vl.R  # the class no encoded unit reaches


# ---- the restated parses and their wrong variants ----------------------------------------------
def _streams32():
    out = [(fmt, n, vl.layout_case(fmt, n, False)) for fmt, n in CASES32]
    return out + [(fmt, n, vl.decode_only(fmt, n)) for fmt, n in vl.DECODE_ONLY_CASES]


def test_restated_parses_agree_with_the_definition():
    """windowed_parse and short_form_sum against vbDec32's serial walk, on every compressed block of every 32-bit
    family; the short form is taken exactly when V has at most 64 bytes and only 1- and 2-byte values"""
    fast = blocks = 0
    for fmt, n, c in _streams32():
        for i in range(c.nu):
            blk = vl.blocks_of_unit(fmt, c.packed, int(c.off[i]), n)[0]
            if blk.mode != "vb_comp":
                continue
            V = bytes(c.packed[blk.v0: blk.end])
            want = vl.serial_parse(V, blk.xn)
            assert want[1] == blk.vlen and vl.windowed_parse(V, blk.xn) == want, (fmt, n, i)
            for v0 in (0, 1, 2, 3):
                path, s = vl.short_form_sum(V[:blk.vlen], blk.xn, v0)
                assert s == sum(want[0]) & 0xFFFFFFFF, (fmt, n, i)
                assert (path == "fast") == (blk.vlen <= 64 and max(blk.lens) <= 2), (fmt, n, i, path)
            fast += path == "fast"
            blocks += 1
    print(blocks, "compressed blocks,", fast, "in the short form")
    assert fast >= 100


def test_wrong_variants_on_their_own_cases():
    """each wrong variant on the smallest stream that separates it from the right parse, and on one that does not"""
    one = bytes([100] * 63)                     # 63 one-byte values
    two = bytes([0x9D, 0x10])                   # a 2-byte value
    five = bytes([0xFD, 1, 2, 3, 4])
    s = one + two + bytes([7] * 10)             # the 2-byte value ends 1 byte past byte 64
    for rule in ("straddle_dropped", "straddle_off_by_one"):
        assert vl.windowed_parse(s, 74, rule) != vl.windowed_parse(s, 74)
        assert vl.windowed_parse(one + bytes([5]), 64, rule)[0] == [100] * 63 + [5]  # one window: nothing carried
    three = bytes([100] * 129)
    assert vl.windowed_parse(three, 129, "two_windows") != vl.windowed_parse(three, 129)
    assert vl.windowed_parse(three[:128], 128, "two_windows") == vl.windowed_parse(three[:128], 128)
    for rule, k in (("ring_64", 64), ("ring_128", 128)):
        v = bytes(range(1, 131)) + five
        assert vl.windowed_parse(v, k + 1, rule) != vl.windowed_parse(v, k + 1)
        assert vl.windowed_parse(v, k, rule) == vl.windowed_parse(v, k)
    assert vl.short_form_sum(one + bytes([1]), 64, 0, "lt_64")[0] == "walk" and vl.short_form_sum(one + bytes([1]), 64)[0] == "fast"
    assert vl.short_form_sum(one, 63, 0, "lt_64") == vl.short_form_sum(one, 63)
    odd = bytes([0x9D, 0x10, 0x20])             # a run of 1: its marker, its data byte, a one-byte value
    assert vl.short_form_sum(odd, 2, 0, "after_run_marker") != vl.short_form_sum(odd, 2) == ("fast", 156 + 256 + 0x10 + 0x20)
    even = bytes([0x9D, 0x9E, 0x20])            # a run of 2 that ends in a data byte: the next byte IS a marker
    assert vl.short_form_sum(even, 2, 0, "after_run_marker") == vl.short_form_sum(even, 2)
    cross = bytes([1, 1, 0x9D, 0xA0, 0xA1, 0xA2, 1, 1])  # a run from byte 2 over the dword boundary at byte 4
    right = vl.short_form_sum(cross, 6)
    assert right == ("fast", 4 + (156 + 256 + 0xA0) + (156 + 5 * 256 + 0xA2))
    assert vl.short_form_sum(cross, 6, 0, "carry_dropped") != right
    inside = bytes([0x9D, 0xA0, 0xA1, 0xA2, 1, 1, 1, 1])  # the same run inside one dword
    assert vl.short_form_sum(inside, 6, 0, "carry_dropped") == vl.short_form_sum(inside, 6)
    assert vl.short_form_sum(cross, 6, 1, "parity_in_dword") != right and vl.short_form_sum(cross, 6, 2, "parity_in_dword") == right
    raw = np.array([0x40, 2, 0xFF] + [9] * 8 + [3, 4], dtype=np.uint8)  # b = 0, two raw exceptions
    assert vl.unit_size32(raw, 0, 64, None) == len(raw) == vl.unit_size32(raw, 0, 64, None, "raw_5xn") + 1


@pytest.mark.parametrize("fmt,n", vl.FULL_WIDTH32)
def test_every_wrong_variant_misparses_the_family(fmt, n):
    c = vl.layout_case(fmt, n, False)
    for rule in vl.MUTANTS:
        bad = set()
        for shift in ((0, 1) if rule == "parity_in_dword" else (0,)):
            bad |= set(vl.misparsed(fmt, n, c.packed, c.off, rule, shift))
        print(fmt, n, rule, len(bad), "units")
        assert len(bad) >= 3, (fmt, n, rule, sorted(bad))
    assert vl.survivors(fmt, n, c.packed, c.off) == []


# ---- what the older inputs reach -------------------------------------------------------------
# Per older input, vbyte_layouts.layout_record of its stream -- compressed vbyte blocks, their windows of V, the units
# in which a value ends 1 / 2 / 3 / 4 bytes past a window boundary, the most exceptions, how many of the case's classes
# (62 at 255 / 256 values, 55 at 127 / 128, 43 at 64; 70 and 62 for the 64-bit cases) it holds in fewer than R units
# and in none -- and the wrong variants that parse every one of its units right.
def _all_but(*killed):
    return [r for r in vl.MUTANTS if r not in killed]


_SMALL = _all_but("after_run_marker", "parity_in_dword")  # what gets through at 127 / 128 values: V never leaves its first window
OLDER = {
    ("vbyte_case", "256v32", 256): ((367, {1: 210, 2: 157}, [5, 3, 1, 1], 85, 48, 33), ["two_windows", "ring_128", "lt_64", "carry_dropped", "raw_5xn"]),
    ("v32_case", "256v32", 256): ((140, {1: 82, 2: 58}, [2, 1, 1, 1], 85, 49, 35), ["two_windows", "ring_128", "lt_64"]),
    ("vbyte_case", "32", 255): ((355, {1: 190, 2: 165}, [6, 2, 4, 1], 85, 46, 37), ["two_windows", "ring_128", "carry_dropped", "raw_5xn"]),
    ("vbyte_case", "128v32", 128): ((365, {1: 365}, [0, 0, 0, 0], 42, 45, 45), _SMALL),
    ("vbyte_case", "32", 127): ((349, {1: 349}, [0, 0, 0, 0], 42, 45, 44), _SMALL),
}
OLDER_WIDE = {
    ("64", 256): (192, {1: 89, 2: 103}, [1, 2, 2, 3], 84, 63, 47),
    ("128v64", 128): (195, {1: 195}, [0, 0, 0, 0], 42, 59, 58),
    ("256v64", 256): (387, {1: 387}, [0, 0, 0, 0], 42, 58, 58),
}
# the tail units of the lists tail families at the three tail sizes used here: three compressed vbyte units each
OLDER_TAILS = {
    ("wide", 255): ((3, {1: 1, 2: 2}, [0, 0, 0, 0], 79, 61, 55), _all_but("straddle_off_by_one", "ring_64", "raw_5xn")),
    ("wide", 127): ((3, {1: 3}, [0, 0, 0, 0], 24, 53, 52), _all_but("raw_5xn")),
    ("wide", 64): ((3, {1: 3}, [0, 0, 0, 0], 21, 41, 39), _all_but("raw_5xn")),
    ("ascending", 255): ((3, {1: 2, 2: 1}, [0, 0, 0, 0], 83, 61, 51), ["straddle_dropped", "two_windows", "ring_128", "lt_64"]),
    ("ascending", 127): ((3, {1: 3}, [0, 0, 0, 0], 29, 53, 49), _all_but("after_run_marker", "parity_in_dword", "raw_5xn")),
    ("ascending", 64): ((3, {1: 3}, [0, 0, 0, 0], 17, 40, 40), _all_but("raw_5xn")),
}


@pytest.mark.parametrize("maker,fmt,n", list(OLDER))
def test_older_inputs_fall_short(maker, fmt, n):
    """the inputs the suite had for compressed vbyte: no third window, no block past 85 exceptions (42 at 127 / 128
    values, where V never leaves its first window), a handful of straddles by luck of the seed, no run of 6 bytes or
    more -- most classes in fewer than R units -- and these wrong variants get through"""
    c = getattr(v32_inputs, maker)(fmt, n, False)
    record, through = OLDER[(maker, fmt, n)]
    assert vl.layout_record(fmt, n, c.packed, c.off) == record
    cen = vl.stream_census(fmt, n, c.packed, c.off)
    assert not any(cen[t] for t in cen if t[0] == "run" and t[1] in (6, 7, 8, "9-15", "16+"))
    assert not any(cen[t] for t in cen if t[0] == "xn" and t[1] >= 127)
    assert vl.survivors(fmt, n, c.packed, c.off) == through


@pytest.mark.parametrize("fmt,n", list(OLDER_WIDE))
def test_older_wide_inputs_fall_short(fmt, n):
    packed, off = vl.oracle_stream(fmt, h64_inputs.wide_vbyte_gaps(fmt, n, 200))
    assert vl.layout_record(fmt, n, packed, off) == OLDER_WIDE[(fmt, n)]


@pytest.mark.parametrize("name,cnt", list(OLDER_TAILS))
def test_older_lists_tails_fall_short(name, cnt):
    """the tails of tests/lists_tails.py hold every MODE at every count, in three units each: of the layout classes at
    255, 127 and 64 values they hold next to none"""
    fam = lists_tails.family(name)
    p = fam.plain()
    parts = [p.packed[int(p.offs[u]): int(p.offs[u + 1])] for j, u in fam.tail_unit(p.base) if fam.cnt[j] == cnt]
    packed, off = np.concatenate(parts), np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    record, through = OLDER_TAILS[(name, cnt)]
    assert vl.layout_record("32", cnt, packed, off) == record
    assert vl.survivors("32", cnt, packed, off) == through


# ---- the host framing ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    L = ctypes.CDLL(LIB)
    L.tpf_block_size.restype = ctypes.c_uint64
    L.tpf_block_size.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint, ctypes.POINTER(ctypes.c_int)]
    L.tpf_scan_offsets.restype = ctypes.c_int64
    L.tpf_scan_offsets.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.tpf_lists_scan_offsets.restype = ctypes.c_int64
    L.tpf_lists_scan_offsets.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint64]
    return L


def _all_streams():
    out = [(fmt, n, vl.layout_case(fmt, n, False)) for fmt, n in vl.CASES]
    return out + [(fmt, n, vl.decode_only(fmt, n)) for fmt, n in vl.DECODE_ONLY_CASES]


def test_block_size_and_scan_offsets(capi):
    for fmt, n, c in _all_streams():
        stream = bytes(c.packed)
        for i in range(c.nu):
            enc = stream[int(c.off[i]): int(c.off[i + 1])]
            assert capi.tpf_block_size(FMT[fmt], enc, len(enc), n, None) == len(enc), (fmt, n, c.names([i]))
            assert capi.tpf_block_size(FMT[fmt], enc, len(enc) - 1, n, None) == 0, (fmt, n, c.names([i]))
        off = (ctypes.c_uint64 * (c.nu + 1))()
        assert capi.tpf_scan_offsets(FMT[fmt], stream, len(stream), n, c.nu, off) == len(stream), (fmt, n)
        assert list(off) == c.off.tolist(), (fmt, n)


@pytest.mark.parametrize("kind", ["reachable", "decode_only"])
def test_lists_scan_offsets(capi, kind):
    """the lists stream of the families: its bytes are the oracle's composition of its lists (reachable units), and the
    host scan finds every unit, with and without the lists' byte anchors"""
    ll = vl.layout_lists(kind)
    assert set(ll.unit_label) == {(n, i) for n in ll.fam for i in range(ll.fam[n].nu)}
    assert sorted(len(lab) for lab in ll.label)[-1] == 71 and {len(g) % 256 for g in ll.gaps} >= set(ll.fam) - {256}
    if kind == "reachable":
        for d1 in (False, True):
            packed, offs, ptr, _ = lists_ref.compose(ll.lists(d1), d1, ll.start0)
            assert np.array_equal(packed, ll.packed) and np.array_equal(offs, ll.offs) and np.array_equal(ptr, ll.ptr)
    for lbyte in (None, ll.list_byte):
        off = np.full(ll.nunits + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        r = capi.tpf_lists_scan_offsets(ll.packed.ctypes.data, len(ll.packed), ll.ptr.ctypes.data, ll.nlists,
                                        None if lbyte is None else np.ascontiguousarray(lbyte).ctypes.data, off.ctypes.data, ll.nunits)
        assert r == len(ll.packed) and np.array_equal(off, ll.offs)


# ---- the oracle against the reference -------------------------------------------------------------
@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref is not built")
def test_oracle_is_the_reference():
    """the reference's scalar encoders write the oracle's bytes for every unit of every family, and its
    decoders return the expected values of the decode-only units, plain and delta-1"""
    L = ref_lib.lib()
    for fmt, n in vl.CASES:
        c = vl.layout_case(fmt, n, False)
        tp, dt = (ref_lib.u32p, np.uint32) if c.W == 32 else (ref_lib.u64p, np.uint64)
        enc_f = getattr(L, "tpref_s_p4enc" + fmt)
        for i in range(c.nu):
            src = np.zeros(256 + 64, dtype=dt)
            src[:n] = c.vals[i]
            want = c.packed[int(c.off[i]): int(c.off[i + 1])]
            out = np.zeros(len(want) + 4096, dtype=np.uint8)
            end = enc_f(src.ctypes.data_as(tp), n, out.ctypes.data_as(ref_lib.u8p))
            assert end - out.ctypes.data == len(want) and np.array_equal(out[:len(want)], want), (fmt, n, c.names([i]))
    for fmt, n in vl.DECODE_ONLY_CASES:
        d = vl.decode_only(fmt, n)
        dec_f, d1dec_f = getattr(L, "tpref_s_p4dec" + fmt), getattr(L, "tpref_s_p4d1dec" + fmt)
        for i in range(d.nu):
            enc = np.concatenate([d.packed[int(d.off[i]): int(d.off[i + 1])], np.zeros(64, np.uint8)])
            out = np.zeros(256 + 64, dtype=np.uint32)
            end = dec_f(enc.ctypes.data_as(ref_lib.u8p), n, out.ctypes.data_as(ref_lib.u32p))
            assert end - enc.ctypes.data == len(enc) - 64 and np.array_equal(out[:n], d.gaps[i]), (fmt, n, d.names([i]))
            end = d1dec_f(enc.ctypes.data_as(ref_lib.u8p), n, out.ctypes.data_as(ref_lib.u32p), int(d.starts[i]))
            assert end - enc.ctypes.data == len(enc) - 64 and np.array_equal(out[:n], d.chained[i]), (fmt, n, d.names([i]))
