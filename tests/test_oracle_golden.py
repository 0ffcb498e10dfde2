"""Pins the CPU restatement (oracle/) against golden vectors generated from
the reference's own src/scalar codec (oracle/gen_golden.cpp)."""
import numpy as np
import pytest

import golden_io
import oracle_lib
import p4_modes
import v64_inputs

FAMILIES = [("g256v32.bin", "256v32"), ("g128v32.bin", "128v32"), ("g32.bin", "32"),
            ("g256v64.bin", "256v64"), ("g128v64.bin", "128v64"), ("g64.bin", "64"),
            ("g256v32s.bin", "256v32"), ("g128v32s.bin", "128v32"), ("g32vb.bin", "32"),
            ("g256v64s.bin", "256v64"), ("g128v64s.bin", "128v64")]
V64_FILES = [("g128v64.bin", "128v64"), ("g256v64.bin", "256v64"), ("g128v64s.bin", "128v64"), ("g256v64s.bin", "256v64")]


def blocks64(fmt, r):
    """The 128v64 blocks of a 128v64 / 256v64 record: [(block's n, Block64)]."""
    out, pos = [], 0
    for bn in v64_inputs.block_ns(fmt, r.n):
        blk = p4_modes.parse64(r.enc, pos, bn, 128)
        out.append((bn, blk))
        pos = blk.end
    assert pos == len(r.enc)
    return out


def pinned_bytes64(fmt, r):
    """A record's bytes with the base payload of every block shorter than 128
    values zeroed: what the reference pins even where its padding bits came
    from its stack -- header, bx / xn, bitmap, patch bits, vbyte stream and
    positions.  Applied to the reference's bytes and to the oracle's."""
    def strip(enc):
        enc = bytearray(enc)
        for bn, blk in blocks64(fmt, r):
            if bn < 128:
                enc[blk.base[0]: blk.base[1]] = bytes(blk.base[1] - blk.base[0])
        return bytes(enc)
    return strip


@pytest.mark.parametrize("fname,fmt", FAMILIES)
def test_oracle_matches_golden(fname, fmt):
    recs = golden_io.load(fname)
    assert len(recs) > 100
    for i, r in enumerate(recs):
        if not r.decode_only:
            enc = oracle_lib.encode(fmt, r.values, d1=r.d1, start=r.start)
            if r.padding_unpinned:
                # padding slots follow the zero convention: same length, same values back
                assert len(enc) == len(r.enc), f"{fname} record {i}: encoded length differs"
                if fmt in ("128v64", "256v64"):
                    # everything outside the short blocks' base payload is the reference's
                    strip = pinned_bytes64(fmt, r)
                    assert strip(enc) == strip(r.enc), f"{fname} record {i}: bytes outside the base payload differ"
                back, used = oracle_lib.decode(fmt, enc, r.n, d1=r.d1, start=r.start)
                assert used == len(enc)
                np.testing.assert_array_equal(back, r.values, err_msg=f"{fname} record {i} (own bytes)")
            else:
                assert enc == r.enc, f"{fname} record {i}: encoder bytes differ"
        dec, used = oracle_lib.decode(fmt, r.enc, r.n, d1=r.d1, start=r.start)
        assert used == len(r.enc), f"{fname} record {i}: end pointer"
        np.testing.assert_array_equal(dec, r.values, err_msg=f"{fname} record {i}")


def test_short_64bit_units_are_pinned():
    """128v64 with n < 128 and 256v64 with n < 256 (the reference takes any
    n): most vectors are byte-pinned; only those whose padding bits depend on
    the reference's uninitialised stack are not."""
    for fname, full in (("g128v64.bin", 128), ("g256v64.bin", 256)):
        short = [r for r in golden_io.load(fname) if r.n < full]
        assert len(short) >= 50
        pinned = [r for r in short if not r.padding_unpinned]
        assert len(pinned) >= len(short) // 2, (fname, len(pinned), len(short))


def _class64(blk):
    """Block64.split with the exception modes over no base (b = 0) apart."""
    return blk.mode + "_0" if blk.mode in ("bitmap", "vb_raw", "vb_comp") and blk.b == 0 else blk.split


UNFLAGGED64 = ("zero", "const", "const63", "plain_v", "plain_h", "plain63", "bitmap_0", "vb_raw_0", "vb_comp_0")


@pytest.mark.parametrize("fname,fmt", V64_FILES)
def test_flag_rule_of_64bit_units(fname, fmt):
    """Where the reference's 128v64 bytes depend on its uninitialised stack
    (flag 4, found by encoding after a 0x00 and after a 0xA5 fill of the
    stack): exactly the records with a block of fewer than 128 values that is
    either in bitmap or vbyte mode with b >= 1 -- base[] is a stack array of
    which p4Enc128v64PayloadExceptions fills n slots and bitpack128v64Scalar
    packs 128 (p4enc128v64_scalar.cpp:59, :113, :130), with or without
    delta-1 -- or a delta-1 block in plain mode, whose n deltas sit in a stack
    array too (p4d1enc128v64_scalar.cpp).  An exception block with b = 0 packs
    no base at all, so it is pinned even with delta-1.  No zero, constant or
    non-delta-1 plain record is flagged.  In the every-mode files at least
    half of the short records without delta-1 are byte-pinned, and so are at
    least two blocks of every class that can be."""
    recs = [r for r in golden_io.load(fname) if not r.decode_only]
    full = v64_inputs.WIDTH[fmt]
    unflagged = dict.fromkeys(UNFLAGGED64, 0)
    for i, r in enumerate(recs):
        want = False
        for bn, blk in blocks64(fmt, r):
            if bn == 128:
                continue
            hit = (blk.mode in ("bitmap", "vb_raw", "vb_comp") and blk.b >= 1) or (r.d1 and blk.mode in ("plain", "plain63"))
            want |= hit
            if not hit and not r.d1:
                unflagged[_class64(blk)] += 1
        assert r.padding_unpinned == want, (fname, i, r.n, r.d1, [b.split for _, b in blocks64(fmt, r)])
    short = [r for r in recs if r.n < full and not r.d1]
    assert len(short) >= 40
    assert 2 * sum(not r.padding_unpinned for r in short) >= len(short), fname
    assert any(r.padding_unpinned for r in recs)  # the rule is exercised
    if fname.endswith("s.bin"):
        assert min(unflagged.values()) >= 2, unflagged


def test_golden64s_cover_every_class():
    """g128v64s.bin holds, at every n of its list, every class the encoder can
    produce there (v64_inputs.required_modes: each mode over the vertical and
    over the horizontal base layout) plain and as the gaps of a delta-1 list,
    the exception modes also over no base (b = 0); across the file bitmap
    patches of bx <= 32 and bx > 32, plain and constant blocks of width
    exactly 63 and exactly 64, compressed vbyte from the smallest n that has
    it with every marker length 1..9, a list that wraps 2^64, and the
    decode-only bx = 0 header at b = 8, 40 and 63 with n = 128, 100 and 7.
    g256v64s.bin holds every class in each half, and the bx = 0 header in
    either half."""
    recs = golden_io.load("g128v64s.bin")
    by_n, lens, bx, top, bx0 = {}, set(), set(), set(), set()
    for r in recs:
        (_, blk), = blocks64("128v64", r)
        assert (blk.mode == "bx0") == r.decode_only
        if r.decode_only:
            bx0.add((blk.b, r.n, r.d1))
            continue
        by_n.setdefault((r.n, r.d1), set()).add(_class64(blk))
        lens.update(blk.lens)
        if blk.mode == "bitmap":
            bx.add(blk.bx > 32)
        if blk.b == 63 and not r.d1:
            top.add((blk.mode, int(r.values.max()).bit_length()))
    assert sorted({n for n, _ in by_n}) == [1, 2, 5, 7, 8, 9, 10, 31, 32, 33, 63, 64, 65, 100, 127]  # 5, 9, 10: where the vbyte classes begin
    for (n, d1), have in by_n.items():
        need = set(v64_inputs.required_modes(n))
        if n >= 2:
            need.add("bitmap_0")
        if n >= v64_inputs.VB_MIN_N64:
            need.add("vb_raw_0")
        if n >= v64_inputs.VB_COMP_MIN_N64:
            need.add("vb_comp_0")
        assert have == need, (n, d1, need ^ have)
    assert lens == set(range(1, 10)) and bx == {False, True}
    assert top == {("plain63", 63), ("plain63", 64), ("const63", 63), ("const63", 64)}
    assert bx0 == {(b, n, d1) for b in (8, 40, 63) for n in (128, 100, 7) for d1 in (False, True)}
    assert any(r.d1 and r.start > (1 << 64) - 2000 and r.values[-1] < r.start for r in recs)  # wraps 2^64
    recs = golden_io.load("g256v64s.bin")
    halves, lens, bx0 = [set(), set()], set(), set()
    for r in recs:
        for h, (bn, blk) in enumerate(blocks64("256v64", r)):
            if r.decode_only:
                bx0.add((h, blk.mode))
                continue
            halves[h].add(_class64(blk))
            lens.update(blk.lens)
    assert {r.n for r in recs} == {1, 100, 128, 129, 200, 255, 256}
    for h in halves:
        assert h == set(v64_inputs.required_modes(128)) | {"bitmap_0", "vb_raw_0", "vb_comp_0"}, h
    assert lens == set(range(1, 10))
    assert {(0, "bx0"), (1, "bx0")} <= bx0
    assert any(r.d1 and r.start > (1 << 64) - 2000 and r.values[-1] < r.start for r in recs)


def test_short_32bit_units_are_pinned():
    """128v32 with n < 128 and 256v32 with n < 256: the reference's bytes
    depend on its uninitialised stack (flag 4) only where p4D1Enc* hands its
    n-delta temporary to the plain encoder and that packs the full width
    (p4d1enc128v32_scalar.cpp:12) -- delta-1, n below the width, plain mode.
    Everything else is byte-pinned, every vector without delta-1 included."""
    for fname, fmt, full in (("g128v32s.bin", "128v32", 128), ("g256v32s.bin", "256v32", 256)):
        recs = [r for r in golden_io.load(fname) if not r.decode_only]
        for i, r in enumerate(recs):
            if r.padding_unpinned:
                mode = p4_modes.parse32(r.enc, 0, r.n, full)[0]
                assert r.d1 and r.n < full and mode in ("plain", "plain32"), (fname, i, r.d1, r.n, mode)
        short = [r for r in recs if r.n < full]
        assert len(short) >= 200
        assert not any(r.padding_unpinned for r in short if not r.d1)
        pinned = [r for r in short if not r.padding_unpinned]
        assert len(pinned) >= len(short) // 2, (fname, len(pinned), len(short))
        assert any(r.padding_unpinned for r in short), fname  # the rule above is exercised


def test_golden32_covers_every_mode():
    """The 32-bit fixtures of every family (horizontal, 128v32, 256v32) reach
    every mode of p4_modes.MODES32 -- all zero, plain, plain at width 32,
    constant, constant at width 32, bitmap patch, the decode-only 0x80 | b
    header with bx == 0, vbyte raw and compressed -- and their compressed
    vbEnc32 streams carry every marker length, 1..5 bytes.  Every record
    parses to exactly its length; the short-unit files hold every n listed."""
    fams = {"32": ["g32.bin", "g32vb.bin"], "128v32": ["g128v32.bin", "g128v32s.bin"],
            "256v32": ["g256v32.bin", "g256v32s.bin"]}
    for fmt, fnames in fams.items():
        modes, lens = set(), set()
        for fname in fnames:
            by_n = {}
            for i, r in enumerate(golden_io.load(fname)):
                m, ls, end = p4_modes.parse32(r.enc, 0, r.n, p4_modes.BASE_N32[fmt])
                assert end == len(r.enc), (fname, i, m, end, len(r.enc))
                assert (m == "bx0") == r.decode_only, (fname, i, m)
                modes.add(m)
                lens.update(ls)
                by_n.setdefault(r.n, set()).add(m)
            if fname == "g128v32s.bin":
                assert set(by_n) == {1, 2, 7, 31, 32, 33, 63, 64, 65, 100, 127, 128}
            if fname == "g256v32s.bin":
                assert set(by_n) == {1, 63, 64, 65, 127, 128, 129, 200, 255, 256}
            if fname.endswith("s.bin"):
                assert any(r.d1 and r.start == 0xFFFFFF00 for r in golden_io.load(fname))  # a list that wraps 2^32
        for m in p4_modes.MODES32:
            assert m in modes, (fmt, m)
        assert lens == {1, 2, 3, 4, 5}, (fmt, sorted(lens))


def test_golden_covers_every_mode():
    """The 256v32 fixtures exercise plain, bitmap, vbyte (raw and compressed),
    constant and b=0 blocks, and the decode-only 0x80/bx=0 header."""
    recs = golden_io.load("g256v32.bin")
    modes = set()
    for r in recs:
        h = r.enc[0]
        if h & 0xC0 == 0xC0:
            modes.add("const")
        elif h & 0xC0 == 0x40:
            b = h & 0x3F
            v0 = 2 + 32 * b
            modes.add("vb_raw" if r.enc[v0] == 0xFF else "vb_comp")
        elif h & 0x80:
            modes.add("bitmap" if r.enc[1] else "bitmap0")
            if r.enc[1] and bin(int.from_bytes(r.enc[2:34], "little")).count("1") >= 32:
                modes.add("bitmap_xn32")
        else:
            modes.add("zero" if h == 0 else "plain")
    for m in ["const", "vb_raw", "vb_comp", "bitmap", "bitmap0", "bitmap_xn32", "zero", "plain"]:
        assert m in modes, m


def test_golden64_covers_every_mode():
    """The horizontal 64-bit fixture (p4Enc64 / p4Dec64) reaches every mode,
    read from the header bytes: all zero, plain, plain with header 63 (width
    63 or 64), constant, constant with header 63, bitmap patch, vbyte raw and
    compressed, and the decode-only 0x80 | b header with bx == 0 -- and the
    compressed vbyte streams carry every vbEnc64 length, 1..9 bytes."""
    recs = golden_io.load("g64.bin")
    modes, lens, by_n = set(), set(), {}
    for i, r in enumerate(recs):
        m, ls, end = p4_modes.parse64(r.enc, 0, r.n)
        assert end == len(r.enc), (i, m, end, len(r.enc))
        assert (m == "bx0") == r.decode_only, (i, m)
        modes.add(m)
        lens.update(ls)
        by_n.setdefault(r.n, set()).add(m)
    for m in p4_modes.MODES64:
        assert m in modes, m
    assert lens == set(range(1, 10)), sorted(lens)
    assert set(by_n) == {1, 2, 63, 64, 65, 127, 128, 129, 255, 256}
    assert any(r.d1 and r.start > (1 << 64) - 2000 for r in recs)  # a delta-1 list that wraps 2^64
