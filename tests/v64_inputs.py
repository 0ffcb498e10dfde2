"""Seeded inputs for the interleaved 64-bit codec tests (128v64 at every n and
256v64, through the generic kernels, the run-pipelined 256v64 kernels, the
per-block API and the chained decode).  Test infrastructure only."""
import functools

import numpy as np

import p4_modes
from h64_inputs import ONE, U64, _below, d1_list, mixed_vbyte_blocks

WIDTH = {"128v64": 128, "256v64": 256}

SHORT_N = [1, 2, 4, 5, 7, 8, 9, 10, 31, 32, 33, 63, 64, 65, 100, 127]
V64_CASES = [("128v64", n) for n in SHORT_N] + [("128v64", 128), ("256v64", 256)]
PAD_CASES = [("128v64", 100), ("128v64", 7), ("128v64", 65)]
BLOCK_SIZE_CASES = V64_CASES + [("256v64", n) for n in (129, 200, 255)]
PER_BLOCK_CASES = [("128v64", 7), ("128v64", 65), ("128v64", 127), ("256v64", 129), ("256v64", 255)]
CHAIN_START0 = (1 << 64) - 4096  # the chained delta-1 list wraps 2^64

# Smallest n at which the encoder can pick vbyte exceptions at all.  p4Bits64
# reads only the values' bit widths (and whether all values are equal).  Over
# every multiset of n widths 0..64 at n = 2, 3, 4 (2,145, 47,905 and 814,385
# multisets through orc_p4bits64) it never picks vbyte.  At n = 5 it does --
# unlike the 32-bit codec, which cannot below n = 9: p4Bits64 prices a vbyte
# exception at 11 bytes at the most, however wide, while the bitmap patch
# charges every exception the widest one's bits, so two exceptions, one about
# 13 bits over a narrow base and one reaching bit 63 (widths 0, 0, 1, 13, 63),
# are cheaper as vbyte (raw: fewer than 5 exceptions are never compressed).
# test_v64_inputs_cpu.py repeats the enumeration and the search.
VB_MIN_N64 = 5
# ... over a horizontal base (b > 32), where no excess has more than 31 bits
# and that asymmetry is gone: none in 60,000 mixed-width draws per n at n =
# 5..8 (a base of width 0..40 and one to n - 1 exceptions of 1..8, 9..29 or 30
# and more bits of excess; test_mixed_width_draws_find_no_earlier_vbyte
# repeats 5,000 of them per n), nor in the directed search of
# test_smallest_n_with_vbyte; at n = 9, where the bitmap takes two bytes, one
# exception 8..15 bits over the base is cheaper as vbyte on either layout.
VB_H_MIN_N64 = 9
# Smallest n with COMPRESSED vbyte.  vbEnc64 keeps the compressed stream only
# when it is 32 bytes under the raw one (sumlen + 32 <= 8 * xn with sumlen >=
# xn: at least 5 exceptions).  At n = 10 four exceptions whose excess has
# exactly 7 bits (one-byte markers, which seven more base bits would absorb at
# ceil(70 / 8) = 9 bytes against 8 for the exceptions) and one outlier 15 bits
# over the base (a 3-byte marker; sumlen = 7, 7 + 32 <= 40) are compressed
# vbyte over either base layout; the same directed search finds none at n =
# 5..9 (at n = 9 seven more base bits cost 8 bytes, no more than the
# exceptions), and neither do the mixed-width draws above.  n = 4, 5 and 10
# are therefore tested n.
VB_COMP_MIN_N64 = 10
# From this n mixed_vbyte_blocks' n/8..n/3 exceptions number at least 5;
# below it the compressed class is tight_vbyte_blocks.
MIXED_MIN_N = 40


def required_modes(n):
    """The classes a test at n must reach (p4_modes.SPLIT64 names): everything
    the encoder can produce there.  n = 1 is all zero or constant; see
    VB_MIN_N64, VB_H_MIN_N64 and VB_COMP_MIN_N64 for the vbyte classes."""
    if n == 1:
        return ["zero", "const", "const63"]
    need = ["zero", "const", "const63", "plain_v", "plain_h", "plain63", "bitmap_v", "bitmap_h"]
    if n >= VB_MIN_N64:
        need.append("vb_raw_v")
    if n >= VB_H_MIN_N64:
        need.append("vb_raw_h")
    if n >= VB_COMP_MIN_N64:
        need += ["vb_comp_v", "vb_comp_h"]
    return need


def _of_width(rng, w):
    """One value of width exactly w (w >= 1)."""
    return (ONE << U64(w - 1)) | _below(rng, (), w - 1)


def _base(rng, n, b):
    """n values of at most b bits, one of them exactly b bits wide."""
    v = _below(rng, (n,), b)
    if b:
        v[int(rng.integers(0, n))] |= ONE << U64(b - 1)
    return v


def wide_base_vbyte_blocks(rng, nb, n):
    """COMPRESSED vbyte over a horizontal base (n >= MIXED_MIN_N): a base of
    width 33..50, xn exceptions with n/8 <= xn <= n/3 whose excess over the
    base is 1..149 (a one-byte marker), then one to three of them replaced by
    a value of random width in [b + 8, 64]."""
    out = np.zeros((nb, n), dtype=np.uint64)
    for i in range(nb):
        b = int(rng.integers(33, 51))
        v = _below(rng, (n,), b)
        xn = int(rng.integers(-(-n // 8), n // 3 + 1))
        pos = rng.choice(n, size=xn, replace=False)
        v[pos] |= rng.integers(1, 150, size=xn, dtype=np.uint64) << U64(b)
        for p in pos[: int(rng.integers(1, 4))]:
            v[p] = _of_width(rng, int(rng.integers(b + 8, 65)))
        out[i] = v
    return out


def tight_vbyte_blocks(rng, nb, n, wide):
    """COMPRESSED vbyte at small n (VB_COMP_MIN_N64 <= n < MIXED_MIN_N): a
    base of width 0..3 (wide: 33..40), 4..12 exceptions (at most 2n/5) whose
    excess has exactly 7 bits (one-byte markers that seven more base bits
    would absorb at 7n/8 bytes) and one outlier 15 bits over the base (a
    2- or 3-byte marker: 16,535, 16,536 or any 15-bit excess), which prices
    the bitmap patch of every exception at that width."""
    out = np.zeros((nb, n), dtype=np.uint64)
    for i in range(nb):
        b = int(rng.integers(33, 41)) if wide else int(rng.integers(0, 4))
        v = _below(rng, (n,), b)
        xn = int(rng.integers(4, min(12, (2 * n) // 5) + 1))
        pos = rng.choice(n, size=xn + 1, replace=False)
        v[pos[:xn]] |= rng.integers(64, 128, size=xn, dtype=np.uint64) << U64(b)
        k = (16535, 16536, int(rng.integers(1 << 14, 1 << 15)))[int(rng.integers(0, 3))]
        v[pos[xn]] = (v[pos[xn]] & ((ONE << U64(b)) - ONE)) | (U64(k) << U64(b))
        out[i] = v
    return out


def boundary_vbyte_blocks(rng, nb, n, wide):
    """COMPRESSED vbyte whose long values sit on the boundaries between the
    vbEnc64 forms (n >= MIXED_MIN_N): a base of width 0..11 (wide: 33..50)
    with every bit set in one value, so that no narrower base fits, n/8..n/3
    exceptions whose excess is 1..149, and one to three of them with an
    excess from p4_modes.VB64_BOUNDS (151 | 152, 16,535 | 16,536, 2,113,687 |
    2,113,688: the last value of a form and the first of the next)."""
    out = np.zeros((nb, n), dtype=np.uint64)
    for i in range(nb):
        b = int(rng.integers(33, 51)) if wide else int(rng.integers(0, 12))
        v = _below(rng, (n,), b)
        xn = int(rng.integers(-(-n // 8), n // 3 + 1))
        pos = rng.choice(n, size=xn + 1, replace=False)
        v[pos[xn]] = (ONE << U64(b)) - ONE
        v[pos[:xn]] |= rng.integers(1, 150, size=xn, dtype=np.uint64) << U64(b)
        for p in pos[: int(rng.integers(1, 4))]:
            k = p4_modes.VB64_BOUNDS[int(rng.integers(0, 6))]
            v[p] = (v[p] & ((ONE << U64(b)) - ONE)) | (U64(k) << U64(b))
        out[i] = v
    return out


def few_wide_blocks(rng, nb, n, wide):
    """A base of width 0..20 (wide: 33..50) with one to three values 8 or
    more bits over it: raw vbyte from n = VB_MIN_N64 (fewer than 5 exceptions
    are never compressed), a bitmap patch below."""
    out = np.zeros((nb, n), dtype=np.uint64)
    for i in range(nb):
        b = int(rng.integers(33, 51)) if wide else int(rng.integers(0, 21))
        v = _base(rng, n, b)
        for p in rng.choice(n, size=min(n - 1, int(rng.integers(1, 4))), replace=False):
            v[p] = _of_width(rng, int(rng.integers(b + 8, 65)))
        out[i] = v
    return out


def two_tier_blocks(rng, nb, n):
    """Raw vbyte at VB_MIN_N64 <= n < VB_H_MIN_N64: a base of width 0..5, one
    value 10..15 bits over it and one 62..64 bits wide (see VB_MIN_N64)."""
    out = np.zeros((nb, n), dtype=np.uint64)
    for i in range(nb):
        b = int(rng.integers(0, 6))
        v = _base(rng, n, b)
        p, q = rng.choice(n, size=2, replace=False)
        v[p] = _of_width(rng, b + int(rng.integers(10, 16)))
        v[q] = _of_width(rng, int(rng.integers(62, 65)))
        out[i] = v
    return out


def patched_wide_base_blocks(rng, nb, n):
    """Bitmap patch over a horizontal base: a base of width 33..50 and n/16
    (at least one, fewer than n) exceptions of one width up to 64."""
    out = np.zeros((nb, n), dtype=np.uint64)
    for i in range(nb):
        b = int(rng.integers(33, 51))
        v = _base(rng, n, b)
        w = int(rng.integers(b + 1, 65))
        for p in rng.choice(n, size=min(n - 1, max(1, n // 16)), replace=False):
            v[p] = _of_width(rng, w)
        out[i] = v
    return out


def v64_values(rng, nb, n):
    """128v64 blocks of every mode and base layout at every n: the mix of
    h64_inputs.h64_values (a base width 0..64 and an exception rate from {0,
    0.02, 0.1, 0.3} with magnitudes up to bit 64; constant blocks, a quarter
    of them 63 or 64 bits wide; all-zero blocks; blocks of width exactly 63,
    dense and with one top value) and the directed classes above, each on the
    vertical (b <= 32) and on the horizontal (b > 32) base layout: plain,
    bitmap patch, a few wide values (raw vbyte), compressed vbyte and its
    values on the boundaries between the vbEnc64 forms, where n admits them
    (required_modes)."""
    bw = rng.integers(0, 65, size=(nb, 1))
    vals = _below(rng, (nb, n), bw)
    rate = rng.choice([0.0, 0.02, 0.1, 0.3], size=(nb, 1))
    exc = rng.random((nb, n)) < rate
    big = _below(rng, (nb, n), rng.integers(1, 65, size=(nb, 1)))
    vals = np.where(exc, big, vals)
    kind = rng.random(nb)

    def of(lo, hi):
        return np.nonzero((kind >= lo) & (kind < hi))[0]

    for i in of(0.0, 0.10):  # constant
        w = int(rng.choice([63, 64])) if rng.random() < 0.25 else int(rng.integers(1, 63))
        vals[i] = _of_width(rng, w)
    vals[of(0.10, 0.13)] = 0  # all zero
    for i in of(0.13, 0.16):  # width exactly 63 or 64, dense
        w = int(rng.choice([63, 64]))
        vals[i] = _base(rng, n, w)
    for i in of(0.16, 0.18):  # width exactly 63, one top value
        vals[i] = _below(rng, (n,), int(rng.integers(0, 30)))
        vals[i, int(rng.integers(0, n))] = (ONE << U64(62)) | U64(5)
    for i in of(0.18, 0.23):  # plain on the horizontal layout
        vals[i] = _base(rng, n, int(rng.integers(33, 63)))
    for i in of(0.23, 0.28):  # plain on the vertical layout
        vals[i] = _base(rng, n, int(rng.integers(1, 33)))
    if n >= 2:
        ix = of(0.28, 0.34)
        vals[ix] = patched_wide_base_blocks(rng, len(ix), n)
        ix = of(0.34, 0.40)
        vals[ix] = few_wide_blocks(rng, len(ix), n, True)
        ix = of(0.40, 0.45)
        vals[ix] = two_tier_blocks(rng, len(ix), n) if VB_MIN_N64 <= n < VB_H_MIN_N64 else few_wide_blocks(rng, len(ix), n, False)
    if n >= VB_COMP_MIN_N64:
        ix, jx = of(0.45, 0.53), of(0.53, 0.61)
        if n >= MIXED_MIN_N:
            vals[ix] = wide_base_vbyte_blocks(rng, len(ix), n)
            vals[jx] = mixed_vbyte_blocks(rng, len(jx), n)
            ix, jx = of(0.61, 0.66), of(0.66, 0.71)
            vals[ix] = boundary_vbyte_blocks(rng, len(ix), n, True)
            vals[jx] = boundary_vbyte_blocks(rng, len(jx), n, False)
        else:
            vals[ix] = tight_vbyte_blocks(rng, len(ix), n, True)
            vals[jx] = tight_vbyte_blocks(rng, len(jx), n, False)
    return np.ascontiguousarray(vals, dtype=np.uint64)


def padded(vals, fmt, fill=0):
    """(nb, n) -> (nb, layout width) units at the full stride; the slots past
    n hold `fill` (a scalar or an (nb, width - n) array)."""
    nb, n = vals.shape
    u = WIDTH[fmt]
    out = np.zeros((nb, u), dtype=np.uint64)
    out[:, :n] = vals
    if u > n:
        out[:, n:] = fill
    return out


def oracle_stream(fmt, units, n, starts=None):
    """The oracle's encoding of every row's first n values, one unit per row;
    a plain-mode 128v64 block without delta-1 carries the row's slots past n
    (oracle_lib.encode's pad).  -> (packed uint8, offsets uint64)"""
    import oracle_lib

    encs = [oracle_lib.encode(fmt, row[:n], d1=starts is not None, start=0 if starts is None else int(starts[i]), pad=row[n:])
            for i, row in enumerate(units)]
    off = np.concatenate([[0], np.cumsum([len(e) for e in encs])]).astype(np.uint64)
    return np.frombuffer(b"".join(encs), dtype=np.uint8).copy(), off


def block_ns(fmt, n):
    """The n of each 128v64 block of one unit."""
    return [n] if fmt == "128v64" else [min(128, n - c) for c in range(0, n, 128)]


def blocks_of(fmt, packed, off, n):
    """Every 128v64 block of a stream, in order: (unit, block's n, Block64)."""
    out = []
    for i in range(len(off) - 1):
        p = int(off[i])
        for bn in block_ns(fmt, n):
            blk = p4_modes.parse64(packed, p, bn, 128)
            out.append((i, bn, blk))
            p = blk.end
        assert p == int(off[i + 1]), (i, p, int(off[i + 1]))
    return out


def census(fmt, packed, off, n):
    """p4_modes.count64 by base layout over the 128v64 blocks of a stream (a
    256v64 unit of n values: a block of 128 and one of n - 128)."""
    return p4_modes.count64(packed, [blk for _, _, blk in blocks_of(fmt, packed, off, n)], split=True)


def as_bx0(fmt, packed, off, n):
    """Rewrite every plain block (header b, width 63 / 64 included) of a
    128v64 / 256v64 stream as the decode-only form 0x80 | b with a bx byte of
    0 (p4d1dec128v64_scalar.cpp:211, :298), which the encoder never emits.
    -> (packed, offsets, rewritten blocks on the vertical layout, on the
    horizontal one)"""
    parts, noff, kv, kh = [], [0], 0, 0
    pos, unit = 0, 0
    for i, _, blk in blocks_of(fmt, packed, off, n):
        if i != unit:
            noff.append(sum(len(p) for p in parts))
            unit = i
        raw = packed[pos: blk.end]
        if blk.mode in ("plain", "plain63"):
            raw = np.concatenate([np.array([0x80 | int(raw[0]), 0], dtype=np.uint8), raw[1:]])
            kv += blk.b <= 32
            kh += blk.b > 32
        parts.append(raw)
        pos = blk.end
    noff.append(sum(len(p) for p in parts))
    return np.concatenate(parts), np.array(noff, dtype=np.uint64), kv, kh


def check_census(c):
    """The conditions test_v64_vs_oracle asserts again before it runs: every
    class the encoder can produce at n in at least 10 units (256v64: in each
    half), bitmap blocks of either patch-width range in at least 10."""
    halves = [c.modes] if c.fmt == "128v64" else []
    if c.fmt == "256v64":
        blocks = blocks_of(c.fmt, c.packed, c.off, c.n)
        for h in (0, 1):
            m = {}
            for _, _, blk in blocks[h::2]:
                m[blk.split] = m.get(blk.split, 0) + 1
            halves.append(m)
    for h, bn in zip(halves, block_ns(c.fmt, c.n)):
        for m in required_modes(bn):
            assert h.get(m, 0) >= 10, (c.fmt, c.n, c.d1, m, dict(h))
    bounds = p4_modes.VB64_BOUNDS if min(block_ns(c.fmt, c.n)) >= MIXED_MIN_N else (16535, 16536) if c.n >= VB_COMP_MIN_N64 else ()
    for k in bounds:  # compressed vbyte exceptions on each side of the boundaries between the forms
        assert c.modes[("vb", k)] >= 3, (c.fmt, c.n, c.d1, k, c.modes[("vb", k)])
    if c.n > 1:
        assert c.modes["bx_le32"] >= 10 and c.modes["bx_gt32"] >= 10, dict(c.modes)


class Case:
    """One (fmt, n, d1) input set with the oracle's stream of it: gaps
    (nu, n), vals (the gaps, or with d1 the chained list they span from
    CHAIN_START0), starts (d1: the value before each unit), units (vals at the
    full stride, zero past n), packed / off (the oracle's bytes), modes / lens
    (census of them by base layout)."""

    def __init__(self, fmt, n, d1, gaps):
        self.fmt, self.n, self.d1, self.gaps = fmt, n, d1, gaps
        self.nu = len(gaps)
        self.vals, self.starts = d1_list(gaps, CHAIN_START0) if d1 else (gaps, None)
        self.units = padded(self.vals, fmt)
        self.packed, self.off = oracle_stream(fmt, self.units, n, self.starts)
        self.modes, self.lens = census(fmt, self.packed, self.off, n)


@functools.lru_cache(maxsize=4)
def v64_case(fmt, n, d1, nu=1029):
    """The mixed-mode units of test_v64_vs_oracle: 1029 = 16 full 64-unit
    workgroups and a ragged run of 5.  A 256v64 unit is a 128-value block and
    one of n - 128, each drawn on its own, so that each half carries every
    class.  Cached: callers leave the arrays unchanged."""
    rng = np.random.default_rng([64000, n, int(d1), int(fmt == "256v64")])
    if fmt == "256v64":
        gaps = np.concatenate([v64_values(rng, nu, 128), v64_values(rng, nu, n - 128)], axis=1)
    else:
        gaps = v64_values(rng, nu, n)
    return Case(fmt, n, d1, gaps)
