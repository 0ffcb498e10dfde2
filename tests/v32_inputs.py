"""Seeded inputs for the 32-bit codec tests (128v32, 256v32 and the horizontal
p4Enc32 at every n, through the generic kernels and the 256v32 hot path).
Test infrastructure only."""
import functools

import numpy as np

import p4_modes

U32 = np.uint32
WIDTH = {"128v32": 128, "256v32": 256}

SHORT_N = {"128v32": [1, 2, 7, 31, 32, 33, 63, 64, 65, 100, 127], "256v32": [1, 63, 64, 65, 127, 128, 129, 200, 255]}
V32_CASES = [(f, n) for f in ("128v32", "256v32") for n in SHORT_N[f]] + [("128v32", 128)]
PAD_CASES = [("128v32", 100), ("128v32", 7), ("256v32", 200), ("256v32", 65)]
VBYTE_CASES = [("32", 127), ("32", 256), ("128v32", 128), ("128v32", 100), ("256v32", 200), ("256v32", 256)]
CHAIN_START0 = 0xFFFFF000  # the chained delta-1 list wraps 2^32

# Smallest n at which the encoder can pick vbyte exceptions at all.  p4Bits32
# reads only the values' bit widths, and up to n = 8 the bitmap patch costs one
# bitmap byte: over every multiset of n widths 0..32 (15,380,937 at n = 7,
# 76,904,685 at n = 8, enumerated through orc_p4bits32) it never picks vbyte;
# at n = 9 it does.  test_v32_inputs_cpu.py repeats the enumeration at n = 2, 3.
VB_MIN_N = 9
# Smallest n with COMPRESSED vbyte.  vbEnc32 keeps the compressed stream only
# when it is 32 bytes under the raw one (sumlen + 32 <= 4 * xn, sumlen >= xn:
# at least 11 exceptions, so never at n <= 10), and p4Bits32 prices a vbyte
# exception at 2 bytes or more against n / 8 bytes per base bit that would
# absorb it, so eleven cheap exceptions pay only when n is a few times eleven.
# The directed search of test_v32_inputs_cpu.py finds compressed blocks at
# n = 26 and none at 11..25; no n between 9 and 30 is among the tested ones.
VB_COMP_MIN_N = 26


def required_modes(n):
    """The modes a test at n must reach (census32 names): everything the
    encoder can produce there.  n = 1 is all zero or constant; see VB_MIN_N
    and VB_COMP_MIN_N for the vbyte modes."""
    if n == 1:
        return ["zero", "const", "const32"]
    need = ["zero", "const", "const32", "plain", "plain32", "bitmap"]
    if n >= VB_MIN_N:
        need.append("vb_raw")
    if n >= VB_COMP_MIN_N:
        need.append("vb_comp")
    return need


def _below(rng, shape, width):
    """Uniform uint32 values of at most `width` bits (width 0..32, broadcast)."""
    w = np.broadcast_to(np.asarray(width, dtype=np.uint64), shape)
    r = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64)
    return (r >> (np.uint64(32) - w)).astype(np.uint32)


def _of_width(rng, w):
    """One value of width exactly w (w >= 1)."""
    return U32((1 << (w - 1)) | int(rng.integers(0, 1 << (w - 1))))


def mixed_vbyte_blocks(rng, nb, n):
    """Blocks that make the encoder choose COMPRESSED vbEnc32 exceptions with
    every marker length: a base of width 0..8, xn exceptions with n/8 <= xn <=
    n/3 whose excess over the base is 1..149 (a one-byte marker), then one to
    three of them replaced by a value of random width in [b + 9, 32] (the 2-,
    3-, 4- and 5-byte forms).  The many short markers keep the compressed
    stream 32 bytes under the raw one."""
    out = np.zeros((nb, n), dtype=np.uint32)
    for i in range(nb):
        b = int(rng.integers(0, 9))
        v = _below(rng, (n,), b)
        xn = int(rng.integers(-(-n // 8), n // 3 + 1))
        pos = rng.choice(n, size=xn, replace=False)
        v[pos] |= (rng.integers(1, 150, size=xn, dtype=np.uint64) << np.uint64(b)).astype(np.uint32)
        for p in pos[: int(rng.integers(1, 4))]:
            v[p] = _of_width(rng, int(rng.integers(b + 9, 33)))
        out[i] = v
    return out


def vbyte32_gaps(fmt, n, nu, seed=1):
    """nu units of mixed_vbyte_blocks, n values each (fmt: for the seed only,
    every 32-bit layout takes the same values)."""
    rng = np.random.default_rng([seed, n, {"32": 0, "128v32": 1, "256v32": 2}[fmt]])
    return mixed_vbyte_blocks(rng, nu, n)


def tight_vbyte_blocks(rng, nb, n):
    """Compressed vbyte at small n (n < 64), where mixed_vbyte_blocks' n/3
    exceptions are fewer than the 11 it takes: a base of width 0..3, 11 or 12
    exceptions whose excess has exactly 7 bits (one-byte markers that seven
    more base bits would absorb at 7n/8 bytes), and one outlier 16 or 18 bits
    over the base (a 2- or 3-byte marker), which prices the bitmap patch of
    every exception at that width."""
    out = np.zeros((nb, n), dtype=np.uint32)
    for i in range(nb):
        b = int(rng.integers(0, 4))
        v = _below(rng, (n,), b)
        xn = int(rng.integers(11, 13))
        pos = rng.choice(n, size=xn + 1, replace=False)
        v[pos[:xn]] |= (rng.integers(64, 128, size=xn, dtype=np.uint64) << np.uint64(b)).astype(np.uint32)
        v[pos[xn]] = _of_width(rng, b + int(rng.choice([16, 18])))
        out[i] = v
    return out


def v32_values(rng, nb, n):
    """32-bit blocks of every mode at every n: per block a base width 0..32
    and an exception rate from {0, 0.02, 0.1, 0.3} with magnitudes up to bit 32
    (plain, bitmap patch and raw vbyte); constant blocks, a quarter of them 32
    bits wide; all-zero blocks; blocks whose every value is 32 bits wide
    (plain at b = 32); a narrow base with one to three large values (raw
    vbyte); and the compressed-vbyte classes above where n admits them."""
    bw = rng.integers(0, 33, size=(nb, 1))
    vals = _below(rng, (nb, n), bw)
    rate = rng.choice([0.0, 0.02, 0.1, 0.3], size=(nb, 1))
    exc = rng.random((nb, n)) < rate
    big = _below(rng, (nb, n), rng.integers(8, 33, size=(nb, 1)))
    vals = np.where(exc, big, vals)
    kind = rng.random(nb)
    for i in np.nonzero(kind < 0.12)[0]:  # constant
        vals[i] = _of_width(rng, 32 if rng.random() < 0.3 else int(rng.integers(1, 32)))
    vals[(kind >= 0.12) & (kind < 0.16)] = 0  # all zero
    dense = (kind >= 0.16) & (kind < 0.22)  # every value 32 bits wide: plain, b = 32
    vals[dense] |= U32(0x80000000)
    for i in np.nonzero((kind >= 0.22) & (kind < 0.30))[0]:  # narrow base, a few large values
        vals[i] = _below(rng, (n,), int(rng.integers(0, 6)))
        for p in rng.choice(n, size=min(n, int(rng.integers(1, 4))), replace=False):
            vals[i, p] = _of_width(rng, int(rng.integers(20, 33)))
    mix = np.nonzero((kind >= 0.30) & (kind < 0.42))[0]
    if n >= VB_COMP_MIN_N and len(mix):
        vals[mix] = tight_vbyte_blocks(rng, len(mix), n) if n < 64 else mixed_vbyte_blocks(rng, len(mix), n)
    return np.ascontiguousarray(vals, dtype=np.uint32)


def d1_list(gaps, start0):
    """The delta-1 list whose gaps are `gaps` (nb, n): x = start0 + cumulative
    (gap + 1), mod 2^32, and each block's start (the value before it)."""
    nb, n = gaps.shape
    x = ((np.cumsum(gaps.ravel().astype(np.uint64) + np.uint64(1), dtype=np.uint64) + np.uint64(start0))
         & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(nb, n)
    starts = np.empty(nb, dtype=np.uint32)
    starts[0] = start0
    starts[1:] = x[:-1, -1]
    return x, starts


def padded(vals, fmt, fill=0):
    """(nb, n) -> (nb, layout width) units at the full stride; the slots past
    n hold `fill` (a scalar or an (nb, width - n) array)."""
    nb, n = vals.shape
    u = WIDTH.get(fmt, n)
    out = np.zeros((nb, u), dtype=np.uint32)
    out[:, :n] = vals
    if u > n:
        out[:, n:] = fill
    return out


def oracle_stream(fmt, units, n, starts=None):
    """The oracle's encoding of every row's first n values, one block per
    row; a plain-mode block without delta-1 carries the row's slots past n
    (oracle_lib.encode's pad).  -> (packed uint8, offsets uint64)"""
    import oracle_lib

    encs = [oracle_lib.encode(fmt, row[:n], d1=starts is not None, start=0 if starts is None else int(starts[i]), pad=row[n:])
            for i, row in enumerate(units)]
    off = np.concatenate([[0], np.cumsum([len(e) for e in encs])]).astype(np.uint64)
    return np.frombuffer(b"".join(encs), dtype=np.uint8).copy(), off


def as_bx0(packed, off, n, base_n=None):
    """Rewrite every plain block (header b, plain32 included) of a 32-bit
    stream as the decode-only form 0x80 | b with a bx byte of 0, which the
    encoder never emits.  -> (packed, offsets, number of rewritten blocks)"""
    parts, noff, k = [], [0], 0
    for i in range(len(off) - 1):
        blk = packed[int(off[i]): int(off[i + 1])]
        if p4_modes.parse32(packed, int(off[i]), n, base_n)[0] in ("plain", "plain32"):
            blk = np.concatenate([np.array([0x80 | int(blk[0]), 0], dtype=np.uint8), blk[1:]])
            k += 1
        parts.append(blk)
        noff.append(noff[-1] + len(blk))
    return np.concatenate(parts), np.array(noff, dtype=np.uint64), k


class Case:
    """One (fmt, n, d1) input set with the oracle's stream of it: gaps
    (nu, n), vals (the gaps, or with d1 the chained list they span from
    CHAIN_START0), starts (d1: the value before each unit), units (vals at the
    full stride, zero past n), packed / off (the oracle's bytes), modes / lens
    (census32 of them)."""

    def __init__(self, fmt, n, d1, gaps):
        self.fmt, self.n, self.d1, self.gaps = fmt, n, d1, gaps
        self.nu = len(gaps)
        self.base_n = p4_modes.BASE_N32[fmt]
        self.vals, self.starts = d1_list(gaps, CHAIN_START0) if d1 else (gaps, None)
        self.units = padded(self.vals, fmt)
        self.packed, self.off = oracle_stream(fmt, self.units, n, self.starts)
        self.modes, self.lens = p4_modes.census32(self.packed, self.off, n, self.base_n)


_FCODE = {"32": 0, "128v32": 1, "256v32": 2}


@functools.lru_cache(maxsize=4)
def v32_case(fmt, n, d1, nu=1029):
    """The mixed-mode units of test_v32_vs_oracle: 1029 = 16 full 64-unit
    workgroups (four waves of 16-unit runs) and a ragged run of 5.  Cached:
    callers leave the arrays unchanged."""
    rng = np.random.default_rng([32000, n, int(d1), _FCODE[fmt]])
    return Case(fmt, n, d1, v32_values(rng, nu, n))


def vbyte_case(fmt, n, d1, nu=400):
    return Case(fmt, n, d1, vbyte32_gaps(fmt, n, nu))
