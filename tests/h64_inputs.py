"""Seeded inputs for the 64-bit codec tests (p4Enc64 / p4Dec64 and the vbyte
paths of 128v64 / 256v64).  Test infrastructure only."""
import numpy as np

U64 = np.uint64
ONE = np.uint64(1)


def _below(rng, shape, width):
    """Uniform values of at most `width` bits (width 0..64, broadcast)."""
    w = np.broadcast_to(np.asarray(width, dtype=np.uint64), shape)
    r = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64, endpoint=False)
    sh = (np.uint64(64) - w) & np.uint64(63)
    return np.where(w == 0, U64(0), np.where(w == 64, r, r >> sh))


def mixed_vbyte_blocks(rng, nb, n):
    """Blocks that make the encoder choose COMPRESSED vbyte exceptions with
    long forms: a base of width 0..11, xn exceptions with n/8 <= xn <= n/3
    whose excess over the base is 1..149 (a one-byte marker), then one to
    three of them replaced by a value of random width in [b + 8, 64] (the 2-
    and 3-byte markers and the 3..8-byte raw forms).  The many short markers
    keep the compressed stream 32 bytes under the raw one."""
    out = np.zeros((nb, n), dtype=np.uint64)
    for i in range(nb):
        b = int(rng.integers(0, 12))
        v = _below(rng, (n,), b)
        xn = int(rng.integers(-(-n // 8), n // 3 + 1))
        pos = rng.choice(n, size=xn, replace=False)
        v[pos] |= rng.integers(1, 150, size=xn, dtype=np.uint64) << U64(b)
        for p in pos[: int(rng.integers(1, 4))]:
            w = int(rng.integers(b + 8, 65))
            v[p] = (ONE << U64(w - 1)) | _below(rng, (), w - 1)
        out[i] = v
    return out


def wide_vbyte_gaps(fmt, n, nu, seed=1):
    """nu units of mixed_vbyte_blocks for fmt (a 256v64 unit: two 128-value blocks)."""
    rng = np.random.default_rng(seed)
    if fmt == "256v64":
        return mixed_vbyte_blocks(rng, 2 * nu, 128).reshape(nu, 256)
    return mixed_vbyte_blocks(rng, nu, n)


def h64_values(rng, nb, n):
    """p4Enc64 blocks of every mode: per block a base width 0..64, an
    exception rate from {0, 0.02, 0.1, 0.3} with magnitudes up to bit 64;
    about 10 percent constant blocks (a quarter of them 63 or 64 bits wide),
    a few all-zero blocks, blocks whose maximum width is exactly 63 (dense,
    and a single top value over a narrow base), and the mixed-exception
    class of mixed_vbyte_blocks."""
    bw = rng.integers(0, 65, size=(nb, 1))
    vals = _below(rng, (nb, n), bw)
    rate = rng.choice([0.0, 0.02, 0.1, 0.3], size=(nb, 1))
    exc = rng.random((nb, n)) < rate
    big = _below(rng, (nb, n), rng.integers(1, 65, size=(nb, 1)))
    vals = np.where(exc, big, vals)
    kind = rng.random(nb)
    for i in np.nonzero(kind < 0.10)[0]:  # constant
        w = int(rng.choice([63, 64])) if rng.random() < 0.25 else int(rng.integers(1, 63))
        vals[i] = (ONE << U64(w - 1)) | _below(rng, (), w - 1)
    vals[(kind >= 0.10) & (kind < 0.13)] = 0  # all zero
    for i in np.nonzero((kind >= 0.13) & (kind < 0.16))[0]:  # width exactly 63, dense
        vals[i] = (ONE << U64(62)) | _below(rng, (n,), 62)
    for i in np.nonzero((kind >= 0.16) & (kind < 0.19))[0]:  # width exactly 63, one top value
        vals[i] = _below(rng, (n,), int(rng.integers(0, 30)))
        vals[i, int(rng.integers(0, n))] = (ONE << U64(62)) | U64(5)
    mix = np.nonzero((kind >= 0.19) & (kind < 0.27))[0]
    if n >= 24 and len(mix):
        vals[mix] = mixed_vbyte_blocks(rng, len(mix), n)
    return np.ascontiguousarray(vals, dtype=np.uint64)


def d1_list(gaps, start0):
    """The delta-1 list whose gaps are `gaps` (nb, n): x = start0 + cumulative
    (gap + 1), mod 2^64, and each block's start (the value before it)."""
    nb, n = gaps.shape
    with np.errstate(over="ignore"):
        x = (np.cumsum(gaps.ravel() + ONE, dtype=np.uint64) + U64(start0)).reshape(nb, n)
    starts = np.empty(nb, dtype=np.uint64)
    starts[0] = start0
    starts[1:] = x[:-1, -1]
    return x, starts


def as_bx0(packed, off, n):
    """Rewrite every plain block (header b) of a p4Enc64 stream as the
    decode-only form 0x80 | b with a bx byte of 0 (p4dec64.cpp:95), which the
    encoder never emits.  -> (packed, offsets, number of rewritten blocks)"""
    import p4_modes

    parts, noff, k = [], [0], 0
    for i in range(len(off) - 1):
        blk = packed[int(off[i]): int(off[i + 1])]
        if p4_modes.parse64(packed, int(off[i]), n)[0] in ("plain", "plain63"):
            blk = np.concatenate([np.array([0x80 | int(blk[0]), 0], dtype=np.uint8), blk[1:]])
            k += 1
        parts.append(blk)
        noff.append(noff[-1] + len(blk))
    return np.concatenate(parts), np.array(noff, dtype=np.uint64), k
