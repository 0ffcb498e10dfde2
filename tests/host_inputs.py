"""The case matrix of the host-stream tests (tests/test_host_streams_cpu.py,
tests/test_gpu_host_streams.py): every format the host entries accept at its
smallest, a short and its full n, in three modes, with the oracle's stream of
each.  The expectation composes every unit with its TRUE start through the
oracle alone; nothing the library computes enters it.  Test infrastructure
only."""
import functools

import numpy as np

import h64_inputs
import oracle_lib
import v32_inputs
import v64_inputs

FMT_NAME = {0: "32", 1: "128v32", 2: "256v32", 3: "64", 4: "128v64", 5: "256v64"}
WIDTH = {1: 128, 2: 256, 4: 128, 5: 256}  # the unit stride of the interleaved layouts (the others: n)
PAIRS = [(0, 1), (0, 127), (0, 256), (1, 1), (1, 100), (1, 128), (2, 1), (2, 200), (2, 256),
         (3, 1), (3, 127), (3, 256), (4, 1), (4, 100), (4, 128), (5, 256)]
MULTI_PAIRS = [(0, 127), (1, 100), (2, 200), (3, 127), (4, 100), (5, 256)]
# plain; delta-1 as ONE chained list (h_starts = NULL, start0 near the top of
# the range: the list wraps 2^32 / 2^64); delta-1 with a start per unit
MODES = ("plain", "chain", "starts")
CHUNK_UNITS = 5  # TPF_HOST_CHUNK_BYTES = five units of the pair's value bytes
# one chunk, an exactly full chunk, a ragged one-unit tail, exactly three
# slots, the first slot reuse, seven chunks plus one unit
NBLOCKS = (1, 5, 6, 15, 16, 36)
MAX_NB = 36
ONE_UNIT_NB = 7  # the run with TPF_HOST_CHUNK_BYTES = 1 (every chunk one unit)
MULTI_NBLOCKS = (2, 16, 36)
MULTI_K = (2, 3)


def wide(fmt):
    return fmt >= 3


def width(fmt, n):
    return WIDTH.get(fmt, n)


def _gaps(fmt, n, rng, nb, flat):
    """flat: no exceptions (a base width per unit only), so that most units
    are plain-mode blocks, which carry the padding slots."""
    if flat:
        below = h64_inputs._below if wide(fmt) else v32_inputs._below
        g = below(rng, (nb, n), rng.integers(1, 65 if wide(fmt) else 33, size=(nb, 1)))
        return np.ascontiguousarray(g, dtype=np.uint64 if wide(fmt) else np.uint32)
    if fmt in (0, 1, 2):
        return v32_inputs.v32_values(rng, nb, n)
    if fmt == 3:
        return h64_inputs.h64_values(rng, nb, n)
    if fmt == 4:
        return v64_inputs.v64_values(rng, nb, n)
    return np.concatenate([v64_inputs.v64_values(rng, nb, 128), v64_inputs.v64_values(rng, nb, n - 128)], axis=1)


def oracle_units(fmt, units, n, starts=None):
    """The oracle's stream of units (nb, stride): the first n values of every
    row, delta-1 from starts[i] when given; a plain block carries the row's
    slots past n.  -> (packed uint8, offsets uint64)"""
    if fmt == 0:
        return oracle_lib.enc32_batch(units[:, :n], starts)
    if fmt == 3:
        return oracle_lib.enc64_batch(units[:, :n], starts)
    mod = v64_inputs if wide(fmt) else v32_inputs
    return mod.oracle_stream(FMT_NAME[fmt], units, n, starts)


def oracle_unit(fmt, row, n, start=None):
    """One unit's bytes (start: delta-1 from it)."""
    return oracle_units(fmt, row[None, :], n, None if start is None else np.array([start], dtype=row.dtype))[0]


class HostCase:
    """One (fmt, n, mode) of the matrix, MAX_NB units long; every smaller
    nblocks is a prefix (each unit is composed with its own true start).

    units    (MAX_NB, stride) what the caller hands over as h_vals; the slots
             past n hold random non-zero words (plain) or, delta-1, a value
             that differs from the unit's value n - 1
    d1, h_starts, start0   the call's arguments (h_starts None: plain / chained)
    true_starts            delta-1: the value before each unit
    packed, off            the oracle's stream of all MAX_NB units"""

    def __init__(self, fmt, n, mode):
        self.fmt, self.n, self.mode = fmt, n, mode
        self.name = FMT_NAME[fmt]
        self.dtype = np.uint64 if wide(fmt) else np.uint32
        self.es = 8 if wide(fmt) else 4
        self.stride = width(fmt, n)
        self.short = n < self.stride
        self.chunk_bytes = CHUNK_UNITS * self.stride * self.es
        self.d1 = int(mode != "plain")
        rng = np.random.default_rng([77000, fmt, n, MODES.index(mode)])
        bits = 8 * self.es
        top = (1 << bits) - 1
        self.start0, self.h_starts, self.true_starts = 0, None, None
        # a plain short unit: no exceptions, or too few of v32_values' /
        # v64_values' units are plain-mode blocks (test_host_streams_cpu.py
        # asserts a quarter carry their padding)
        gaps = _gaps(fmt, n, rng, MAX_NB, flat=self.short and mode == "plain")
        d1_list = h64_inputs.d1_list if wide(fmt) else v32_inputs.d1_list
        if mode == "plain":
            vals = gaps
            fill = rng.integers(1, top, size=(MAX_NB, self.stride - n), dtype=np.uint64, endpoint=True).astype(self.dtype)
        else:
            if mode == "chain":
                self.start0 = v64_inputs.CHAIN_START0 if wide(fmt) else v32_inputs.CHAIN_START0
                vals, self.true_starts = d1_list(gaps, self.start0)
            else:
                st = rng.integers(0, top, size=MAX_NB, dtype=np.uint64, endpoint=True).astype(self.dtype)
                st[0] = top  # the first unit wraps at once
                vals = np.concatenate([d1_list(gaps[i: i + 1], int(st[i]))[0] for i in range(MAX_NB)])
                self.true_starts = self.h_starts = st
            with np.errstate(over="ignore"):
                fill = (vals[:, n - 1:n] + self.dtype(0x9E3779B1)).astype(self.dtype)
        self.gaps = gaps
        self.units = np.zeros((MAX_NB, self.stride), dtype=self.dtype)
        self.units[:, :n] = vals
        if self.short:
            self.units[:, n:] = fill
        self.packed, self.off = oracle_units(fmt, self.units, n, self.true_starts)
        assert self.packed.dtype == np.uint8 and len(self.off) == MAX_NB + 1 and int(self.off[-1]) == len(self.packed)
        for a in (self.units, self.packed, self.off, self.true_starts):
            if a is not None:
                a.setflags(write=False)

    @property
    def id(self):
        return f"{self.name}-n{self.n}-{self.mode}"

    def stream(self, nb, first=0):
        """The expected bytes and (rebased) offsets of units first .. first + nb."""
        o = self.off[first: first + nb + 1]
        return self.packed[int(o[0]): int(o[-1])], o - o[0]

    def starts_arg(self, nb, first=0):
        return None if self.h_starts is None else np.ascontiguousarray(self.h_starts[first: first + nb])

    def start0_arg(self, first=0):
        """start0 of a call that begins at unit `first` of the chained list."""
        return int(self.true_starts[first]) if self.mode == "chain" else 0


@functools.lru_cache(maxsize=None)
def case(fmt, n, mode):
    """Cached: callers leave the arrays unchanged (they are read-only)."""
    return HostCase(fmt, n, mode)


def cuts(nblocks):
    """Every position at which the GPU tests cut a stream of nblocks units:
    the chunk cuts at multiples of CHUNK_UNITS, the shard cuts nblocks * d / k
    and the chunk cuts inside each shard."""
    out = set(range(CHUNK_UNITS, nblocks, CHUNK_UNITS))
    for k in MULTI_K:
        sh = [nblocks * d // k for d in range(k + 1)]
        for a, b in zip(sh, sh[1:]):
            out |= set(range(a, b, CHUNK_UNITS))
    out.discard(0)
    return sorted(out)


ALL_CUTS = sorted(set().union(*[cuts(nb) for nb in set(NBLOCKS) | set(MULTI_NBLOCKS)]) | set(range(1, ONE_UNIT_NB)))


# the pairs and blocks of the corrupt-offset test: off[b] + 1 makes block
# b - 1 a byte too long (chunk 0, chunk 1, the reused slot, the ragged tail)
CORRUPT_PAIRS = [(2, 256), (3, 127), (1, 100)]
CORRUPT_AT = (3, 8, 18, MAX_NB - 1)


def corrupt_case(fmt, n):
    """The first mode of the pair whose blocks b - 1 and b are at least three
    bytes long at every b of CORRUPT_AT, so that bumped offsets never decrease."""
    for mode in MODES:
        c = case(fmt, n, mode)
        lens = np.diff(c.off.astype(np.int64))
        if all(lens[b - 1] >= 3 and lens[b] >= 3 for b in CORRUPT_AT):
            return c
    raise AssertionError((fmt, n))
