"""Two seeded families of lists whose TAIL units (the horizontal p4Enc32 /
p4D1Enc32 block of a list's last n % 256 values) hold, at every count 1..255,
every mode the encoder can produce there -- the inputs of
tests/test_lists_tails_cpu.py and tests/test_gpu_lists_tails.py.

A list is a row of gaps and a start: the plain stream encodes the gaps
themselves, the delta-1 stream the list start0 + cumsum(gap + 1) mod 2^32, so
both tails hold the same deltas and the oracle encodes both in the same mode.
The rows are chosen by rejection: per count, rounds of CAND candidates of every
gap class are encoded by the oracle (oracle_lib.enc32_batch, one call per
round), their modes are read back from its bytes (p4_modes.parse32) and a row
is kept under the mode the oracle produced until every required mode has R
rows.  The k-th row of a (count, mode) group is a tail-only list for even k and
follows one full 256-value block for odd k, so its start comes from start0 or
from the skip table.

"wide": gaps of up to 32 bits, every 32-bit mode, lists that wrap 2^32.
"ascending": every gap below 2^CAP_BITS and start0 below 2^31, so that a list of
256 + 255 values ends below 2^31 + 511 * 2^22 < 2^32 and the numpy definitions
of the set operations (strictly ascending lists) apply.  No gap of 32 bits
exists there, so const32 and plain32 are dropped from its required modes; no
other mode is.  Test infrastructure only."""
import collections
import functools

import numpy as np

import lists_index as li
import lists_ref as ref
import oracle_lib as orc
import p4_modes
import v32_inputs as vi

R = 3                   # lists per (family, count, mode)
ROUNDS, CAND = 60, 2    # the bound of the draws: rounds per count, candidates per class and round
CAP_BITS = 22           # the widest gap of "ascending"
FAMILIES = ("wide", "ascending")
COUNTS = range(1, 256)
# (family, count, mode) triples whose floor is 1 instead of R.  Only vb_comp at
# counts 26..29 may ever stand here (test_lists_tails_cpu.py asserts it); the
# directed class below reaches R everywhere, so the list is empty.
UNREACHED = []


def required_modes(family, cnt):
    need = vi.required_modes(cnt)
    return need if family == "wide" else [m for m in need if m not in ("const32", "plain32")]


def floor(family, cnt, mode):
    return 1 if (family, cnt, mode) in UNREACHED else R


def _directed_vbyte(rng, nb, n):
    """The directed family of test_v32_inputs_cpu.test_smallest_n_with_compressed_vbyte:
    a base of width b, 11..14 exceptions whose excess has exactly d bits
    (one-byte markers) and one outlier ow bits over the base: compressed vbyte
    at the smallest counts that have it.  At n = 26 that search finds it at
    d = 7 with ow = 15 and at d = 8 with ow = 16, so d and ow are drawn around
    those; the widest value has 3 + 18 bits, inside either family's cap."""
    out = np.zeros((nb, n), dtype=np.uint32)
    for i in range(nb):
        xn, d, b = int(rng.integers(11, min(n, 15))), int(rng.integers(7, 9)), int(rng.choice([0, 3]))
        ow = int(rng.integers(15, 19))
        v = vi._below(rng, (n,), b)
        pos = rng.choice(n, size=xn + 1, replace=False)
        v[pos[:xn]] |= (rng.integers(1 << (d - 1), min(1 << d, 156), size=xn, dtype=np.uint64) << np.uint64(b)).astype(np.uint32)
        v[pos[xn]] = vi._of_width(rng, b + max(ow, d + 1))
        out[i] = v
    return out


def candidates(rng, n, cap):
    """CAND gap rows of n values of every class, at most `cap` bits wide."""
    rows = [np.zeros((CAND, n), np.uint32)]                                                      # zero
    rows.append(np.stack([np.full(n, vi._of_width(rng, int(rng.integers(1, min(cap, 31) + 1)))) for _ in range(CAND)]))  # constant
    if cap == 32:
        rows.append(np.stack([np.full(n, vi._of_width(rng, 32)) for _ in range(CAND)]))          # constant of width 32
        rows.append(vi._below(rng, (CAND, n), 32) | np.uint32(0x80000000))                       # every value 32 bits wide
    rows.append(vi._below(rng, (CAND, n), rng.integers(1, cap + 1, size=(CAND, 1))))             # uniform width w
    for few in (False, True):  # a narrow base with about n / 10 much wider values, or with 1..3 very wide ones
        v = vi._below(rng, (CAND, n), rng.integers(0, 9, size=(CAND, 1)))
        for i in range(CAND):
            k = min(n, int(rng.integers(1, 4))) if few else max(1, n // 10)
            lo = cap - 6 if few else 12
            for p in rng.choice(n, size=k, replace=False):
                v[i, p] = vi._of_width(rng, int(rng.integers(lo, cap + 1)))
        rows.append(v)
    if n >= vi.VB_COMP_MIN_N:
        rows.append(vi.tight_vbyte_blocks(rng, CAND, n) if n < 64 else vi.mixed_vbyte_blocks(rng, CAND, n))
        rows.append(vi.mixed_vbyte_blocks(rng, CAND, n))
        if n < 40:
            rows.append(_directed_vbyte(rng, 4 * CAND, n))
    return np.concatenate(rows) & np.uint32((1 << cap) - 1 if cap < 32 else 0xFFFFFFFF)


def moded_rows(family, cnt):
    """-> {mode: up to R gap rows of cnt values the oracle encodes in that mode}, by bounded seeded rejection."""
    cap = 32 if family == "wide" else CAP_BITS
    rng = np.random.default_rng([7100, FAMILIES.index(family), cnt])
    need = required_modes(family, cnt)
    got = {m: [] for m in need}
    for _ in range(ROUNDS):
        rows = candidates(rng, cnt, cap)
        packed, off = orc.enc32_batch(rows, None)
        for i, row in enumerate(rows):
            mode, _, end = p4_modes.parse32(packed, int(off[i]), cnt)
            assert end == int(off[i + 1])
            if mode in got and len(got[mode]) < R:
                got[mode].append(row)
        if all(len(v) == R for v in got.values()):
            break
    return got


def _front_gaps(rng, cap):
    """The gaps of one full block in front of a tail: those of lists_ref.d1_values(..., outliers=True), capped."""
    v = ref.d1_values(256, 0, rng, outliers=True)
    gaps = np.diff(np.concatenate([[np.uint32(0)], v]).astype(np.uint32)) - np.uint32(1)
    return gaps & np.uint32((1 << cap) - 1 if cap < 32 else 0xFFFFFFFF)


class Family:
    """gaps[j], start0[j]: list j; cnt[j], mode[j], front[j]: its tail count
    (0: an empty list), the mode its tail was chosen for and whether a full
    block precedes the tail.  values(d1), index() and plain(): the lists and the
    oracle's composition of them."""

    def __init__(self, name):
        self.name = name
        cap = 32 if name == "wide" else CAP_BITS
        rng = np.random.default_rng([7200, FAMILIES.index(name)])
        entries = []
        for cnt in COUNTS:
            for mode, rows in moded_rows(name, cnt).items():
                for k, row in enumerate(rows):
                    front = k % 2 == 1
                    entries.append((np.concatenate([_front_gaps(rng, cap), row]) if front else row, cnt, mode, front))
        entries = [entries[i] for i in rng.permutation(len(entries))]
        empty = (np.zeros(0, np.uint32), 0, None, False)
        mid = len(entries) // 2
        entries = [empty] * 2 + entries[:mid] + [empty] * 3 + entries[mid:] + [empty] * 2
        self.gaps = [e[0] for e in entries]
        self.cnt = np.array([e[1] for e in entries])
        self.mode = [e[2] for e in entries]
        self.front = np.array([e[3] for e in entries])
        self.nlists = len(entries)
        self.lens = np.array([len(g) for g in self.gaps])
        self.start0 = rng.integers(0, 1 << (32 if name == "wide" else 31), size=self.nlists, dtype=np.uint64).astype(np.uint32)
        self._d1 = [((np.cumsum(g.astype(np.uint64) + np.uint64(1)) + np.uint64(s)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                    for g, s in zip(self.gaps, self.start0)]

    def values(self, d1):
        return self._d1 if d1 else self.gaps

    @functools.lru_cache(maxsize=None)
    def index(self):
        """The delta-1 index (lists_index.Index)."""
        return li.Index(None, None, start0=self.start0, lists=self._d1)

    @functools.lru_cache(maxsize=None)
    def plain(self):
        """The plain index of the same lengths: .packed, .offs, .ptr, .vals, .base, .lists, .nlists, .nunits."""
        p = collections.namedtuple("Plain", "packed offs ptr vals base lists nlists nunits start0")
        packed, offs, ptr, vals = ref.compose(self.gaps, False)
        return p(packed, offs, ptr, vals, np.asarray(ref.units_loop(ptr)[1], dtype=np.uint32), self.gaps, self.nlists, len(offs) - 1, None)

    def form(self, d1):
        return self.index() if d1 else self.plain()

    def tail_unit(self, base):
        """per list with a tail: (list, its tail's unit in a stream whose directory is `base`)"""
        return [(j, int(base[j + 1]) - 1) for j in range(self.nlists) if self.cnt[j]]

    def tail_start(self, j):
        """the value a delta-1 decode of list j's tail starts from"""
        return int(self._d1[j][255]) if self.front[j] else int(self.start0[j])


@functools.lru_cache(maxsize=None)
def family(name):
    """Cached: callers leave the arrays unchanged."""
    return Family(name)


def census(fam, packed, offs, base):
    """The tail units of a stream of `fam`'s lists, read with p4_modes.parse32:
    every parse ends exactly at the next offset and finds the mode the list was
    chosen for.  -> {(cnt, mode): [tail-only lists, lists with a block in front]}"""
    seen = {}
    for j, u in fam.tail_unit(base):
        cnt = int(fam.cnt[j])
        mode, _, end = p4_modes.parse32(packed, int(offs[u]), cnt)
        assert end == int(offs[u + 1]), (fam.name, j, cnt, mode, end, int(offs[u + 1]))
        assert mode == fam.mode[j], (fam.name, j, cnt, mode, fam.mode[j])
        seen.setdefault((cnt, mode), [0, 0])[int(fam.front[j])] += 1
    return seen


def check_floor(fam, seen):
    """Every required (cnt, mode) meets its floor, in both list shapes where it has two lists.
    -> the smallest count of a group"""
    for cnt in COUNTS:
        for mode in required_modes(fam.name, cnt):
            shapes = seen.get((cnt, mode), [0, 0])
            assert sum(shapes) >= floor(fam.name, cnt, mode), (fam.name, cnt, mode, shapes)
            assert sum(shapes) < 2 or min(shapes) >= 1, (fam.name, cnt, mode, shapes)
    assert set(seen) == {(c, m) for c in COUNTS for m in required_modes(fam.name, c)}
    return min(sum(s) for s in seen.values())
