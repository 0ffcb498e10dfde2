"""The numpy definition of tpf_lists_extract (include/turbopfor_gpu.h): the
selected unit ranges' bytes sliced out of the stream and laid end to end,
their offsets rebased, the directories of the result, its delta-1 starts and
the skip table's entries of the copied units -- and the sliced value lists
the result must decode to.  Also the case matrix the CPU and the GPU tests of
the call share.  Test infrastructure only."""
import numpy as np

import lists_ref as ref

LENS = [0, 1, 255, 256, 257, 513]  # every (ufirst, ucount) of each
BIG = 256 * 17 + 3                 # a sample of its ranges
BIG_RANGES = [(0, 18), (0, 17), (0, 1), (1, 1), (17, 1), (16, 2), (5, 7), (3, 15), (18, 0), (0, 0), (9, 0)]
WRAP = 300                         # a delta-1 list that runs through 2^32
PTR0 = 37                          # d_list_ptr[0] of the source


def table(lists):
    """The skip table by its definition: the last value of every unit."""
    return np.array([v[min(256 * (i + 1), len(v)) - 1] for v in lists for i in range(ref.n_units(len(v)))], dtype=np.uint32)


class Source:
    """An index: the oracle's composition of `lists` (tests/lists_ref.py), its unit directory and, with d1, the skip table."""

    def __init__(self, lists, d1, start0=None, ptr0=PTR0):
        self.d1, self.lists, self.start0 = d1, lists, start0 if d1 else None
        self.packed, self.offs, self.ptr, _ = ref.compose(lists, d1, self.start0, ptr0=ptr0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.nlists, self.nunits = len(lists), len(self.offs) - 1
        self.table = table(lists) if d1 else None

    def s0(self, j):
        return int(self.start0[j]) if self.start0 is not None else 0


class Result:
    pass


def ranges(n):
    """every (ufirst, ucount) inside a list of n values, the empty ones included"""
    units = ref.n_units(n)
    return [(a, c) for a in range(units + 1) for c in range(units - a + 1)]


def whole(src, sel):
    return [0] * len(sel), [ref.n_units(len(src.lists[j])) for j in sel]


def extract(src, sel, ufirst=None, ucount=None, d1=None, start_mutant=False, rebase=True):
    """The definition.  src: a Source, or a lists_index.Index (a delta-1
    stream); sel / ufirst / ucount: sequences (ufirst None: whole lists).
    d1: default src.d1 (True for an Index).  -> a Result: packed, offs, ptr,
    base (d_list_unit_out), start0 (None without d1), table (None without d1),
    lists (the sliced values).  The two mutants are the mistakes the matrix
    must tell from the definition: a start taken from start0[j] at ufirst > 0,
    and offsets that keep their source values."""
    if d1 is None:
        d1 = getattr(src, "d1", True)
    if ufirst is None:
        ufirst, ucount = whole(src, sel)
    start0 = getattr(src, "start0", None) if d1 else None
    parts, offs, ptr, base, st, tab, lists, at = [], [0], [0], [0], [], [], [], 0
    for j, a, c in zip(sel, ufirst, ucount):
        j, a, c = int(j), int(a), int(c)
        v = src.lists[j]
        assert a + c <= ref.n_units(len(v))
        u0 = int(src.base[j]) + a
        b0, b1 = int(src.offs[u0]), int(src.offs[u0 + c])
        parts.append(src.packed[b0:b1])
        shift = at - b0 if rebase else 0
        offs += [int(o) + shift for o in src.offs[u0 + 1: u0 + c + 1]]
        at += b1 - b0
        lists.append(v[256 * a: min(256 * (a + c), len(v))])
        ptr.append(ptr[-1] + len(lists[-1]))
        base.append(base[-1] + c)
        if d1:
            s0 = int(start0[j]) if start0 is not None else 0
            st.append(s0 if a == 0 or start_mutant else int(src.table[u0 - 1]))
            tab += [int(x) for x in src.table[u0: u0 + c]]
    r = Result()
    r.packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    r.offs, r.ptr = np.asarray(offs, dtype=np.uint64), np.asarray(ptr, dtype=np.uint64)
    r.base = np.asarray(base, dtype=np.uint32)
    r.start0 = np.asarray(st, dtype=np.uint32) if d1 else None
    r.table = np.asarray(tab, dtype=np.uint32) if d1 else None
    r.lists, r.nunits, r.nlists, r.d1 = lists, len(offs) - 1, len(lists), d1
    return r


def values(n, d1, s0, rng):
    return ref.d1_values(n, int(s0), rng, outliers=True) if d1 else ref.plain_values(n, rng)


def matrix_source(d1, st=True, seed=2207):
    """The lists of the matrix: LENS twice (the second set after BIG), BIG and,
    last, the list that wraps 2^32 (delta-1 with starts) -- mixed gap widths
    and outlier rates, so some blocks carry vbyte exceptions and some bitmaps."""
    rng = np.random.default_rng(seed + 2 * d1 + st)
    lens = LENS + [BIG] + LENS[::-1] + [WRAP]
    start0 = rng.integers(0, 1 << 31, size=len(lens), dtype=np.uint64).astype(np.uint32) if (d1 and st) else None
    if start0 is not None:
        start0[-1] = (1 << 32) - 1000
    lists = [values(n, d1, start0[j] if start0 is not None else 0, rng) for j, n in enumerate(lens)]
    if start0 is not None:
        assert int(lists[-1][0]) > int(lists[-1][-1])  # it wraps
    return Source(lists, d1, start0)


def matrix_selection(src, seed=11):
    """(sel, ufirst, ucount): every range of every list of at most 513 values, the sample of BIG's, in a seeded order."""
    rows = []
    for j, v in enumerate(src.lists):
        rows += [(j, a, c) for a, c in (BIG_RANGES if len(v) == BIG else ranges(len(v)))]
    rows = [rows[i] for i in np.random.default_rng(seed).permutation(len(rows))]
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
