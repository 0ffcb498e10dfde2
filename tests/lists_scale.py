"""Indexes of many lists without one oracle call per list, and whole-request
numpy statements of what the lists entry points return, for the tests that
cross the launch caps (tests/test_gpu_lists_scale.py).

A list's stream depends only on its values and its start0, so an index of N
lists is a seeded choice out of a dictionary of a few dozen KINDS, each
composed once by the oracle (tests/lists_ref.py) for delta-1 and once for
plain; every field of the index is a numpy concatenation of the per-kind pieces
with the offsets shifted.  tests/test_lists_scale_cpu.py holds the construction
against lists_ref.compose plus lists_index.Index field for field, and the
vectorised statements against the per-query ones of the small GPU tests.  Test
infrastructure only."""
import numpy as np

import lists_ref as ref

BIG_LENS = [255, 256, 257, 513, 256 * 17 + 3]  # around one unit, three units, a tail after the 16-unit decode run


def gather_segments(pool, start, length):
    """pool[start[i]: start[i] + length[i]] for every i, laid end to end"""
    length = np.asarray(length, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    at = np.cumsum(length) - length
    idx = np.arange(int(length.sum()), dtype=np.int64) + np.repeat(start - at, length)
    return pool[idx]


def _starts(counts):
    """exclusive prefix of counts, with the total appended"""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])


class Kinds:
    """The dictionary: kind i is (values[i], start0[i]); the delta-1 kinds
    ascend without wrapping (start0 < 2^31, gaps below 2^14, at most 4,355
    values).  Lengths: `empties` of 0, `variants` each of 1, 2 and 3, one each
    of BIG_LENS."""

    def __init__(self, rng, empties=2, variants=8):
        lens = [0] * empties + [n for n in (1, 2, 3) for _ in range(variants)] + BIG_LENS
        self.lens = np.asarray(lens, dtype=np.int64)
        self.units = self.lens // 256 + (self.lens % 256 != 0)
        self.start0 = rng.integers(0, 1 << 31, size=len(lens), dtype=np.uint64).astype(np.uint32)
        self.values = [ref.d1_values(n, int(s), rng) for n, s in zip(lens, self.start0)]
        assert all(len(v) == 0 or (int(v[0]) > int(s) and (np.diff(v.astype(np.int64)) > 0).all()) for v, s in zip(self.values, self.start0))
        self.vpool = np.concatenate(self.values)
        self.voff = _starts(self.lens)[:-1]
        # the definition of the skip table: the last value of every unit
        self.tpool = np.array([v[min(256 * (i + 1), len(v)) - 1] for v in self.values for i in range(ref.n_units(len(v)))], dtype=np.uint32)
        self.uoff = _starts(self.units)[:-1]
        self._streams = {}

    def streams(self, d1):
        """-> (bytes of every kind's stream end to end, where kind i's begin, their lengths, every unit's offset inside its
        kind's stream -- indexed as tpool is)"""
        if d1 not in self._streams:
            packed, urel = [], []
            for v, s in zip(self.values, self.start0):
                p, o, _, _ = ref.compose([v], d1, [s])
                assert len(o) == ref.n_units(len(v)) + 1 and int(o[-1]) == len(p)
                packed.append(p)
                urel.append(o[:-1])
            blen = np.asarray([len(p) for p in packed], dtype=np.int64)
            self._streams[d1] = (np.concatenate(packed), _starts(blen)[:-1], blen, np.concatenate(urel).astype(np.int64))
        return self._streams[d1]

    def choose(self, rng, n, empty=0.1, big=0.004):
        """n kinds: `empty` of them of length 0, `big` of them out of BIG_LENS, the rest of 1 to 3 values; every kind occurs"""
        nbig = len(BIG_LENS)
        small = np.nonzero((self.lens > 0) & (self.lens <= 3))[0]
        empties = np.nonzero(self.lens == 0)[0]
        r = rng.random(n)
        k = small[rng.integers(0, len(small), size=n)]
        k = np.where(r < empty, empties[rng.integers(0, len(empties), size=n)], k)
        k = np.where(r > 1.0 - big, len(self.lens) - nbig + rng.integers(0, nbig, size=n), k)
        k[rng.permutation(n)[:len(self.lens)]] = np.arange(len(self.lens))
        return k


class ScaleIndex:
    """An index of len(kind_of) lists out of `kinds`: the fields of
    lists_index.Index (ptr, base, start0, vals, table, lens, nlists, nunits),
    and per stream form its packed bytes and unit offsets."""

    def __init__(self, kinds, kind_of, ptr0=0):
        k = np.asarray(kind_of, dtype=np.int64)
        self.kinds, self.kind_of = kinds, k
        self.nlists = len(k)
        self.lens = kinds.lens[k]
        self.ptr = (ptr0 + _starts(self.lens)).astype(np.uint64)
        self.units = kinds.units[k]
        self.base = _starts(self.units).astype(np.uint32)
        self.nunits = int(self.base[-1])
        self.start0 = kinds.start0[k]
        self.vals = gather_segments(kinds.vpool, kinds.voff[k], self.lens)
        self.table = gather_segments(kinds.tpool, kinds.uoff[k], self.units)
        self._streams = {}

    def stream(self, d1):
        """-> (packed u8, offsets u64 [nunits + 1])"""
        if d1 not in self._streams:
            pool, boff, blen, urel = self.kinds.streams(d1)
            k = self.kind_of
            packed = gather_segments(pool, boff[k], blen[k])
            at = _starts(blen[k])
            offs = np.concatenate([np.repeat(at[:-1], self.units) + gather_segments(urel, self.kinds.uoff[k], self.units), at[-1:]])
            self._streams[d1] = (packed, offs.astype(np.uint64))
        return self._streams[d1]


class Twin:
    """The plain stream of the same list lengths as the delta-1 lists_index.Index
    `ix` (the term frequencies of its doc ids): one directory serves both."""

    def __init__(self, ix, rng):
        self.ix = ix
        self.freqs = [ref.plain_values(n, rng) for n in ix.lens]
        self.fpacked, self.foffs, fptr, self.fvals = ref.compose(self.freqs, False, ptr0=int(ix.ptr[0]))
        assert np.array_equal(fptr, ix.ptr) and len(self.foffs) == len(ix.offs)

    def stream(self, d1):
        """-> (packed, offsets, every value of the index end to end)"""
        return (self.ix.packed, self.ix.offs, self.ix.vals) if d1 else (self.fpacked, self.foffs, self.fvals)


# ---- whole-request statements of the definitions (include/turbopfor_gpu.h) ---------------------
# `ix`: anything with ptr, base, table, vals, nlists (ScaleIndex, lists_index.Index).

def rel(ix):
    """where every list begins in ix.vals, nlists + 1 entries"""
    return (np.asarray(ix.ptr, dtype=np.uint64) - np.uint64(ix.ptr[0])).astype(np.int64)


def _keys(lists, values):
    return (np.asarray(lists, dtype=np.uint64) << np.uint64(32)) | np.asarray(values, dtype=np.uint32).astype(np.uint64)


def value_keys(ix):
    """(list << 32) | value of every value of an index whose lists ascend: ascending as a whole"""
    keys = _keys(np.repeat(np.arange(ix.nlists), np.diff(rel(ix))), ix.vals)
    assert (keys[1:] > keys[:-1]).all()
    return keys


def tail_units(ix):
    """per unit of the stream: it is its list's p4Enc32 tail"""
    r = rel(ix)
    t = np.zeros(int(ix.base[-1]), dtype=bool)
    t[ix.base[1:].astype(np.int64)[np.diff(r) % 256 != 0] - 1] = True
    return t


def want_select(ix, sel):
    """tpf_p4ndec256v32_lists_select: -> (values, out_ptr)"""
    r = rel(ix)
    sel = np.asarray(sel, dtype=np.int64)
    n = np.diff(r)[sel]
    return gather_segments(ix.vals, r[sel], n), _starts(n)


def want_units(ix, sel, ufirst, ucount):
    """tpf_p4ndec256v32_lists_units for ranges inside their lists: -> (values, out_ptr)"""
    r = rel(ix)
    sel, uf, uc = (np.asarray(x, dtype=np.int64) for x in (sel, ufirst, ucount))
    n = np.diff(r)[sel]
    count = np.where(uc > 0, np.minimum(256 * (uf + uc), n) - 256 * uf, 0)
    return gather_segments(ix.vals, r[sel] + 256 * uf, count), _starts(count)


def want_range(ix, qlist, qlo, qhi):
    """tpf_lists_range_units for lists that ascend: the first unit of the list
    whose last value is >= lo, through the first whose last value is >= hi or
    the list's last unit; (0, 0) when lo > hi, the list is empty or every value
    lies below lo.  -> (ufirst, ucount)"""
    qlist, lo, hi = (np.asarray(x, dtype=np.int64) for x in (qlist, qlo, qhi))
    base = ix.base.astype(np.int64)
    ua, ub = base[qlist], base[qlist + 1]
    tkeys = _keys(np.repeat(np.arange(ix.nlists), np.diff(base)), ix.table)
    assert (tkeys[1:] > tkeys[:-1]).all()
    a = np.searchsorted(tkeys, _keys(qlist, lo))  # in [ua, ub]: the keys of the lists before qlist are smaller, those after larger
    b = np.minimum(np.searchsorted(tkeys, _keys(qlist, hi)), ub - 1)
    some = (lo <= hi) & (a < ub)
    return np.where(some, a - ua, 0).astype(np.uint32), np.where(some, b - a + 1, 0).astype(np.uint32)


def probe_units(ix, lists, values):
    """The unit of the stream every probe value lands in -- the first unit of its
    list whose last value is >= the value -- or -1 past the list's last value."""
    lists = np.asarray(lists, dtype=np.int64)
    base = ix.base.astype(np.int64)
    tkeys = _keys(np.repeat(np.arange(ix.nlists), np.diff(base)), ix.table)
    a = np.searchsorted(tkeys, _keys(lists, values))
    return np.where(a < base[lists + 1], a, -1)


def item_heads(lists, units):
    """Indices that head an item: a request index naming a unit (units >= 0)
    whose predecessor names another unit or another list."""
    lists, units = np.asarray(lists, dtype=np.int64), np.asarray(units, dtype=np.int64)
    head = units >= 0
    head[1:] &= (units[1:] != units[:-1]) | (lists[1:] != lists[:-1])
    return np.nonzero(head)[0]


def want_hits(ix, qlist, probe_ptr, probe):
    """tpf_lists_intersect for an index whose lists ascend, the whole probe at
    once: a probe value is a hit iff (list << 32) | value is a key of the
    index, at the position np.searchsorted finds.  probe_ptr: int64 [nq + 1].
    -> (values, out_ptr, pidx, tpos)"""
    keys, r = value_keys(ix), rel(ix)
    pp = np.asarray(probe_ptr, dtype=np.int64)
    a, b = int(pp[0]), int(pp[-1])
    ql = np.repeat(np.asarray(qlist, dtype=np.int64), np.diff(pp))
    pv = np.asarray(probe, dtype=np.uint32)[a:b]
    pk = _keys(ql, pv)
    hit = np.isin(pk, keys)
    tpos = np.searchsorted(keys, pk[hit]) - r[ql[hit]]
    out_ptr = _starts(hit)[pp - a]
    return pv[hit], out_ptr, (a + np.nonzero(hit)[0]).astype(np.uint32), tpos.astype(np.uint32)


def want_gather(ix_ptr, values, qlist, pos_ptr, pos):
    """tpf_lists_gather for positions inside their lists: values[ptr[list] + pos] for the request indices of the segments"""
    r = (np.asarray(ix_ptr, dtype=np.uint64) - np.uint64(ix_ptr[0])).astype(np.int64)
    pp = np.asarray(pos_ptr, dtype=np.int64)
    ql = np.repeat(np.asarray(qlist, dtype=np.int64), np.diff(pp))
    return values[r[ql] + np.asarray(pos, dtype=np.int64)[int(pp[0]): int(pp[-1])]]
