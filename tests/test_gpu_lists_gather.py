"""GPU checks of the positional read of a resident index
(include/turbopfor_gpu.h tpf_lists_gather): list-relative positions, as CSR
segments with one target list each, against a delta-1 lists stream with its
skip table and against the plain stream of the same list lengths stored in
parallel with it.  The streams are the oracle's composition (tests/lists_ref.py,
the delta-1 one through tests/lists_index.py); the expected values are slices
of the original numpy lists -- lists[j][pos] -- never the code under test."""
import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
from lists_index import CLEAN, DEV, SENT, Index

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SMALL = [300, 0, 612, 256, 90, 0, 256 * 17]
PTR0 = 3    # request entries before the first segment ...
TRAIL = 5   # ... and after the last: positions past every list, never to be read (a read would be reported)
OUTSIDE = 0xFFFFFFFF


class Pair:
    """A delta-1 index and the plain stream of the same list lengths (the term frequencies of its doc ids)."""

    def __init__(self, ix, rng):
        self.ix = ix
        self.freqs = [ref.plain_values(n, rng) for n in ix.lens]
        self.fpacked, self.foffs, fptr, _ = ref.compose(self.freqs, False, ptr0=int(ix.ptr[0]))
        # one directory serves both streams
        assert np.array_equal(fptr, ix.ptr) and len(self.foffs) == len(ix.offs)

    def stream(self, d1):
        """-> (packed, offsets, the original lists)"""
        return (self.ix.packed, self.ix.offs, self.ix.lists) if d1 else (self.fpacked, self.foffs, self.freqs)


@pytest.fixture(scope="module")
def pairs():
    """[the shape matrix permuted, SMALL]"""
    rng = np.random.default_rng(117)
    lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
    return [Pair(Index(lens, rng, ptr0=37, start_bits=31), rng), Pair(Index(SMALL, rng, ptr0=11, start_bits=31), rng)]


def _run(pr, queries, d1, shift=0, table=None, offs=None, base=None, pos_ptr=None, qlist=None, ptr0=PTR0):
    """Read queries [(list, positions)] from `pr` in one call.  The request
    lies between ptr0 leading and TRAIL trailing entries that name no position
    of any list; d_out is sentinel-guarded, 4 bytes past a 16-byte boundary."""
    ix = pr.ix
    packed, soffs, _ = pr.stream(d1)
    segs = [np.asarray(p, dtype=np.uint32) for _, p in queries]
    pos = np.concatenate([np.full(ptr0, OUTSIDE, np.uint32)] + segs + [np.full(TRAIL, OUTSIDE, np.uint32)])
    pp = ptr0 + np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    out = li.Guarded32(torch, len(pos))
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tbl = None if (table is None and not d1) else li.dev32(torch, ix.table if table is None else table)
    tpf.lists_gather(li.dev8(torch, packed, shift), li.dev64(torch, soffs if offs is None else offs), li.dev64(torch, ix.ptr),
                     li.dev32(torch, ix.base if base is None else base), li.dev32(torch, pos),
                     li.dev64(torch, pp if pos_ptr is None else pos_ptr), li.dev32(torch, [j for j, _ in queries] if qlist is None else qlist),
                     d1=d1, start0=li.dev32(torch, ix.start0) if d1 else None, unit_last=tbl, out=out.view, err=err)
    got, ok = out.read()
    assert ok, "a value outside d_out was written"
    return dict(err=int(err.item()), out=got, pp=pp, pos=pos)


def _want(pr, queries, d1):
    src = pr.stream(d1)[2]
    parts = [src[j][np.asarray(p, dtype=np.int64)] for j, p in queries if len(p)]
    return np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)


def _check(pr, queries, r, d1):
    assert r["err"] == CLEAN
    a, b = int(r["pp"][0]), int(r["pp"][-1])
    want = _want(pr, queries, d1)
    assert len(want) == b - a
    assert np.array_equal(r["out"][a:b], want)
    # parallel to d_pos: nothing before the first segment or after the last
    assert (r["out"][:a] == SENT).all() and (r["out"][b:] == SENT).all()
    return len(want)


def _untouched(r):
    assert (r["out"] == SENT).all()


# ---- 1. the edges of the definition ---------------------------------------------------
def _edge_positions(n):
    if n == 0:
        return np.zeros(0, np.uint32)
    marks = {0, n - 1}
    bounds = list(range(1, (n - 1) // 256 + 1))  # 256 * i <= n - 1: a position on either side exists
    for i in ([bounds[0], bounds[len(bounds) // 2], bounds[-1]] if bounds else []):
        marks |= {256 * i - 1, 256 * i, 256 * i + 1}
    return np.array(sorted(m for m in marks if 0 <= m < n), dtype=np.uint32)


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("d1", [True, False])
def test_edges_of_the_definition(pairs, d1, shift):
    for pr in pairs:
        queries = [(j, _edge_positions(pr.ix.lens[j])) for j in range(pr.ix.nlists)]
        n = _check(pr, queries, _run(pr, queries, d1, shift=shift), d1)
        assert n >= 2 * sum(1 for x in pr.ix.lens if x > 1)
    mx = pairs[0].ix
    assert {0, 5, 256, 256 * 17 + 3} <= set(mx.lens)  # an empty target, a tail-only list, exactly one full block, a tail after full blocks
    assert _edge_positions(256 * 17 + 3).tolist()[-4:] == [256 * 17 - 1, 256 * 17, 256 * 17 + 1, 256 * 17 + 2]
    assert _edge_positions(256).tolist() == [0, 255] and _edge_positions(257).tolist() == [0, 255, 256]


# ---- 2. every position of two lists ---------------------------------------------------
@pytest.mark.parametrize("d1", [True, False])
def test_every_position_equals_the_full_decode(pairs, d1):
    pr = pairs[0]
    ix = pr.ix
    a, b = ix.of_len(256 * 64 + 1), ix.of_len(256 * 130 + 77)
    queries = [(a, np.arange(ix.lens[a])), (b, np.arange(ix.lens[b]))]
    r = _run(pr, queries, d1)
    assert _check(pr, queries, r, d1) == ix.lens[a] + ix.lens[b]
    # ... and bit for bit what the many-lists decode writes at ptr[j] + p
    packed, offs, _ = pr.stream(d1)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    full = tpf.decn256v32_lists(li.dev8(torch, packed), li.dev64(torch, offs), li.dev64(torch, ix.ptr), d1=d1,
                                start0=li.dev32(torch, ix.start0) if d1 else None,
                                out=torch.zeros(int(ix.ptr[-1]), dtype=torch.int32, device=DEV), err=err)
    assert int(err.item()) == CLEAN
    full = full.cpu().numpy().view(np.uint32)
    at = PTR0
    for j in (a, b):
        assert np.array_equal(r["out"][at: at + ix.lens[j]], full[int(ix.ptr[j]): int(ix.ptr[j + 1])])
        at += ix.lens[j]


# ---- 3. segment lengths ----------------------------------------------------------------
@pytest.mark.parametrize("d1", [True, False])
def test_segment_lengths(pairs, d1):
    pr = pairs[0]
    ix = pr.ix
    rng = np.random.default_rng(67)
    j, other = ix.of_len(256 * 17 + 3), ix.of_len(513)
    queries = []
    for m in (1, 63, 64, 65, 257):
        p = np.sort(rng.integers(256 * 5, 256 * 6, size=m))  # inside unit 5; 257 positions of 256 repeat at least one
        queries += [(j, p), (other, np.sort(rng.integers(0, 513, size=3)))]  # another list in between: the segments stay separate items
    queries.append((j, np.arange(256 * 5, 256 * 6)))
    queries.append((j, np.arange(256 * 5 + 100, 256 * 6)))  # the next segment names the same list and unit: one item across two queries
    _check(pr, queries, _run(pr, queries, d1), d1)


# ---- 4. more positions than one scan tile covers -----------------------------------------
@pytest.mark.parametrize("d1", [True, False])
def test_positions_past_one_scan_tile(pairs, d1):
    """More than 64 * 4,096 request indices: the run scan over the 64-index runs takes its two-launch form."""
    pr = pairs[0]
    ix = pr.ix
    j, other = ix.of_len(256 * 130 + 77), ix.of_len(257)
    n = ix.lens[j]
    total = 263000
    strided = np.arange(total, dtype=np.int64) * n // total  # every position of the long list, about 8 times each, in order
    assert strided[0] == 0 and strided[-1] == n - 1
    queries = [(other, np.arange(0, 257, 3)), (j, strided), (j, np.arange(n - 300, n))]
    assert PTR0 + sum(len(p) for _, p in queries) > 64 * 4096
    assert _check(pr, queries, _run(pr, queries, d1), d1) == 86 + total + 300


# ---- 5. many small queries -------------------------------------------------------------
@pytest.mark.parametrize("d1", [True, False])
def test_many_small_queries(pairs, d1):
    """150 queries of 0 to 40 positions: the item runs span many queries, the tails kernel many waves."""
    pr = pairs[0]
    ix = pr.ix
    rng = np.random.default_rng(43)
    queries, tails = [], 0
    for _ in range(150):
        j = int(rng.integers(0, ix.nlists))
        n = ix.lens[j]
        m = int(rng.integers(0, 41)) if n else 0
        p = np.sort(rng.integers(0, max(n, 1), size=m))
        if m and n % 256 and rng.random() < 0.4:
            p[-1] = n - 1 - int(rng.integers(0, n % 256))  # into the list's tail unit
            p = np.sort(p)
        queries.append((j, p))
        tails += bool(n % 256 and len(p) and int(p[-1]) >= 256 * (n // 256))
    assert tails >= 10
    assert min(len(p) for _, p in queries) == 0 and max(len(p) for _, p in queries) == 40
    _check(pr, queries, _run(pr, queries, d1), d1)


# ---- 6. unsorted positions with repeats ----------------------------------------------------
@pytest.mark.parametrize("d1", [True, False])
def test_unsorted_positions_with_repeats(pairs, d1):
    pr = pairs[0]
    ix = pr.ix
    rng = np.random.default_rng(71)
    queries = []
    for j in (ix.of_len(256 * 17 + 3), ix.of_len(257), ix.of_len(256 * 64)):
        p = rng.integers(0, ix.lens[j], size=90)
        p = np.concatenate([p, p[rng.permutation(90)[:30]], p[:5]])
        queries.append((j, p[rng.permutation(len(p))]))
    for _, p in queries:
        assert len(np.unique(p)) < len(p) and (np.diff(p.astype(np.int64)) < 0).any()
    n = _check(pr, queries, _run(pr, queries, d1), d1)  # exact, every occurrence answered
    assert n == 3 * 125


# ---- 7. blocks of every exception kind -------------------------------------------------------
def _kinds_lists(rng, lens, start0):
    """per 256-value block a gap width of 1..7 bits and an outlier rate; outlier gaps of 9..14 bits
    (the shape of test_gpu_lists_intersect.py's index of the same name)"""
    lists = []
    for n, s in zip(lens, start0):
        nb = n // 256 + 1
        bw = rng.integers(1, 8, size=nb).repeat(256)[:n].astype(np.uint64)
        rate = rng.choice([0, .005, .03, .1, .3], size=nb).repeat(256)[:n]
        raw = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
        gaps = (raw & ((np.uint64(1) << bw) - np.uint64(1))) + np.uint64(1)
        hit = rng.random(n) < rate
        big = rng.integers(9, 15, size=n).astype(np.uint64)
        gaps[hit] = ((rng.integers(0, 1 << 62, size=n, dtype=np.uint64) & ((np.uint64(1) << big) - np.uint64(1))) + np.uint64(1))[hit]
        lists.append((np.cumsum(gaps) + np.uint64(s)).astype(np.uint32))
    return lists


def test_every_exception_kind():
    rng = np.random.default_rng(10)
    lens = [256 * 70 + 130, 5, 256 * 3, 256 * 33 + 1, 0, 200, 256 * 18 + 255]
    start0 = rng.integers(0, 1 << 31, size=len(lens), dtype=np.uint64).astype(np.uint32)
    ix = Index(None, rng, ptr0=2, start0=start0, lists=_kinds_lists(rng, lens, start0))
    kinds = ref.block_kinds(ix.packed, ix.offs, ix.ptr - ix.ptr[0])
    assert kinds["vbyte"] >= 5 and kinds["bitmap"] >= 5 and kinds["plain"] >= 5, kinds
    pr = Pair(ix, rng)
    queries = []
    for j in range(ix.nlists):
        n = ix.lens[j]
        p = [256 * u + np.sort(rng.permutation(min(256, n - 256 * u))[:3]) for u in range(ix.units(j))]  # three positions per unit
        queries.append((j, np.concatenate(p + [np.zeros(0, np.int64)])))
    asked = sum(len(p) for _, p in queries)
    assert asked >= 3 * (ix.nunits - 1)  # the one-value tail of the 33-block list has no three
    for d1 in (True, False):
        assert _check(pr, queries, _run(pr, queries, d1), d1) == asked


# ---- 8. chained with the intersection, on the device -------------------------------------------
def test_chained_with_the_intersection():
    rng = np.random.default_rng(73)
    common = np.unique(rng.integers(1, 1 << 28, size=3000, dtype=np.uint64))
    lists = [np.unique(np.concatenate([common, rng.integers(1, 1 << 28, size=n, dtype=np.uint64)])).astype(np.uint32)
             for n in (5000, 9000)]
    pr = Pair(Index(None, rng, ptr0=7, start0=np.zeros(2, np.uint32), lists=lists), rng)
    ix = pr.ix
    assert ix.ascends()
    hits = np.intersect1d(lists[0], lists[1])
    assert len(common) <= len(hits) < len(lists[0])
    ptr, base, table, st = li.dev64(torch, ix.ptr), li.dev32(torch, ix.base), li.dev32(torch, ix.table), li.dev32(torch, ix.start0)
    packed, offs = li.dev8(torch, ix.packed), li.dev64(torch, ix.offs)
    fpacked, foffs = li.dev8(torch, pr.fpacked), li.dev64(torch, pr.foffs)
    n0 = len(lists[0])
    qlist = li.dev32(torch, [1])
    err = torch.zeros(3, dtype=torch.int64, device=DEV)
    tpos = torch.full((n0,), -1, dtype=torch.int32, device=DEV)  # entries past the hits stay out of range: never read
    _, out_ptr = tpf.lists_intersect(packed, offs, ptr, base, table, li.dev32(torch, lists[0]), li.dev64(torch, [0, n0]), qlist,
                                     start0=st, tpos=tpos, err=err[0:1])
    # (tpos, out_ptr, qlist) unchanged, nothing read back in between
    fr = tpf.lists_gather(fpacked, foffs, ptr, base, tpos, out_ptr, qlist, d1=False, err=err[1:2])
    ids = tpf.lists_gather(packed, offs, ptr, base, tpos, out_ptr, qlist, d1=True, start0=st, unit_last=table, err=err[2:3])
    assert err.tolist() == [CLEAN, CLEAN, CLEAN]
    assert out_ptr.tolist() == [0, len(hits)]
    n = len(hits)
    assert np.array_equal(fr.cpu().numpy().view(np.uint32)[:n], pr.freqs[1][np.searchsorted(lists[1], hits)])
    assert np.array_equal(ids.cpu().numpy().view(np.uint32)[:n], hits)


# ---- 9. refusals ------------------------------------------------------------------------------
def _eight(ix, rng):
    """8 queries over SMALL, 10 sorted positions each (none for the empty list); query 3 is the only one that names list 6"""
    return [(j, np.sort(rng.integers(0, ix.lens[j], size=10)) if ix.lens[j] else np.zeros(0, np.int64)) for j in (0, 2, 3, 6, 4, 1, 2, 0)]


@pytest.mark.parametrize("d1", [True, False])
@pytest.mark.parametrize("what", ["nlists", "ffffffff", "descending", "past_pos", "past_pos_last", "directory"])
def test_refused_query(pairs, what, d1):
    pr = pairs[1]
    ix = pr.ix
    queries = _eight(ix, np.random.default_rng(79))
    lens = [len(p) for _, p in queries]
    pp = PTR0 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos_values = PTR0 + sum(lens) + TRAIL
    qlist = [j for j, _ in queries]
    kw, k = {}, 3
    if what == "nlists":
        qlist[3] = ix.nlists
        kw = dict(qlist=qlist)
    elif what == "ffffffff":
        qlist[3] = 0xFFFFFFFF
        kw = dict(qlist=qlist)
    elif what == "descending":
        pp[4] = pp[3] - 1
        kw = dict(pos_ptr=pp)
    elif what == "past_pos":
        pp[4] = pos_values + 1
        kw = dict(pos_ptr=pp)
    elif what == "past_pos_last":
        pp[8] = pos_values + 1  # pos_ptr[nq]: the last query's end
        kw, k = dict(pos_ptr=pp), 7
    else:
        base = ix.base.copy()
        assert base[7] == ix.nunits
        base[7] = ix.nunits + 1
        kw = dict(base=base)
    r = _run(pr, queries, d1, **kw)
    assert r["err"] == ix.nunits + k
    _untouched(r)


@pytest.mark.parametrize("d1", [True, False])
def test_refused_position(pairs, d1):
    pr = pairs[1]
    ix = pr.ix
    nq = 8

    def run(edits, **kw):
        queries = [(j, p.copy()) for j, p in _eight(ix, np.random.default_rng(79))]
        for k, at, v in edits:
            queries[k][1][at] = v
        r = _run(pr, queries, d1, **kw)
        _untouched(r)
        return r["err"], [int(x) for x in r["pp"]]

    err, pp = run([(3, 9, ix.lens[6])])  # one past the list's last position
    assert err == ix.nunits + nq + pp[3] + 9
    err, pp = run([(1, 4, 0xFFFFFFFF)])
    assert err == ix.nunits + nq + pp[1] + 4
    err, pp = run([(6, 2, ix.lens[2]), (2, 0, 256), (7, 9, 0xFFFFFFFF)])  # the lowest request index of three
    assert err == ix.nunits + nq + pp[2]
    # a refused query together with a bad position before it: the query's code
    qlist = [0, 2, 3, 6, 4, ix.nlists, 2, 0]
    err, _ = run([(0, 0, ix.lens[0])], qlist=qlist)
    assert err == ix.nunits + 5


def test_nq_zero(pairs):
    for d1 in (True, False):
        r = _run(pairs[1], [], d1)
        assert r["err"] == CLEAN
        _untouched(r)


# ---- 10. a corrupted block is reported only when a position names it -----------------------------
@pytest.mark.parametrize("d1", [True, False])
@pytest.mark.parametrize("tail", [False, True])
def test_corrupted_block(pairs, tail, d1):
    pr = pairs[1]
    ix = pr.ix
    j, i = (2, 2) if tail else (6, 9)  # the tail of the 612-value list; unit 9 of the 17-unit list
    u = int(ix.base[j]) + i
    offs = pr.stream(d1)[1].copy()
    offs[u + 1] += 1  # its end offset, the start of the unit after it, moves by one
    far = np.concatenate([np.arange(0, 200), np.arange(256, 306)] if tail else [np.arange(256 * 2, 256 * 2 + 40), np.arange(256 * 12, 256 * 14, 7)])
    others = [(0, np.arange(5, 290, 31)), (4, np.arange(0, 90, 9))]  # not list 3: its unit follows the 612-value list's tail
    into = np.sort(np.concatenate([far, 256 * i + np.arange(3, 6)]))
    assert _run(pr, others + [(j, into)], d1, offs=offs)["err"] == u
    # no position in that unit or in the one after it: clean and exact
    queries = others + [(j, far)]
    _check(pr, queries, _run(pr, queries, d1, offs=offs), d1)


# ---- 11. a wrong table is harmless, and what it does is determined -------------------------------
def test_wrong_table(pairs):
    pr = pairs[0]
    ix = pr.ix
    rng = np.random.default_rng(89)
    queries = [(j, np.sort(rng.integers(0, ix.lens[j], size=80))) for j in range(ix.nlists) if ix.lens[j]]
    bogus = np.full(ix.nunits, 0xFFFFFFFF, np.uint32)
    r = _run(pr, queries, True, table=bogus)  # _run asserts the guards
    assert r["err"] == CLEAN
    pos = np.concatenate([p for _, p in queries])
    a, b = int(r["pp"][0]), int(r["pp"][-1])
    first = pos < 256
    assert first.sum() > 100 and (~first).sum() > 100
    # the first unit of a list starts from start0, whatever the table holds
    assert np.array_equal(r["out"][a:b][first], _want(pr, queries, True)[first])
    assert (r["out"][:a] == SENT).all() and (r["out"][b:] == SENT).all()
    # the plain form ignores the table
    _check(pr, queries, _run(pr, queries, False, table=bogus), False)


# ---- 12. the work does not depend on the rest of the index -----------------------------------------
def test_index_independence(pairs):
    pr = pairs[1]
    ix = pr.ix
    rng = np.random.default_rng(53)
    more_len = [int(n) for n in rng.integers(0, 300, size=1000)]
    more_s0 = rng.integers(0, 1 << 31, size=1000, dtype=np.uint64).astype(np.uint32)
    more = [ref.d1_values(n, int(s), rng) for n, s in zip(more_len, more_s0)]
    grown = Pair(Index(None, rng, ptr0=11, start0=np.concatenate([ix.start0, more_s0]), lists=ix.lists + more), rng)
    grown.freqs[:ix.nlists] = pr.freqs  # the same frequencies for the lists the two share
    grown.fpacked, grown.foffs, _, _ = ref.compose(grown.freqs, False, ptr0=11)
    queries = _eight(ix, np.random.default_rng(79))
    for d1 in (True, False):
        a, b = _run(pr, queries, d1), _run(grown, queries, d1)
        _check(pr, queries, a, d1)
        assert b["err"] == CLEAN
        assert np.array_equal(a["out"], b["out"])
