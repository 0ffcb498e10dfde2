"""GPU checks of the intersection with a resident index
(include/turbopfor_gpu.h tpf_lists_intersect): probe doc ids, as CSR segments
with one target list each, against a delta-1 lists stream with its skip table.
The streams are the oracle's composition (tests/lists_ref.py through
tests/lists_index.py); the expected hits, output pointers, probe indices and
list positions are numpy restatements of the definition -- np.isin,
np.searchsorted, slices of the original lists -- never the code under test."""
import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
from lists_index import CLEAN, DEV, SENT, SENT64, Index

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SMALL = [300, 0, 612, 256, 90, 0, 256 * 17]
PTR0 = 3  # probe values before the first segment: members of a list, never to be read


@pytest.fixture(scope="module")
def ascending():
    """[the shape matrix, SMALL]: start0 < 2^31 and gaps below 2^14, so at most 33,357 values cannot wrap"""
    rng = np.random.default_rng(17)
    lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
    ixs = [Index(lens, rng, ptr0=37, start_bits=31), Index(SMALL, rng, ptr0=11, start_bits=31)]
    for ix in ixs:
        assert ix.ascends()
    return ixs


def _run(ix, queries, cap=None, shift=0, table=None, offs=None, base=None, probe_ptr=None, qlist=None, ptr0=PTR0, positions=True):
    """Intersect queries [(list, probe values)] with `ix` in one call.  The
    probe lies between ptr0 leading and 5 trailing values that are members of
    the first non-empty list; the four outputs are sentinel-guarded, d_out,
    pidx and tpos 4 bytes past a 16-byte boundary."""
    member = next(int(v[0]) for v in ix.lists if len(v))
    segs = [np.asarray(pv, dtype=np.uint32) for _, pv in queries]
    probe = np.concatenate([np.full(ptr0, member, np.uint32)] + segs + [np.full(5, member, np.uint32)])
    pp = ptr0 + np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    cap = len(probe) if cap is None else cap
    out, pidx, tpos = li.Guarded32(torch, cap), li.Guarded32(torch, cap), li.Guarded32(torch, cap)
    out_ptr = li.Guarded64(torch, len(queries) + 1)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.lists_intersect(li.dev8(torch, ix.packed, shift), li.dev64(torch, ix.offs if offs is None else offs), li.dev64(torch, ix.ptr),
                        li.dev32(torch, ix.base if base is None else base), li.dev32(torch, ix.table if table is None else table),
                        li.dev32(torch, probe), li.dev64(torch, pp if probe_ptr is None else probe_ptr),
                        li.dev32(torch, [j for j, _ in queries] if qlist is None else qlist), start0=li.dev32(torch, ix.start0),
                        out=out.view, out_ptr=out_ptr.view, pidx=pidx.view if positions else None,
                        tpos=tpos.view if positions else None, err=err)
    r = dict(err=int(err.item()), probe=probe, pp=pp)
    for name, g in (("out", out), ("pidx", pidx), ("tpos", tpos), ("out_ptr", out_ptr)):
        r[name], ok = g.read()
        assert ok, name + ": a value outside the buffer was written"
    return r


def _check(ix, queries, r, ptr0=PTR0):
    assert r["err"] == CLEAN
    vals, out_ptr, pidx, tpos = li.want_hits(ix, queries, ptr0)
    assert np.array_equal(r["out_ptr"], out_ptr)
    n = len(vals)
    assert np.array_equal(r["out"][:n], vals)
    assert np.array_equal(r["pidx"][:n], pidx) and np.array_equal(r["tpos"][:n], tpos)
    for name in ("out", "pidx", "tpos"):
        assert (r[name][n:] == SENT).all(), name
    return n


def _untouched(r, out_ptr_too=True):
    for name in ("out", "pidx", "tpos"):
        assert (r[name] == SENT).all(), name
    if out_ptr_too:
        assert (r["out_ptr"] == SENT64).all()


def _clip(x):
    return min(max(x, 0), 0xFFFFFFFF)


def _mixed(ix, j, rng, members=40, others=40):
    """a sorted probe for list j: about `members` of its values and `others` values that are not in it"""
    v = ix.lists[j]
    take = v[rng.permutation(len(v))[:members]] if len(v) else np.zeros(0, np.uint32)
    hi = int(v[-1]) + 20000 if len(v) else 1 << 31
    lo = max(int(ix.start0[j]) - 20000, 0)
    cand = rng.integers(lo, min(hi, 1 << 32), size=others, dtype=np.uint64).astype(np.uint32)
    cand = cand[~np.isin(cand, v)]
    return np.sort(np.concatenate([take, cand]))


# ---- 1. the edges of the definition ---------------------------------------------------
def _edge_probe(ix, j):
    v = ix.lists[j]
    n = len(v)
    marks = {int(ix.start0[j]), 0, 0xFFFFFFFF}
    if n:
        marks |= {int(v[0]), int(v[-1]), int(v[-1]) + 1}  # the last value + 1 (and + 2) lies past the list: it names no unit
        for i in {0, ref.n_units(n) // 2, ref.n_units(n) - 2}:
            if 0 <= i and 256 * (i + 1) < n:
                marks |= {int(v[256 * (i + 1) - 1]), int(v[256 * (i + 1)])}
    return np.array(sorted({_clip(m + d) for m in marks for d in (-1, 0, 1)}), dtype=np.uint32)


@pytest.mark.parametrize("shift", [0, 5])
def test_edges_of_the_definition(ascending, shift):
    for ix in ascending:
        queries = [(j, _edge_probe(ix, j)) for j in range(ix.nlists)]
        n = _check(ix, queries, _run(ix, queries, shift=shift))
        assert n > 2 * ix.nlists
        for j, pv in queries:
            assert not np.isin(ix.start0[j], ix.lists[j]) and ix.start0[j] in pv  # start0 itself is no member
    mx = ascending[0]
    targets = {mx.lens[j] for j in range(mx.nlists)}
    assert {0, 5, 256} <= targets  # an empty target, a tail-only list, exactly one full block
    j = mx.of_len(256 * 17 + 3)
    assert np.isin(mx.lists[j][-1], _edge_probe(mx, j))  # a hit in a p4Enc32 tail after full blocks


# ---- 2. sampled members and non-members ------------------------------------------------
def test_sampled_members_and_non_members(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(61)
    queries = [(j, _mixed(ix, j, rng)) for j in range(ix.nlists)]
    twice = ix.of_len(256 * 63 + 255)
    queries.append((twice, _mixed(ix, twice, rng)))  # the same list again, another probe
    empty = np.zeros(0, np.uint32)
    queries += [(0, empty), (twice, empty), (ix.of_len(0), empty), (3, empty)]
    queries = [queries[i] for i in rng.permutation(len(queries))]
    queries = [(1, empty)] + queries + [(2, empty), (2, empty)]  # empty segments first and last too
    n = _check(ix, queries, _run(ix, queries))
    assert n > 30 * 10


# ---- 3. segment lengths ----------------------------------------------------------------
def test_segment_lengths(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(67)
    j, other = ix.of_len(256 * 17 + 3), ix.of_len(513)
    unit = ix.lists[j][256 * 5: 256 * 6]
    inside = np.setdiff1d(rng.integers(int(unit[0]), int(unit[-1]), size=400, dtype=np.uint64).astype(np.uint32), unit)
    queries = []
    for m in (1, 63, 64, 65, 257):
        half = min(m // 2 + 1, 200)
        pv = np.sort(np.concatenate([unit[rng.permutation(256)[:half]], inside[rng.permutation(len(inside))[:m - half]]]))
        assert len(pv) == m
        queries += [(j, pv), (other, _mixed(ix, other, rng, 3, 3))]  # another list in between: the segments stay separate items
    p = int(np.argmax(np.diff(unit.astype(np.int64))))
    assert int(unit[p + 1]) - int(unit[p]) > 1001 and 3 <= p <= 250
    run = np.arange(int(unit[p]) + 1, int(unit[p]) + 1001, dtype=np.uint32)  # 1,000 consecutive integers between two target values
    queries.append((j, np.sort(np.concatenate([unit[p - 3: p + 4], run]))))
    queries.append((j, unit))  # the next segment names the same list and unit: one item across two queries
    for _, pv in queries[::2]:
        assert int(unit[0]) <= int(pv[0]) and int(pv[-1]) <= int(unit[-1])  # every value lands in the one unit
    _check(ix, queries, _run(ix, queries))


def test_dense_probe(ascending):
    ix = ascending[0]
    a, b = ix.of_len(256 * 64 + 1), ix.of_len(256 * 130 + 77)
    queries = [(b, ix.lists[a]), (a, ix.lists[b]), (b, ix.lists[b])]  # a whole list against the longer one, the reverse, and itself
    n = _check(ix, queries, _run(ix, queries))
    assert n >= ix.lens[b]


def test_probe_past_one_scan_tile(ascending):
    """More than 64 * 4,096 probe values: the run scans over the probe's 64-value runs take their two-launch form."""
    ix = ascending[0]
    j, other = ix.of_len(256 * 130 + 77), ix.of_len(257)
    v = ix.lists[j]
    run = np.arange(int(v[1000]) - 5, int(v[1000]) - 5 + 64 * 4096 + 1500, dtype=np.uint32)  # consecutive integers across a few units
    queries = [(other, ix.lists[other][::3]), (j, run), (j, v[-300:])]
    n = _check(ix, queries, _run(ix, queries))
    assert n > 10 + 86 + 300 and PTR0 + sum(len(pv) for _, pv in queries) > 64 * 4096


# ---- 4. many small queries -------------------------------------------------------------
def test_many_small_queries(ascending):
    """150 queries of 0 to 40 probe values: the item runs of 16 span many queries, the tails kernel many waves."""
    ix = ascending[0]
    rng = np.random.default_rng(43)
    queries, tails = [], 0
    for _ in range(150):
        j = int(rng.integers(0, ix.nlists))
        m = int(rng.integers(0, 41))
        pv = _mixed(ix, j, rng, m // 2, m - m // 2)[:m]
        if ix.lens[j] % 256 and rng.random() < 0.4:
            pv = np.sort(np.concatenate([pv, ix.lists[j][-int(rng.integers(1, 4)):]]))[:40]
        queries.append((j, pv))
        if len(pv) and ix.lens[j] % 256:  # the probe values past the last full block land in the list's tail unit
            nfull = ix.lens[j] // 256
            lo = int(ix.lists[j][256 * nfull - 1]) if nfull else -1
            tails += bool(((pv.astype(np.int64) > lo) & (pv <= ix.lists[j][-1])).any())
    assert tails >= 10
    assert min(len(pv) for _, pv in queries) == 0 and max(len(pv) for _, pv in queries) == 40
    _check(ix, queries, _run(ix, queries))


# ---- 5. an unsorted probe with repeats ---------------------------------------------------
def test_unsorted_and_duplicated_probe(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(71)
    queries = []
    for j in (ix.of_len(256 * 17 + 3), ix.of_len(257), ix.of_len(256 * 64)):
        pv = _mixed(ix, j, rng, 60, 30)
        pv = np.concatenate([pv, pv[rng.permutation(len(pv))[:30]], pv[:5]])
        queries.append((j, pv[rng.permutation(len(pv))]))
    r = _run(ix, queries)
    n = _check(ix, queries, r)  # exact membership in probe order, every occurrence
    assert len(np.unique(r["pidx"][:n])) == n and len(np.unique(r["out"][:n])) < n


# ---- 6. chaining: a 3-term AND on the device ----------------------------------------------
def test_chained_three_term_and():
    rng = np.random.default_rng(73)
    common = np.unique(rng.integers(1, 1 << 28, size=3000, dtype=np.uint64))
    lists = [np.unique(np.concatenate([common, rng.integers(1, 1 << 28, size=n, dtype=np.uint64)])).astype(np.uint32)
             for n in (5000, 9000, 14000)]
    ix = Index(None, rng, ptr0=7, start0=np.zeros(3, np.uint32), lists=lists)
    assert ix.ascends()
    want = np.intersect1d(np.intersect1d(lists[0], lists[1]), lists[2])
    assert 0 < len(want) < min(len(v) for v in lists)
    packed, offs, ptr, base = li.dev8(torch, ix.packed), li.dev64(torch, ix.offs), li.dev64(torch, ix.ptr), li.dev32(torch, ix.base)
    table, st = li.dev32(torch, ix.table), li.dev32(torch, ix.start0)
    n0 = len(lists[0])
    err = torch.zeros(2, dtype=torch.int64, device=DEV)
    pidx1 = torch.empty(n0, dtype=torch.int32, device=DEV)
    pidx2 = torch.empty(n0, dtype=torch.int32, device=DEV)
    tpos2 = torch.empty(n0, dtype=torch.int32, device=DEV)
    out1, ptr1 = tpf.lists_intersect(packed, offs, ptr, base, table, li.dev32(torch, lists[0]), li.dev64(torch, [0, n0]),
                                     li.dev32(torch, [1]), start0=st, pidx=pidx1, err=err[0:1])
    # the output of the first call is the probe of the second: nothing comes back to the host in between
    out2, ptr2 = tpf.lists_intersect(packed, offs, ptr, base, table, out1, ptr1, li.dev32(torch, [2]), start0=st, pidx=pidx2, tpos=tpos2,
                                     err=err[1:2])
    assert err.tolist() == [CLEAN, CLEAN]
    n1, n2 = int(ptr1[1].item()), int(ptr2[1].item())
    assert ptr1[0].item() == 0 and ptr2[0].item() == 0
    assert n1 == len(np.intersect1d(lists[0], lists[1])) and n2 == len(want)
    got = out2.cpu().numpy().view(np.uint32)[:n2]
    assert np.array_equal(got, want)
    # positions: through both calls back into the first list, and directly into the third
    p2 = pidx2.cpu().numpy().view(np.uint32)[:n2]
    p1 = pidx1.cpu().numpy().view(np.uint32)[:n1]
    assert np.array_equal(lists[0][p1[p2]], want)
    assert np.array_equal(lists[2][tpos2.cpu().numpy().view(np.uint32)[:n2]], want)


# ---- 7. blocks of every exception kind -------------------------------------------------------
def _kinds_lists(rng, lens, start0):
    """per 256-value block a gap width of 1..7 bits and an outlier rate; outlier gaps of 9..14 bits"""
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
    assert ix.ascends()
    queries = []
    for j in range(ix.nlists):
        v = ix.lists[j]
        take = np.concatenate([v[256 * u: 256 * (u + 1)][rng.permutation(min(256, len(v) - 256 * u))[:3]] for u in range(ix.units(j))]
                              + [np.zeros(0, np.uint32)]).astype(np.int64)
        pv = np.unique(np.clip(np.concatenate([take - 1, take, take + 1]), 0, 0xFFFFFFFF)).astype(np.uint32)  # members of every unit, +-1
        queries.append((j, pv))
    n = _check(ix, queries, _run(ix, queries))
    assert n >= 3 * (ix.nunits - 3)


# ---- 8. refusals ------------------------------------------------------------------------------
def _eight(ix, rng):
    """8 queries over SMALL; query 3 is the only one that names list 6 (the last list of the directory)"""
    return [(j, _mixed(ix, j, rng, 6, 4)) for j in (0, 2, 3, 6, 4, 1, 2, 0)]


@pytest.mark.parametrize("what", ["nlists", "ffffffff", "descending", "past_probe", "past_probe_last", "directory"])
def test_refused_query(ascending, what):
    ix = ascending[1]
    queries = _eight(ix, np.random.default_rng(79))
    lens = [len(pv) for _, pv in queries]
    pp = PTR0 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    probe_values = PTR0 + sum(lens) + 5
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
        kw = dict(probe_ptr=pp)
    elif what == "past_probe":
        pp[4] = probe_values + 1
        kw = dict(probe_ptr=pp)
    elif what == "past_probe_last":
        pp[8] = probe_values + 1  # probe_ptr[nq]: the last query's end
        kw, k = dict(probe_ptr=pp), 7
    else:
        base = ix.base.copy()
        assert base[7] == ix.nunits
        base[7] = ix.nunits + 1
        kw = dict(base=base)
    r = _run(ix, queries, **kw)
    assert r["err"] == ix.nunits + k
    _untouched(r)


def test_capacity_one_short(ascending):
    ix = ascending[1]
    queries = _eight(ix, np.random.default_rng(79))
    vals, out_ptr, _, _ = li.want_hits(ix, queries, PTR0)
    assert len(vals) > 8
    r = _run(ix, queries, cap=len(vals) - 1)
    assert r["err"] == ix.nunits + len(queries)
    _untouched(r, out_ptr_too=False)
    assert np.array_equal(r["out_ptr"], out_ptr)  # complete and correct: out_ptr[nq] is what to allocate
    _check(ix, queries, _run(ix, queries, cap=len(vals)))


def test_nq_zero(ascending):
    r = _run(ascending[1], [])
    assert r["err"] == CLEAN and r["out_ptr"].tolist() == [0]
    _untouched(r, out_ptr_too=False)


# ---- 9. a corrupted block is reported only when a probe value lands in it -----------------------
@pytest.mark.parametrize("tail", [False, True])
def test_corrupted_block(ascending, tail):
    ix = ascending[1]
    j, i = (2, 2) if tail else (6, 9)  # the tail of the 612-value list; unit 9 of the 17-unit list
    u = int(ix.base[j]) + i
    offs = ix.offs.copy()
    offs[u + 1] += 1  # its end offset, the start of the unit after it, moves by one
    v = ix.lists[j]
    rng = np.random.default_rng(83)
    far = np.sort(np.concatenate([v[:200], v[256: 256 + 50]] if tail else [v[256 * 2: 256 * 2 + 40], v[256 * 12: 256 * 14: 7]]))
    others = [(0, _mixed(ix, 0, rng, 5, 5)), (4, _mixed(ix, 4, rng, 5, 5))]  # not list 3: its unit follows the 612-value list's tail
    into = np.sort(np.concatenate([far, v[256 * i + 3: 256 * i + 6]]))
    assert _run(ix, others + [(j, into)], offs=offs)["err"] == u
    # no probe value in that unit or in the one after it: clean and exact
    queries = others + [(j, far)]
    _check(ix, queries, _run(ix, queries, offs=offs))


# ---- 10. a wrong table is harmless, and what it does is determined -------------------------------
def test_wrong_table(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(89)
    queries = [(j, _mixed(ix, j, rng, 60, 20)) for j in range(ix.nlists)]
    j = ix.of_len(256 * 17 + 3)
    queries.append((j, np.sort(np.concatenate([ix.lists[j][200:300], np.array([0, 0xFFFFFFFF], np.uint32)]))))
    r = _run(ix, queries, table=np.full(ix.nunits, 0xFFFFFFFF, np.uint32))
    assert r["err"] == CLEAN
    # every probe value maps to its list's first unit, which starts from start0: exactly the members at positions below 256
    first = Index(None, rng, start0=ix.start0, lists=[v[:256] for v in ix.lists])
    vals, out_ptr, pidx, tpos = li.want_hits(first, queries, PTR0)
    n = len(vals)
    assert n > 100 and np.array_equal(r["out_ptr"], out_ptr)
    assert np.array_equal(r["out"][:n], vals) and np.array_equal(r["pidx"][:n], pidx) and np.array_equal(r["tpos"][:n], tpos)
    assert (r["out"][n:] == SENT).all() and (r["pidx"][n:] == SENT).all() and (r["tpos"][n:] == SENT).all()


# ---- 11. a target that wraps ------------------------------------------------------------------
def test_wrapping_target():
    rng = np.random.default_rng(23)
    ix = Index([256 * 20 + 5, 300, 256 * 3], rng, start0=np.array([(1 << 32) - 40000, 7, (1 << 32) - 3000000], np.uint32))
    assert int(ix.lists[0][-1]) < int(ix.lists[0][0]) and int(ix.lists[2][-1]) < int(ix.lists[2][0])  # wrapped
    queries = []
    for j in (0, 2, 1, 0):
        v = ix.lists[j]
        pv = np.concatenate([v[rng.permutation(len(v))[:80]], rng.integers(0, 1 << 32, size=40, dtype=np.uint64).astype(np.uint32),
                             np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)])
        queries.append((j, np.sort(pv)))
    r = _run(ix, queries)
    assert r["err"] == CLEAN
    op = r["out_ptr"]
    assert op[0] == 0 and (np.diff(op) >= 0).all()
    for k, (j, pv) in enumerate(queries):
        assert op[k + 1] - op[k] <= len(pv)
        a, b = int(op[k]), int(op[k + 1])
        # every reported triple is true of the list: the value at tpos is v, and v is the probe value at pidx
        assert np.array_equal(ix.lists[j][r["tpos"][a:b]], r["out"][a:b])
        assert np.array_equal(r["probe"][r["pidx"][a:b]], r["out"][a:b])
        assert ((r["pidx"][a:b] >= r["pp"][k]) & (r["pidx"][a:b] < r["pp"][k + 1])).all()
    n = int(op[-1])
    assert (r["out"][n:] == SENT).all() and (r["pidx"][n:] == SENT).all() and (r["tpos"][n:] == SENT).all()
    # the list that does not wrap is answered exactly
    k = 2
    want = queries[k][1][np.isin(queries[k][1], ix.lists[1])]
    assert np.array_equal(r["out"][int(op[k]): int(op[k + 1])], want)


# ---- 12. the work does not depend on the rest of the index -----------------------------------------
def test_index_independence(ascending):
    ix = ascending[1]
    rng = np.random.default_rng(53)
    more_len = [int(n) for n in rng.integers(0, 300, size=1000)]
    more_s0 = rng.integers(0, 1 << 31, size=1000, dtype=np.uint64).astype(np.uint32)
    more = [ref.d1_values(n, int(s), rng) for n, s in zip(more_len, more_s0)]
    grown = Index(None, rng, ptr0=11, start0=np.concatenate([ix.start0, more_s0]), lists=ix.lists + more)
    queries = _eight(ix, np.random.default_rng(79))
    a, b = _run(ix, queries), _run(grown, queries)
    _check(ix, queries, a)
    assert b["err"] == CLEAN
    for name in ("out", "out_ptr", "pidx", "tpos"):
        assert np.array_equal(a[name], b[name]), name
