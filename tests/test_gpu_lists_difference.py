"""GPU checks of the difference with a resident index (include/turbopfor_gpu.h
tpf_lists_difference): probe doc ids, as CSR segments with one target list
each, that are NOT in the lists of a delta-1 stream with its skip table.  The
streams are the oracle's composition (tests/lists_ref.py through
tests/lists_index.py); the expected values, output pointers, probe indices and
insertion positions are the numpy restatement of the definition in
tests/lists_difference_ref.py (tests/test_lists_difference_cpu.py holds it
against np.setdiff1d and the union's reference), never the code under test.
Every comparison is bit for bit."""
import numpy as np
import pytest

import lists_difference_ref as dr
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


def _run(ix, queries, cap=None, shift=0, table=None, offs=None, base=None, probe_ptr=None, qlist=None, ptr0=PTR0, positions=True,
         fn=None):
    """The difference of queries [(list, probe values)] against `ix` in one
    call (fn: another entry point with the same arguments).  The probe lies
    between ptr0 leading and 5 trailing values that must not be read: members
    of the first non-empty list, alternating with a value no ascending list
    holds (they end below 2^31 + 2^29) -- counted by mistake, the one would
    show in the intersection's pointers and the other in the difference's.
    The four outputs are sentinel-guarded, d_out, pidx and tpos 4 bytes past a
    16-byte boundary.  cap: the capacity (default: the probe values, 9 more)."""
    member = next(int(v[0]) for v in ix.lists if len(v))
    around = np.array([member, 0xF0000001] * 4, np.uint32)
    segs = [np.asarray(pv, dtype=np.uint32) for _, pv in queries]
    probe = np.concatenate([np.resize(around, ptr0)] + segs + [around[1:6]])
    pp = ptr0 + np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    if cap is None:
        cap = sum(len(s) for s in segs) + 9
    out, pidx, tpos = li.Guarded32(torch, cap), li.Guarded32(torch, cap), li.Guarded32(torch, cap)
    out_ptr = li.Guarded64(torch, len(queries) + 1)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    (fn or tpf.lists_difference)(li.dev8(torch, ix.packed, shift), li.dev64(torch, ix.offs if offs is None else offs),
                                 li.dev64(torch, ix.ptr), li.dev32(torch, ix.base if base is None else base),
                                 li.dev32(torch, ix.table if table is None else table), li.dev32(torch, probe),
                                 li.dev64(torch, pp if probe_ptr is None else probe_ptr),
                                 li.dev32(torch, [j for j, _ in queries] if qlist is None else qlist), start0=li.dev32(torch, ix.start0),
                                 out=out.view, out_ptr=out_ptr.view, pidx=pidx.view if positions else None,
                                 tpos=tpos.view if positions else None, err=err)
    r = dict(err=int(err.item()), probe=probe, pp=pp)
    for name, g in (("out", out), ("pidx", pidx), ("tpos", tpos), ("out_ptr", out_ptr)):
        r[name], ok = g.read()
        assert ok, name + ": a value outside the buffer was written"
    return r


def _check(ix, queries, r, ptr0=PTR0, positions=True):
    assert r["err"] == CLEAN
    vals, out_ptr, pidx, tpos = dr.want_difference(ix, queries, ptr0)
    assert np.array_equal(r["out_ptr"], out_ptr)
    n = len(vals)
    assert np.array_equal(r["out"][:n], vals)
    if positions:
        assert np.array_equal(r["pidx"][:n], pidx) and np.array_equal(r["tpos"][:n], tpos)
    else:
        assert (r["pidx"] == SENT).all() and (r["tpos"] == SENT).all()
    for name in ("out", "pidx", "tpos"):
        assert (r[name][n:] == SENT).all(), name  # the slots past the result still hold the sentinel
    return n


def _untouched(r, out_ptr_too=True):
    for name in ("out", "pidx", "tpos"):
        assert (r[name] == SENT).all(), name
    if out_ptr_too:
        assert (r["out_ptr"] == SENT64).all()


def _mixed(ix, j, rng, members=40, others=40):
    """an ascending probe for list j: about `members` of its values and `others` values that are not in it"""
    v = ix.lists[j]
    take = v[rng.permutation(len(v))[:members]] if len(v) else np.zeros(0, np.uint32)
    hi = int(v[-1]) + 20000 if len(v) else 1 << 31
    lo = max(int(ix.start0[j]) - 20000, 0)
    cand = rng.integers(lo, min(hi, 1 << 32), size=others, dtype=np.uint64).astype(np.uint32)
    cand = cand[~np.isin(cand, v)]
    return np.unique(np.concatenate([take, cand]))


# ---- 1. the edges of the definition ---------------------------------------------------
@pytest.mark.parametrize("shift", [0, 5])
def test_edges_of_the_definition(ascending, shift):
    for ix in ascending:
        queries = [(j, dr.edge_probe(ix, j)) for j in range(ix.nlists)]
        r = _run(ix, queries, shift=shift)
        n = _check(ix, queries, r)
        assert n > 2 * ix.nlists
        # empty lists: everything is a miss and tpos is 0
        for k, (j, pv) in enumerate(queries):
            if ix.lens[j] == 0:
                a, b = int(r["out_ptr"][k]), int(r["out_ptr"][k + 1])
                assert b - a == len(pv) and (r["tpos"][a:b] == 0).all()
    mx = ascending[0]
    assert {0, 5, 256, 257, 256 * 17 + 3} <= set(mx.lens)  # empty, tail only, one block, a block and one, a tail after full blocks


# ---- 2. mixed members and non-members --------------------------------------------------
def _mixed_request(ix):
    rng = np.random.default_rng(61)
    queries = [(j, _mixed(ix, j, rng)) for j in range(ix.nlists)]
    twice = ix.of_len(256 * 63 + 255)
    queries.append((twice, _mixed(ix, twice, rng)))  # the same list again, another probe
    empty = np.zeros(0, np.uint32)
    full = ix.of_len(513)
    queries += [(0, empty), (twice, empty), (ix.of_len(0), empty), (3, empty),
                (ix.of_len(0), np.array([0, 7, 0xFFFFFFFF], np.uint32)),       # a probe on an empty list
                (full, ix.lists[full][3:400:2]),                                # all members: an empty slice
                (full, np.setdiff1d(ix.lists[full][:-1] + 1, ix.lists[full]))]  # all non-members
    queries = [queries[i] for i in rng.permutation(len(queries))]
    return [(1, empty)] + queries + [(2, empty), (2, empty)]  # empty segments first, last and in a row


@pytest.mark.parametrize("positions", [True, False])
def test_mixed_members_and_non_members(ascending, positions):
    ix = ascending[0]
    queries = _mixed_request(ix)
    r = _run(ix, queries, positions=positions)
    n = _check(ix, queries, r, positions=positions)
    assert n > 30 * ix.nlists
    sizes = np.diff(r["out_ptr"])
    lens = np.array([len(pv) for _, pv in queries])
    assert ((sizes == 0) & (lens > 100)).any() and ((sizes == lens) & (lens > 100)).any()  # the all-members and the all-others segment


def test_small_index_every_list(ascending):
    ix = ascending[1]
    rng = np.random.default_rng(3)
    queries = [(j, _mixed(ix, j, rng, 20, 50)) for j in (6, 5, 4, 3, 2, 1, 0, 2, 6)]
    _check(ix, queries, _run(ix, queries, shift=5))


# ---- 3. misses that cost no decode, beside a segment that needs decodes ----------------------
def test_misses_without_a_decode(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(97)
    j, e = ix.of_len(256 * 17 + 3), ix.of_len(0)
    v = ix.lists[j]
    above = np.arange(int(v[-1]) + 1, int(v[-1]) + 201, dtype=np.uint32)  # wholly above the list's last value: no unit
    needs = np.unique(np.concatenate([v[:3], _mixed(ix, j, rng, 100, 100)]))  # lands in the list's first unit, among others
    queries = [(j, above), (j, needs), (e, np.arange(5, 150, dtype=np.uint32)), (j, above[::-1].copy())]
    r = _run(ix, queries)
    _check(ix, queries, r)
    assert (r["tpos"][:200] == len(v)).all()  # n_j: no value above
    # with the end of every unit of the list moved by one byte its first unit's parse disagrees with its offsets, and any
    # decode of it is reported; the segments without a unit are still answered, clean: nothing was decoded for them
    offs = ix.offs.copy()
    offs[int(ix.base[j]) + 1: int(ix.base[j + 1])] += 1
    quiet = [queries[0], queries[2], queries[3]]
    _check(ix, quiet, _run(ix, quiet, offs=offs))
    assert _run(ix, queries, offs=offs)["err"] == int(ix.base[j])


# ---- 4. misses crowding into one position ---------------------------------------------------
def _gap_run(unit, m):
    """m consecutive integers strictly between two neighbouring values of `unit`"""
    p = int(np.argmax(np.diff(unit.astype(np.int64))))
    assert int(unit[p + 1]) - int(unit[p]) > m + 1
    return p, np.arange(int(unit[p]) + 1, int(unit[p]) + 1 + m, dtype=np.uint32)


def test_miss_crowding(ascending):
    ix = ascending[0]
    j, tailonly = ix.of_len(256 * 17 + 3), ix.of_len(255)
    v = ix.lists[j]
    unit = v[256 * 5: 256 * 6]
    p, run = _gap_run(unit, 300)  # 300 non-members between two neighbours of one unit: several 64-index runs, one L
    queries = [(j, np.concatenate([unit[max(p - 3, 0): p + 1], run, unit[p + 1: p + 4]]))]
    # 300 values above a tail's last value (no unit: L = n), and 300 inside a gap of a tail-only list
    tail = v[256 * 17:]
    assert len(tail) == 3
    t = ix.lists[tailonly]
    queries.append((j, np.concatenate([tail, np.arange(int(tail[-1]) + 1, int(tail[-1]) + 301, dtype=np.uint32)])))
    pt, runt = _gap_run(t, 300)
    queries.append((tailonly, np.concatenate([t[pt: pt + 1], runt, t[pt + 1:]])))
    r = _run(ix, queries)
    _check(ix, queries, r)
    a = int(np.nonzero(r["out"] == run[0])[0][0])
    assert (r["tpos"][a: a + 300] == 256 * 5 + p + 1).all()
    # the same 300 past the tail's last value with a table whose last entries are 0xFFFFFFFF: they land in the tail unit,
    # q == cnt, L = n -- the same answer, now through a decode
    table = ix.table.copy()
    table[int(ix.base[j + 1]) - 1] = 0xFFFFFFFF
    table[int(ix.base[tailonly + 1]) - 1] = 0xFFFFFFFF
    edge = [(j, queries[1][1]), (tailonly, np.concatenate([t[-2:], np.arange(int(t[-1]) + 1, int(t[-1]) + 301, dtype=np.uint32)]))]
    r = _run(ix, edge, table=table)
    _check(ix, edge, r)
    assert (r["tpos"][:300] == len(v)).all() and (r["tpos"][300:600] == 255).all()


# ---- 5. an unsorted probe with repeats: every occurrence, in probe order ------------------------
def test_unsorted_and_duplicated_probe(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(71)
    queries = []
    for j in (ix.of_len(256 * 17 + 3), ix.of_len(257), ix.of_len(256 * 64), ix.of_len(0), ix.of_len(5)):
        pv = _mixed(ix, j, rng, 60, 300)
        pv = np.concatenate([pv, pv[rng.permutation(len(pv))[:100]], pv[:5]])
        queries.append((j, pv[rng.permutation(len(pv))]))
    n = _check(ix, queries, _run(ix, queries))
    assert n > 5 * 300


# ---- 6. the complement law --------------------------------------------------------------------
def _complement(ix, queries, **kw):
    d = _run(ix, queries, **kw)
    i = _run(ix, queries, fn=tpf.lists_intersect, **kw)
    assert d["err"] == CLEAN and i["err"] == CLEAN
    assert d["out_ptr"][0] == 0 and i["out_ptr"][0] == 0
    pp = d["pp"]
    for k in range(len(queries)):
        dp = d["pidx"][int(d["out_ptr"][k]): int(d["out_ptr"][k + 1])]
        ip = i["pidx"][int(i["out_ptr"][k]): int(i["out_ptr"][k + 1])]
        assert (np.diff(dp.astype(np.int64)) > 0).all() and (np.diff(ip.astype(np.int64)) > 0).all()  # probe order
        both = np.sort(np.concatenate([dp, ip]))
        assert np.array_equal(both, np.arange(pp[k], pp[k + 1])), k  # disjoint, and together every index of the segment
        assert np.array_equal(d["out"][int(d["out_ptr"][k]): int(d["out_ptr"][k + 1])], d["probe"][dp])
    n = int(d["out_ptr"][-1])
    for name in ("out", "pidx", "tpos"):
        assert (d[name][n:] == SENT).all(), name
    return d, i


def test_complement_law_on_the_mixed_request(ascending):
    ix = ascending[0]
    d, i = _complement(ix, _mixed_request(ix))
    assert d["out_ptr"][-1] > 100 and i["out_ptr"][-1] > 100


def test_complement_law_on_a_wrapping_target():
    rng = np.random.default_rng(23)
    ix = Index([256 * 20 + 5, 300, 256 * 3], rng, start0=np.array([(1 << 32) - 40000, 7, (1 << 32) - 3000000], np.uint32))
    assert int(ix.lists[0][-1]) < int(ix.lists[0][0]) and int(ix.lists[2][-1]) < int(ix.lists[2][0])  # wrapped
    queries = []
    for j in (0, 2, 1, 0):
        v = ix.lists[j]
        pv = np.concatenate([v[rng.permutation(len(v))[:80]], rng.integers(0, 1 << 32, size=40, dtype=np.uint64).astype(np.uint32),
                             np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)])
        queries.append((j, np.sort(pv)))
    d, _ = _complement(ix, queries)
    for k, (j, pv) in enumerate(queries):
        a, b = int(d["out_ptr"][k]), int(d["out_ptr"][k + 1])
        assert (d["tpos"][a:b] <= ix.lens[j]).all()
    # the list that does not wrap is answered exactly
    k = 2
    want = dr.difference_one(ix.lists[1], queries[k][1], int(d["pp"][k]))
    a, b = int(d["out_ptr"][k]), int(d["out_ptr"][k + 1])
    assert np.array_equal(d["out"][a:b], want[0]) and np.array_equal(d["pidx"][a:b], want[1]) and np.array_equal(d["tpos"][a:b], want[2])


def test_complement_law_with_a_wrong_table(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(89)
    queries = [(j, _mixed(ix, j, rng, 60, 20)) for j in range(ix.nlists)]
    j = ix.of_len(256 * 17 + 3)
    queries.append((j, np.sort(np.concatenate([ix.lists[j][200:300], np.array([0, 0xFFFFFFFF], np.uint32)]))))
    d, i = _complement(ix, queries, table=np.full(ix.nunits, 0xFFFFFFFF, np.uint32))
    # every probe value maps to its list's first unit, which starts from start0: which indices are reported is determined --
    # the difference against the lists cut to their first 256 values.  L is the search's q over that unit: the insertion
    # position for a value that is not above the unit's last value (the table's promise), and at most the unit's count
    first = Index(None, rng, start0=ix.start0, lists=[v[:256] for v in ix.lists])
    vals, out_ptr, pidx, tpos = dr.want_difference(first, queries, PTR0)
    n = len(vals)
    assert n > 100 and np.array_equal(d["out_ptr"], out_ptr)
    assert np.array_equal(d["out"][:n], vals) and np.array_equal(d["pidx"][:n], pidx)
    cnt = np.repeat([len(first.lists[j]) for j, _ in queries], np.diff(out_ptr))
    inside = tpos < cnt
    assert inside.sum() > 100 and np.array_equal(d["tpos"][:n][inside], tpos[inside]) and (d["tpos"][:n] <= cnt).all()
    _complement(ix, queries, table=rng.integers(0, 1 << 32, size=ix.nunits, dtype=np.uint64).astype(np.uint32))


# ---- 7. chaining on the device ----------------------------------------------------------------
def test_chained_three_operator_queries():
    """(A AND B) AND NOT C, and A AND NOT B AND NOT C: chained calls on one stream with no host step in between; the last
    call's tpos, without the positions equal to n_j, read through tpf_lists_gather gives the successor doc ids."""
    rng = np.random.default_rng(73)
    common = np.unique(rng.integers(1, 1 << 28, size=3000, dtype=np.uint64))
    lists = [np.unique(np.concatenate([common[rng.random(len(common)) < 0.8], rng.integers(1, 1 << 28, size=n, dtype=np.uint64)]))
             .astype(np.uint32) for n in (5000, 9000, 14000)]
    ix = Index(None, rng, ptr0=7, start0=np.zeros(3, np.uint32), lists=lists)
    assert ix.ascends()
    A, B, C = lists
    packed, offs, ptr, base = li.dev8(torch, ix.packed), li.dev64(torch, ix.offs), li.dev64(torch, ix.ptr), li.dev32(torch, ix.base)
    table, st = li.dev32(torch, ix.table), li.dev32(torch, ix.start0)
    n0 = len(A)
    err = torch.zeros(5, dtype=torch.int64, device=DEV)
    q = [li.dev32(torch, [j]) for j in range(3)]
    new = lambda: torch.empty(n0, dtype=torch.int32, device=DEV)
    # the first probe is a selective decode; nothing comes back to the host between the calls
    out0, ptr0 = tpf.decn256v32_lists_select(packed, offs, ptr, base, q[0], d1=True, start0=st, out=new(), err=err[0:1])
    ab, ab_ptr = tpf.lists_intersect(packed, offs, ptr, base, table, out0, ptr0, q[1], start0=st, err=err[1:2])
    tpos1 = new()
    r1, r1_ptr = tpf.lists_difference(packed, offs, ptr, base, table, ab, ab_ptr, q[2], start0=st, tpos=tpos1, err=err[2:3])
    anb, anb_ptr = tpf.lists_difference(packed, offs, ptr, base, table, out0, ptr0, q[1], start0=st, err=err[3:4])
    tpos2, pidx2 = new(), new()
    r2, r2_ptr = tpf.lists_difference(packed, offs, ptr, base, table, anb, anb_ptr, q[2], start0=st, pidx=pidx2, tpos=tpos2,
                                      err=err[4:5])
    assert err.tolist() == [CLEAN] * 5
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    want1 = np.setdiff1d(np.intersect1d(A, B), C)
    want2 = np.setdiff1d(np.setdiff1d(A, B), C)
    assert len(want1) > 100 and len(want2) > 100 and len(np.intersect1d(np.intersect1d(A, B), C)) > 100
    assert r1_ptr.tolist() == [0, len(want1)] and r2_ptr.tolist() == [0, len(want2)]
    assert np.array_equal(u32(r1)[:len(want1)], want1) and np.array_equal(u32(r2)[:len(want2)], want2)
    assert np.array_equal(u32(pidx2)[:len(want2)], np.nonzero(~np.isin(np.setdiff1d(A, B), C))[0])
    for got, want in ((tpos1, want1), (tpos2, want2)):
        tp = u32(got)[:len(want)]
        assert np.array_equal(tp, np.searchsorted(C, want, side="left"))
        keep = tp < len(C)  # n_j is not a gather position
        assert 0 < keep.sum()
        pos = li.dev32(torch, tp[keep])
        gerr = torch.zeros(1, dtype=torch.int64, device=DEV)
        succ = tpf.lists_gather(packed, offs, ptr, base, pos, li.dev64(torch, [0, int(keep.sum())]), q[2], d1=True, start0=st,
                                unit_last=table, err=gerr)
        assert int(gerr.item()) == CLEAN
        nxt = u32(succ)
        assert np.array_equal(nxt, C[tp[keep]]) and (nxt > want[keep]).all()  # the first doc id of C above each result


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
    vals, out_ptr, _, _ = dr.want_difference(ix, queries, PTR0)
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


@pytest.mark.parametrize("tail", [False, True])
def test_corrupted_block(ascending, tail):
    """A corrupted unit is reported, by its source unit, only when a probe value lands in it; all writes stay in bounds."""
    ix = ascending[1]
    j, i = (2, 2) if tail else (6, 9)  # the tail of the 612-value list; unit 9 of the 17-unit list
    u = int(ix.base[j]) + i
    offs = ix.offs.copy()
    offs[u + 1] += 1  # its end offset, the start of the unit after it, moves by one
    v = ix.lists[j]
    rng = np.random.default_rng(83)
    far = np.sort(np.concatenate([v[:200], v[256: 256 + 50] + 1] if tail else [v[256 * 2: 256 * 2 + 40] + 1, v[256 * 12: 256 * 14: 7]]))
    others = [(0, _mixed(ix, 0, rng, 5, 5)), (4, _mixed(ix, 4, rng, 5, 5))]  # not list 3: its unit follows the 612-value list's tail
    into = np.sort(np.concatenate([far, v[256 * i + 3: 256 * i + 6] + 1]))
    r = _run(ix, others + [(j, into)], offs=offs)  # _run holds the guards
    assert r["err"] == u
    op = r["out_ptr"]
    assert op[0] == 0 and (np.diff(op) >= 0).all() and op[-1] <= sum(len(pv) for _, pv in others) + len(into)
    for name in ("out", "pidx", "tpos"):
        assert (r[name][int(op[-1]):] == SENT).all(), name
    # no probe value in that unit or in the one after it: clean and exact
    queries = others + [(j, far)]
    _check(ix, queries, _run(ix, queries, offs=offs))


# ---- 9. the work does not depend on the rest of the index -----------------------------------------
def test_index_independence(ascending):
    ix = ascending[1]
    rng = np.random.default_rng(53)
    more_len = [int(n) for n in rng.integers(0, 300, size=1000)]
    more_s0 = rng.integers(0, 1 << 31, size=1000, dtype=np.uint64).astype(np.uint32)
    more = [ref.d1_values(n, int(s), rng) for n, s in zip(more_len, more_s0)]
    grown = Index(None, rng, ptr0=11, start0=np.concatenate([ix.start0, more_s0]), lists=ix.lists + more)
    assert grown.nunits > 10 * ix.nunits or len(grown.vals) > 10 * len(ix.vals)
    queries = _eight(ix, np.random.default_rng(79))
    a, b = _run(ix, queries), _run(grown, queries)
    _check(ix, queries, a)
    assert b["err"] == CLEAN
    for name in ("out", "out_ptr", "pidx", "tpos"):
        assert np.array_equal(a[name], b[name]), name
