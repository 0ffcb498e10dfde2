"""GPU checks of the union with a resident index (include/turbopfor_gpu.h
tpf_lists_union): probe doc ids, as CSR segments with one target list each,
merged with the lists of a delta-1 stream with its skip table.  The streams are
the oracle's composition (tests/lists_ref.py through tests/lists_index.py); the
expected values, output pointers, probe indices and list positions are the
numpy restatement of the definition in tests/lists_union_ref.py
(tests/test_lists_union_cpu.py holds it against np.union1d), never the code
under test."""
import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
import lists_union_ref as ur
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
         slack=9):
    """The union of queries [(list, probe values)] with `ix` in one call.  The
    probe lies between ptr0 leading and 5 trailing values that are members of
    the first non-empty list; the four outputs are sentinel-guarded, d_out,
    pidx and tpos 4 bytes past a 16-byte boundary.  cap: the capacity (default:
    the probe values and the targets' lengths, `slack` more)."""
    member = next(int(v[0]) for v in ix.lists if len(v))
    segs = [np.asarray(pv, dtype=np.uint32) for _, pv in queries]
    probe = np.concatenate([np.full(ptr0, member, np.uint32)] + segs + [np.full(5, member, np.uint32)])
    pp = ptr0 + np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    if cap is None:
        cap = sum(len(s) for s in segs) + sum(ix.lens[j] for j, _ in queries) + slack
    out, pidx, tpos = li.Guarded32(torch, cap), li.Guarded32(torch, cap), li.Guarded32(torch, cap)
    out_ptr = li.Guarded64(torch, len(queries) + 1)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.lists_union(li.dev8(torch, ix.packed, shift), li.dev64(torch, ix.offs if offs is None else offs), li.dev64(torch, ix.ptr),
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


def _check(ix, queries, r, ptr0=PTR0, positions=True):
    assert r["err"] == CLEAN
    vals, out_ptr, pidx, tpos = ur.want_union(ix, queries, ptr0)
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
    """a strictly ascending probe for list j: about `members` of its values and `others` values that are not in it"""
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
        queries = [(j, ur.edge_probe(ix, j)) for j in range(ix.nlists)]
        n = _check(ix, queries, _run(ix, queries, shift=shift))
        assert n > sum(ix.lens) + 2 * ix.nlists
    mx = ascending[0]
    assert {0, 5, 256, 257, 256 * 17 + 3} <= set(mx.lens)  # empty, tail only, one block, a block and one, a tail after full blocks


# ---- 2. mixed members and non-members --------------------------------------------------
def test_mixed_members_and_non_members(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(61)
    queries = [(j, _mixed(ix, j, rng)) for j in range(ix.nlists)]
    twice = ix.of_len(256 * 63 + 255)
    queries.append((twice, _mixed(ix, twice, rng)))  # the same list again, another probe
    empty = np.zeros(0, np.uint32)
    # an empty probe on a non-empty list (the result is the list), on an empty list, a probe on an empty list (the result is the probe)
    queries += [(0, empty), (twice, empty), (ix.of_len(0), empty), (3, empty), (ix.of_len(0), np.array([0, 7, 0xFFFFFFFF], np.uint32))]
    assert ix.lens[0] and ix.lens[3]
    queries = [queries[i] for i in rng.permutation(len(queries))]
    queries = [(1, empty)] + queries + [(2, empty), (2, empty)]  # empty segments first, last and in a row
    n = _check(ix, queries, _run(ix, queries))
    assert n > sum(ix.lens) + 30 * 10


def test_small_index_every_list(ascending):
    ix = ascending[1]
    rng = np.random.default_rng(3)
    queries = [(j, _mixed(ix, j, rng, 20, 50)) for j in (6, 5, 4, 3, 2, 1, 0, 2, 6)]
    _check(ix, queries, _run(ix, queries, shift=5))


# ---- 3. misses crowding into one unit and one position --------------------------------------
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
    queries = []
    for m in (65, 257, 1000):  # more than 64 and more than 256 misses in one unit, with the same L
        p, run = _gap_run(unit, m)
        queries.append((j, np.unique(np.concatenate([unit[max(p - 3, 0): p + 4], run]))))
    # misses spread over one unit: every gap of it gets one, next to the members
    spread = np.setdiff1d(unit[:-1] + 1, unit)
    assert len(spread) > 200
    queries.append((j, np.unique(np.concatenate([spread, unit[::3]]))))
    # the same in a p4Enc32 tail, after full blocks and alone
    tail = v[256 * 17:]
    queries.append((j, np.unique(np.concatenate([np.setdiff1d(tail[:-1] + 1, tail), tail[:1]]))))
    t = ix.lists[tailonly]
    p, run = _gap_run(t, 300)
    queries.append((tailonly, np.unique(np.concatenate([run, t[::5], np.setdiff1d(t[:-1] + 2, t)]))))
    # 3,000 misses with one L: all below the first value (L = 0), all past the last (L = n: no unit is decoded)
    assert int(v[0]) > 3000 and int(v[-1]) < 0xFFFFFFFF - 3000
    queries.append((j, np.arange(int(v[0]) - 3000, int(v[0]), dtype=np.uint32)))
    queries.append((j, np.arange(int(v[-1]) + 1, int(v[-1]) + 3001, dtype=np.uint32)))
    queries.append((tailonly, np.arange(int(t[-1]) + 1, int(t[-1]) + 3001, dtype=np.uint32)))
    # a probe that is exactly the list: no miss
    queries.append((j, v))
    queries.append((tailonly, t))
    _check(ix, queries, _run(ix, queries))


def test_dense_probe(ascending):
    ix = ascending[0]
    a, b = ix.of_len(256 * 64 + 1), ix.of_len(256 * 130 + 77)
    queries = [(b, ix.lists[a]), (a, ix.lists[b]), (b, ix.lists[b])]  # a whole list into the longer one, the reverse, and itself
    _check(ix, queries, _run(ix, queries))


# ---- 4. segment lengths -----------------------------------------------------------------
def test_segment_lengths(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(67)
    j, other = ix.of_len(256 * 17 + 3), ix.of_len(513)
    unit = ix.lists[j][256 * 5: 256 * 6]
    inside = np.setdiff1d(rng.integers(int(unit[0]), int(unit[-1]), size=400, dtype=np.uint64).astype(np.uint32), unit)
    queries = []
    for m in (1, 63, 64, 65, 257):  # 257: a segment across several 64-index runs
        half = min(m // 2 + 1, 200)
        pv = np.sort(np.concatenate([unit[rng.permutation(256)[:half]], inside[rng.permutation(len(inside))[:m - half]]]))
        assert len(pv) == m and (np.diff(pv.astype(np.int64)) > 0).all()
        queries += [(j, pv), (other, _mixed(ix, other, rng, 3, 3))]
    queries += [(int(rng.integers(0, ix.nlists)), _mixed(ix, j, rng, 2, 3)) for _ in range(20)]  # several queries in one 64-index run
    _check(ix, queries, _run(ix, queries))


def test_many_small_queries(ascending):
    """150 queries of 0 to 40 probe values: the unit runs of 16 span many queries, the tails kernel many waves."""
    ix = ascending[1]
    rng = np.random.default_rng(43)
    queries = []
    for _ in range(150):
        j = int(rng.integers(0, ix.nlists))
        m = int(rng.integers(0, 41))
        queries.append((j, _mixed(ix, j, rng, m // 2, m - m // 2)))
    _check(ix, queries, _run(ix, queries))


# ---- 5. chaining: a 3-term OR on the device --------------------------------------------------
def test_chained_three_term_or():
    rng = np.random.default_rng(73)
    common = np.unique(rng.integers(1, 1 << 28, size=3000, dtype=np.uint64))
    lists = [np.unique(np.concatenate([common, rng.integers(1, 1 << 28, size=n, dtype=np.uint64)])).astype(np.uint32)
             for n in (5000, 9000, 14000)]
    ix = Index(None, rng, ptr0=7, start0=np.zeros(3, np.uint32), lists=lists)
    assert ix.ascends()
    want = np.union1d(np.union1d(lists[0], lists[1]), lists[2])
    packed, offs, ptr, base = li.dev8(torch, ix.packed), li.dev64(torch, ix.offs), li.dev64(torch, ix.ptr), li.dev32(torch, ix.base)
    table, st = li.dev32(torch, ix.table), li.dev32(torch, ix.start0)
    n0, n1, n2 = (len(v) for v in lists)
    err = torch.zeros(4, dtype=torch.int64, device=DEV)
    # the first probe is a selective decode; nothing comes back to the host between the calls
    out0, ptr0 = tpf.decn256v32_lists_select(packed, offs, ptr, base, li.dev32(torch, [0]), d1=True, start0=st,
                                             out=torch.empty(n0, dtype=torch.int32, device=DEV), err=err[0:1])
    out1, ptr1 = tpf.lists_union(packed, offs, ptr, base, table, out0, ptr0, li.dev32(torch, [1]), start0=st,
                                 out=torch.empty(n0 + n1, dtype=torch.int32, device=DEV), err=err[1:2])
    pidx2 = torch.empty(n0 + n1 + n2, dtype=torch.int32, device=DEV)
    tpos2 = torch.empty(n0 + n1 + n2, dtype=torch.int32, device=DEV)
    out2, ptr2 = tpf.lists_union(packed, offs, ptr, base, table, out1, ptr1, li.dev32(torch, [2]), start0=st,
                                 out=torch.empty(n0 + n1 + n2, dtype=torch.int32, device=DEV), pidx=pidx2, tpos=tpos2, err=err[2:3])
    hits, hptr = tpf.lists_intersect(packed, offs, ptr, base, table, out0, ptr0, li.dev32(torch, [1]), start0=st, err=err[3:4])
    assert err.tolist() == [CLEAN] * 4
    m1, m2 = int(ptr1[1].item()), int(ptr2[1].item())
    assert ptr1[0].item() == 0 and ptr2[0].item() == 0
    assert m1 == n0 + n1 - int(hptr[1].item()) == len(np.union1d(lists[0], lists[1]))
    assert np.array_equal(out1.cpu().numpy().view(np.uint32)[:m1], np.union1d(lists[0], lists[1]))
    got = out2.cpu().numpy().view(np.uint32)[:m2]
    assert np.array_equal(got, want)
    tp = tpos2.cpu().numpy().view(np.uint32)[:m2]
    pi = pidx2.cpu().numpy().view(np.uint32)[:m2]
    assert np.array_equal(got[tp != ur.NONE], lists[2]) and np.array_equal(tp[tp != ur.NONE], np.arange(n2))
    assert np.array_equal(pi[pi != ur.NONE], np.arange(m1))  # every value of the probe, in order


# ---- 6. the optional outputs -----------------------------------------------------------------
def test_without_positions(ascending):
    ix = ascending[1]
    rng = np.random.default_rng(79)
    queries = [(j, _mixed(ix, j, rng, 30, 30)) for j in (0, 2, 3, 6, 4, 1, 2, 0)]
    _check(ix, queries, _run(ix, queries, positions=False), positions=False)


# ---- 7. refusals ------------------------------------------------------------------------------
def _eight(ix, rng):
    """8 queries over SMALL; query 3 is the only one that names list 6 (the last list of the directory)"""
    return [(j, _mixed(ix, j, rng, 6, 4)) for j in (0, 2, 3, 6, 4, 1, 2, 0)]


@pytest.mark.parametrize("what", ["nlists", "ffffffff", "descending", "past_probe", "past_probe_last", "directory", "units"])
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
    elif what == "directory":
        base = ix.base.copy()
        assert base[7] == ix.nunits
        base[7] = ix.nunits + 1
        kw = dict(base=base)
    else:
        base = ix.base.copy()  # list 2 gets a unit of list 3: both unit counts disagree with the lengths, query 1 names list 2
        base[3] += 1
        kw, k = dict(base=base), 1
    r = _run(ix, queries, **kw)
    assert r["err"] == ix.nunits + k
    _untouched(r)


def test_capacity_one_short(ascending):
    ix = ascending[1]
    queries = _eight(ix, np.random.default_rng(79))
    vals, out_ptr, _, _ = ur.want_union(ix, queries, PTR0)
    r = _run(ix, queries, cap=len(vals) - 1)
    assert r["err"] == ix.nunits + len(queries)
    _untouched(r, out_ptr_too=False)
    assert np.array_equal(r["out_ptr"], out_ptr)  # complete and correct: out_ptr[nq] is what to allocate
    _check(ix, queries, _run(ix, queries, cap=len(vals)))


def test_nq_zero(ascending):
    r = _run(ascending[1], [], cap=4)
    assert r["err"] == CLEAN and r["out_ptr"].tolist() == [0]
    _untouched(r, out_ptr_too=False)


@pytest.mark.parametrize("tail", [False, True])
def test_corrupted_block(ascending, tail):
    """Every unit of a targeted list is decoded: its corrupted offset is reported by its source unit, and all stays in bounds."""
    ix = ascending[1]
    j, i = (2, 2) if tail else (6, 9)  # the tail of the 612-value list; unit 9 of the 17-unit list
    u = int(ix.base[j]) + i
    offs = ix.offs.copy()
    offs[u + 1] += 1  # its end offset, the start of the unit after it, moves by one
    rng = np.random.default_rng(83)
    queries = [(0, _mixed(ix, 0, rng, 5, 5)), (4, _mixed(ix, 4, rng, 5, 5)), (j, _mixed(ix, j, rng, 20, 20))]
    r = _run(ix, queries, offs=offs)
    assert r["err"] == u
    _, out_ptr, _, _ = ur.want_union(ix, queries, PTR0)
    assert r["out_ptr"][0] == 0 and len(r["out_ptr"]) == len(out_ptr)
    # a list that is not targeted leaves the call clean and exact: list 3 follows the 612-value list, list 6 is the last
    clean = [(0, queries[0][1]), (4, queries[1][1])]
    _check(ix, clean, _run(ix, clean, offs=offs))


# ---- 8. outside the precondition: in bounds, and d_out_ptr as defined ----------------------------
def _in_bounds(ix, queries, r):
    op = r["out_ptr"]
    assert op[0] == 0
    for k, (j, pv) in enumerate(queries):
        assert ix.lens[j] <= op[k + 1] - op[k] <= ix.lens[j] + len(pv), k
    n = int(op[-1])
    for name in ("out", "pidx", "tpos"):
        assert (r[name][n:] == SENT).all(), name


def test_wrapping_target():
    rng = np.random.default_rng(23)
    ix = Index([256 * 20 + 5, 300, 256 * 3], rng, start0=np.array([(1 << 32) - 40000, 7, (1 << 32) - 3000000], np.uint32), start_bits=32)
    assert int(ix.lists[0][-1]) < int(ix.lists[0][0]) and int(ix.lists[2][-1]) < int(ix.lists[2][0])  # wrapped
    queries = []
    for j in (0, 2, 1, 0):
        v = ix.lists[j]
        pv = np.concatenate([v[rng.permutation(len(v))[:80]], rng.integers(0, 1 << 32, size=40, dtype=np.uint64).astype(np.uint32),
                             np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)])
        queries.append((j, np.unique(pv)))
    r = _run(ix, queries)
    assert r["err"] == CLEAN
    _in_bounds(ix, queries, r)
    # the list that does not wrap is answered exactly
    k = 2
    a, b = int(r["out_ptr"][k]), int(r["out_ptr"][k + 1])
    assert np.array_equal(r["out"][a:b], np.union1d(ix.lists[1], queries[k][1]))


def test_random_table(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(89)
    queries = [(j, _mixed(ix, j, rng, 60, 60)) for j in range(ix.nlists)]
    r = _run(ix, queries, table=rng.integers(0, 1 << 32, size=ix.nunits, dtype=np.uint64).astype(np.uint32))
    assert r["err"] == CLEAN
    _in_bounds(ix, queries, r)


def test_unsorted_probe_with_repeats(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(71)
    queries = []
    for j in (ix.of_len(256 * 17 + 3), ix.of_len(257), ix.of_len(256 * 64), ix.of_len(0), ix.of_len(5)):
        pv = _mixed(ix, j, rng, 60, 300)
        pv = np.concatenate([pv, pv[rng.permutation(len(pv))[:100]], pv[:5]])
        queries.append((j, pv[rng.permutation(len(pv))]))
    r = _run(ix, queries)
    assert r["err"] == CLEAN
    _in_bounds(ix, queries, r)
    # d_out_ptr is as defined: n_j + the probe values (every occurrence) that are not in the list
    want = np.cumsum([0] + [ix.lens[j] + int((~np.isin(pv, ix.lists[j])).sum()) for j, pv in queries])
    assert np.array_equal(r["out_ptr"], want)


# ---- 9. the work does not depend on the rest of the index -----------------------------------------
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
