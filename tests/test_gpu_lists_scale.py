"""GPU checks of the lists entry points (include/turbopfor_gpu.h) past one grid:
more lists, units, selections, queries and request values than the capped plan
and heads kernels have threads (flat_grid, csrc/p4_lists_host.h), more items
than one trip of the item decodes k_ix_dec / k_ga_dec covers, and more lists
than three steps of find_list resolve.  The sizes come from the caps the
binding restates (turbopfor_amd.lists_flat_cap / lists_item_cap, held against
the sources by tests/test_lists_scale_cpu.py) on the device the test runs on,
and every test asserts that the count it means to cross is crossed.

The many-lists index is tests/lists_scale.py's concatenation of oracle-composed
kinds; the expected results are its whole-request numpy statements of the
definitions or direct indexing into the original values -- never the code
under test -- and every comparison is bit for bit."""
import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
import lists_scale as sc
from lists_index import CLEAN, DEV, SENT, SENT64

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
PTR0 = 3   # request entries before the first segment ...
TRAIL = 5  # ... and after the last: never to be read
SLACK = 91


def _caps():
    return tpf.lists_flat_cap(DEV), tpf.lists_item_cap(DEV)


def _over(cap, extra):
    """cap + extra, the remainder no multiple of 256 (nor, then, of a grid of 256-thread workgroups)"""
    n = cap + extra
    return n + 1 if (n - cap) % 256 == 0 else n


class Resident:
    """The device tensors of one stream of an index."""

    def __init__(self, ix, packed, offs, d1):
        self.ix, self.d1 = ix, d1
        self.packed, self.offs = li.dev8(torch, packed), li.dev64(torch, offs)
        self.ptr, self.base = li.dev64(torch, ix.ptr), li.dev32(torch, ix.base)
        self.start0 = li.dev32(torch, ix.start0) if d1 else None
        self.table = li.dev32(torch, ix.table) if d1 else None


def _sentinel32(n):
    """n values inside a sentinel-filled buffer -> (whole buffer, view)"""
    big = torch.full((n + 2 * SLACK,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    return big, big[SLACK: SLACK + n]


def _read32(big, n):
    """-> (the n values, every value around them is still the sentinel)"""
    got = big.cpu().numpy().view(np.uint32)
    return got[SLACK: SLACK + n], bool((got[:SLACK] == SENT).all() and (got[SLACK + n:] == SENT).all())


def _err():
    return torch.zeros(1, dtype=torch.int64, device=DEV)


# ---- a. many lists --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many():
    """An index of more lists than max(lists_flat_cap, 64^3), and more units than lists_flat_cap, with both streams resident."""
    flat, _ = _caps()
    rng = np.random.default_rng(101)
    kinds = sc.Kinds(rng)
    n = _over(max(flat, 64 ** 3), 70001)
    ix = sc.ScaleIndex(kinds, kinds.choose(rng, n), ptr0=37)
    return ix, {d1: Resident(ix, *ix.stream(d1), d1) for d1 in (False, True)}


def _assert_many(ix):
    flat, _ = _caps()
    assert ix.nlists > flat and ix.nunits > flat  # a second trip over the lists, and over the unit records k_lists_plan clears
    assert ix.nlists > 64 ** 3                    # a fourth step of find_list
    assert (ix.nlists - flat) % 256 != 0          # the last trip is partial
    assert len(ix.vals) < 8 << 20


@pytest.mark.parametrize("d1", [False, True])
def test_many_lists_decode(many, d1):
    ix, res = many
    _assert_many(ix)
    R = res[d1]
    cap, lo = int(ix.ptr[-1]), int(ix.ptr[0])
    big = torch.full((cap + SLACK,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    err = _err()
    tpf.decn256v32_lists(R.packed, R.offs, R.ptr, d1=d1, start0=R.start0, out=big[:cap], err=err)
    got = big.cpu().numpy().view(np.uint32)
    assert int(err.item()) == CLEAN
    assert np.array_equal(got[lo:cap], ix.vals)
    assert (got[:lo] == SENT).all() and (got[cap:] == SENT).all()


@pytest.mark.parametrize("d1", [False, True])
def test_many_lists_encode(many, d1):
    ix, res = many
    _assert_many(ix)
    R = res[d1]
    packed, offs = ix.stream(d1)
    lo = int(ix.ptr[0])
    values = li.dev32(torch, np.concatenate([np.full(lo, 0xDEADBEEF, np.uint32), ix.vals]))
    cap = len(packed) + 64  # the bound is advice: the device holds the real length against the capacity
    big = torch.full((SLACK + cap + SLACK,), 0xA5, dtype=torch.uint8, device=DEV)
    d_offs = torch.full((ix.nunits + 1 + 16,), SENT64, dtype=torch.int64, device=DEV)
    err = _err()
    tpf.encn256v32_lists(values, R.ptr, d1=d1, start0=R.start0, nunits=ix.nunits, out=big[SLACK: SLACK + cap],
                         offsets=d_offs[8: 8 + ix.nunits + 1], err=err)
    got, got_offs = big.cpu().numpy(), d_offs.cpu().numpy()
    assert int(err.item()) == CLEAN
    assert np.array_equal(got_offs[8: 8 + ix.nunits + 1].view(np.uint64), offs)
    assert (got_offs[:8] == SENT64).all() and (got_offs[8 + ix.nunits + 1:] == SENT64).all()
    assert np.array_equal(got[SLACK: SLACK + len(packed)], packed)
    assert (got[:SLACK] == 0xA5).all() and (got[SLACK + len(packed):] == 0xA5).all()


def test_many_lists_directory_and_skip_table(many):
    ix, res = many
    _assert_many(ix)
    R = res[True]
    big, view = _sentinel32(ix.nlists + 1)
    err = _err()
    tpf.lists_unit_base(R.ptr, out=view, err=err)
    got, ok = _read32(big, ix.nlists + 1)
    assert int(err.item()) == CLEAN and ok
    assert np.array_equal(got, ix.base)
    big, view = _sentinel32(ix.nunits)
    tpf.lists_unit_last(R.packed, R.offs, R.ptr, start0=R.start0, out=view, err=err)
    got, ok = _read32(big, ix.nunits)
    assert int(err.item()) == CLEAN and ok
    assert np.array_equal(got, ix.table)


def test_many_lists_refused_structure_past_the_cap(many):
    """list_ptr decreases at a list index the first trip of the plan does not reach: reported as nunits + j, nothing written."""
    ix, res = many
    flat, _ = _caps()
    R = res[False]
    j = flat + 1234
    assert j + 1 < ix.nlists
    bad = ix.ptr.copy()
    bad[j + 1] = bad[j] - 1
    d_bad = li.dev64(torch, bad)
    cap = int(ix.ptr[-1])
    big = torch.full((cap + SLACK,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    err = _err()
    tpf.decn256v32_lists(R.packed, R.offs, d_bad, out=big[:cap], err=err)
    assert int(err.item()) == ix.nunits + j
    assert bool((big == SENT - (1 << 32)).all())
    big, view = _sentinel32(ix.nlists + 1)
    tpf.lists_unit_base(d_bad, out=view, err=err)
    got, ok = _read32(big, ix.nlists + 1)
    assert int(err.item()) == j and ok and (got == SENT).all()


# ---- b. many selections -----------------------------------------------------------------------------
def _selections(ix, rng):
    """More selections than lists_flat_cap, in random order with repeats and empty lists; ranges: whole lists, and sub-ranges
    of about half the multi-unit ones."""
    flat, _ = _caps()
    nsel = _over(flat, 50001)
    sel = rng.integers(0, ix.nlists, size=nsel)
    sel[rng.permutation(nsel)[:600]] = rng.choice(np.nonzero(ix.units > 1)[0], size=600)
    units = ix.units[sel]
    uc = np.where((units > 1) & (rng.random(nsel) < 0.5), (rng.random(nsel) * (units + 1)).astype(np.int64), units)
    uf = (rng.random(nsel) * (units - uc + 1)).astype(np.int64)
    assert nsel > flat and (nsel - flat) % 256 != 0
    assert len(np.unique(sel)) < nsel and (ix.lens[sel] == 0).sum() > 1000
    assert ((uc < units) & (uc > 0)).sum() > 300 and ((uf > 0) & (uf + uc == units) & (ix.lens[sel] % 256 != 0)).sum() > 30
    return sel, uf, uc


def _decode_selection(R, sel, ranges, total):
    """the selective decode (ranges None) or the units decode into `total` guarded values -> (values, guards intact, out_ptr, err)"""
    nsel = len(sel)
    big, view = _sentinel32(total)
    d_ptr = torch.full((nsel + 1 + 16,), SENT64, dtype=torch.int64, device=DEV)
    err = _err()
    if ranges is None:
        tpf.decn256v32_lists_select(R.packed, R.offs, R.ptr, R.base, li.dev32(torch, sel), d1=R.d1, start0=R.start0, out=view,
                                    out_ptr=d_ptr[8: 8 + nsel + 1], err=err)
    else:
        tpf.decn256v32_lists_units(R.packed, R.offs, R.ptr, R.base, li.dev32(torch, sel), li.dev32(torch, ranges[0]),
                                   li.dev32(torch, ranges[1]), d1=R.d1, start0=R.start0, unit_last=R.table, out=view,
                                   out_ptr=d_ptr[8: 8 + nsel + 1], err=err)
    got, ok = _read32(big, total)
    p = d_ptr.cpu().numpy()
    ok = ok and bool((p[:8] == SENT64).all() and (p[8 + nsel + 1:] == SENT64).all())
    return got, ok, p[8: 8 + nsel + 1], int(err.item())


@pytest.mark.parametrize("d1", [False, True])
def test_many_selections(many, d1):
    ix, res = many
    flat, _ = _caps()
    sel, uf, uc = _selections(ix, np.random.default_rng(103))
    for ranges, (want, want_ptr) in ((None, sc.want_select(ix, sel)), ((uf, uc), sc.want_units(ix, sel, uf, uc))):
        got, ok, out_ptr, err = _decode_selection(res[d1], sel, ranges, len(want))
        assert err == CLEAN and ok
        assert np.array_equal(out_ptr, want_ptr)
        assert np.array_equal(got, want)
        assert len(want) // 256 + len(sel) > flat  # the records of the virtual units the plan clears: a second trip too
    # a bad list id in a selection past the cap
    k = flat + 777
    bad = sel.copy()
    bad[k] = ix.nlists
    for ranges in (None, (uf, uc)):
        got, ok, out_ptr, err = _decode_selection(res[d1], bad, ranges, 4096)
        assert err == ix.nunits + k and ok
        assert (got == SENT).all() and (out_ptr == SENT64).all()


def test_many_range_queries(many):
    import test_gpu_lists_units as units_tests  # its _want_range is the statement of the definition

    ix, res = many
    flat, _ = _caps()
    R = res[True]
    rng = np.random.default_rng(107)
    nq = _over(flat, 50001)
    qlist = rng.integers(0, ix.nlists, size=nq)
    qlist[rng.permutation(nq)[:3000]] = rng.choice(np.nonzero(ix.units > 1)[0], size=3000)
    n = ix.lens[qlist]
    at = sc.rel(ix)[qlist] + (rng.random(nq) * n).astype(np.int64)
    c = np.where(n > 0, ix.vals[np.minimum(at, len(ix.vals) - 1)].astype(np.int64), rng.integers(0, 1 << 32, size=nq))
    lo = np.clip(c + rng.integers(-3, 4, size=nq) - rng.choice([0, 1, 3000, 1 << 21], size=nq), 0, 0xFFFFFFFF)
    hi = np.clip(c + rng.integers(-3, 4, size=nq) + rng.choice([-5, 0, 1, 3000, 1 << 21], size=nq), 0, 0xFFFFFFFF)
    assert nq > flat and (nq - flat) % 256 != 0 and (lo > hi).sum() > 1000
    want_uf, want_uc = sc.want_range(ix, qlist, lo, hi)
    assert (want_uc == 0).sum() > 1000 and (want_uc > 1).sum() > 300
    # the whole-request statement is the per-query one of tests/test_gpu_lists_units.py: a sample on both sides of the cap
    for k in np.concatenate([rng.integers(0, flat, size=500), rng.integers(flat, nq, size=500), np.nonzero(want_uc > 1)[0][:200]]):
        assert units_tests._want_range(ix, int(qlist[k]), int(lo[k]), int(hi[k])) == (want_uf[k], want_uc[k])
    ubig, uview = _sentinel32(nq)
    cbig, cview = _sentinel32(nq)
    err = _err()
    tpf.lists_range_units(R.base, R.table, li.dev32(torch, qlist), li.dev32(torch, lo), li.dev32(torch, hi), ufirst=uview, ucount=cview, err=err)
    (uf, ok1), (uc, ok2) = _read32(ubig, nq), _read32(cbig, nq)
    assert int(err.item()) == CLEAN and ok1 and ok2
    assert np.array_equal(uf, want_uf) and np.array_equal(uc, want_uc)


# ---- c. many queries and many values: intersect and gather ----------------------------------------------
@pytest.fixture(scope="module")
def matrix():
    """The shape-matrix index, ascending, with its plain twin; both resident."""
    rng = np.random.default_rng(117)
    ix = li.Index([ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))], rng, ptr0=37, start_bits=31)
    assert ix.ascends()
    tw = sc.Twin(ix, rng)
    return ix, tw, {True: Resident(ix, ix.packed, ix.offs, True), False: Resident(ix, tw.fpacked, tw.foffs, False)}


def _lay(segs_len, lead, fill, flat_values):
    """the request array: PTR0 leading entries, the segments, TRAIL trailing entries -> (array, CSR pointers)"""
    pp = PTR0 + sc._starts(segs_len)
    return np.concatenate([np.full(PTR0, lead, np.uint32), flat_values.astype(np.uint32), np.full(TRAIL, fill, np.uint32)]), pp


def _intersect(R, qlist, pp, probe):
    cap = len(probe)
    out, pidx, tpos = (_sentinel32(cap) for _ in range(3))
    nq = len(qlist)
    d_ptr = torch.full((nq + 1 + 16,), SENT64, dtype=torch.int64, device=DEV)
    err = _err()
    tpf.lists_intersect(R.packed, R.offs, R.ptr, R.base, R.table, li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist),
                        start0=R.start0, out=out[1], out_ptr=d_ptr[8: 8 + nq + 1], pidx=pidx[1], tpos=tpos[1], err=err)
    r = dict(err=int(err.item()))
    for name, (big, _) in (("out", out), ("pidx", pidx), ("tpos", tpos)):
        r[name], ok = _read32(big, cap)
        assert ok, name + ": a value outside the buffer was written"
    p = d_ptr.cpu().numpy()
    assert (p[:8] == SENT64).all() and (p[8 + nq + 1:] == SENT64).all(), "out_ptr: a value outside the buffer was written"
    r["out_ptr"] = p[8: 8 + nq + 1]
    return r


def _check_hits(ix, qlist, pp, probe, r):
    assert r["err"] == CLEAN
    vals, out_ptr, pidx, tpos = sc.want_hits(ix, qlist, pp, probe)
    n = len(vals)
    assert np.array_equal(r["out_ptr"], out_ptr)
    assert np.array_equal(r["out"][:n], vals)
    assert np.array_equal(r["pidx"][:n], pidx) and np.array_equal(r["tpos"][:n], tpos)
    for name in ("out", "pidx", "tpos"):
        assert (r[name][n:] == SENT).all(), name
    return n


def _gather(R, qlist, pp, pos):
    big, view = _sentinel32(len(pos))
    err = _err()
    tpf.lists_gather(R.packed, R.offs, R.ptr, R.base, li.dev32(torch, pos), li.dev64(torch, pp), li.dev32(torch, qlist), d1=R.d1,
                     start0=R.start0, unit_last=R.table, out=view, err=err)
    got, ok = _read32(big, len(pos))
    assert ok, "a value outside d_out was written"
    return got, int(err.item())


def _check_gather(ix, values, qlist, pp, pos, got, err):
    assert err == CLEAN
    a, b = int(pp[0]), int(pp[-1])
    assert np.array_equal(got[a:b], sc.want_gather(ix.ptr, values, qlist, pp, pos))
    assert (got[:a] == SENT).all() and (got[b:] == SENT).all()  # parallel to d_pos: nothing outside the segments


def _sorted_in_queries(counts, values):
    """values, sorted inside every query of `counts` values"""
    q = np.repeat(np.arange(len(counts), dtype=np.uint64), counts)
    return values[np.argsort((q << np.uint64(32)) | values.astype(np.uint64), kind="stable")]


def _small_queries(ix, rng):
    """more queries than lists_flat_cap, 0 to 2 request values each -> (qlist, values per query)"""
    flat, _ = _caps()
    nq = _over(flat, 60011)  # about one value per query, a seventeenth of them on the empty list: more values than the cap as well
    qlist = rng.integers(0, ix.nlists, size=nq)
    counts = rng.integers(0, 3, size=nq)
    assert nq > flat and (nq - flat) % 256 != 0 and counts.sum() > flat
    return qlist, counts


def test_many_small_queries_intersect(matrix):
    ix, _, res = matrix
    flat, _ = _caps()
    rng = np.random.default_rng(109)
    qlist, counts = _small_queries(ix, rng)
    ql = np.repeat(qlist, counts)
    n, r0 = np.asarray(ix.lens)[ql], sc.rel(ix)[ql]
    member = ix.vals[np.minimum(r0 + (rng.random(len(ql)) * n).astype(np.int64), len(ix.vals) - 1)]
    last = np.where(n > 0, ix.vals[np.maximum(r0 + n - 1, 0)].astype(np.int64), 1 << 31)
    lo = np.maximum(ix.start0[ql].astype(np.int64) - 20000, 0)
    other = (lo + rng.random(len(ql)) * (last + 20000 - lo)).astype(np.int64).clip(0, 0xFFFFFFFF).astype(np.uint32)
    values = np.where((n > 0) & (rng.random(len(ql)) < 0.5), member, other)
    probe, pp = _lay(counts, ix.vals[0], ix.vals[0], _sorted_in_queries(counts, values))
    r = _intersect(res[True], qlist, pp, probe)
    hits = _check_hits(ix, qlist, pp, probe, r)
    assert 0.3 * len(ql) < hits < 0.7 * len(ql)
    # a refused query at an index past the cap: the documented code, nothing written
    k = len(qlist) - 5
    assert k > flat
    bad = qlist.copy()
    bad[k] = ix.nlists
    r = _intersect(res[True], bad, pp, probe)
    assert r["err"] == ix.nunits + k
    assert (r["out"] == SENT).all() and (r["pidx"] == SENT).all() and (r["tpos"] == SENT).all() and (r["out_ptr"] == SENT64).all()


def test_many_values_intersect(matrix):
    """A handful of queries that total more probe values than lists_flat_cap."""
    ix, _, res = matrix
    flat, _ = _caps()
    rng = np.random.default_rng(113)
    targets = [ix.of_len(n) for n in (256 * 130 + 77, 256 * 64 + 1, 256 * 63 + 255, 257, 256 * 130 + 77)]
    each = flat // len(targets) + 1013
    segs = []
    for k, j in enumerate(targets):
        v = ix.lists[j]
        at = int(v[int(rng.integers(0, len(v) // 2))]) - 5
        m = each + (k == 0 and (len(targets) * each - flat) % 256 == 0)  # the total past the cap is no multiple of 256
        run = np.arange(at, at + m - len(v), dtype=np.int64).astype(np.uint32)  # consecutive integers across a few units ...
        segs.append(np.sort(np.concatenate([run, v])))                              # ... and every member, some of them twice
    counts = np.array([len(s) for s in segs])
    probe, pp = _lay(counts, ix.vals[0], ix.vals[0], np.concatenate(segs))
    assert counts.sum() > flat and (counts.sum() - flat) % 256 != 0
    r = _intersect(res[True], np.asarray(targets), pp, probe)
    assert _check_hits(ix, np.asarray(targets), pp, probe, r) > sum(ix.lens[j] for j in targets)


@pytest.mark.parametrize("d1", [True, False])
def test_many_small_queries_gather(matrix, d1):
    ix, tw, res = matrix
    flat, _ = _caps()
    values = tw.stream(d1)[2]
    rng = np.random.default_rng(127)
    qlist, counts = _small_queries(ix, rng)
    counts = np.where(np.asarray(ix.lens)[qlist] > 0, counts, 0)  # an empty list has no position
    ql = np.repeat(qlist, counts)
    positions = _sorted_in_queries(counts, (rng.random(len(ql)) * np.asarray(ix.lens)[ql]).astype(np.uint32))
    pos, pp = _lay(counts, 0xFFFFFFFF, 0xFFFFFFFF, positions)
    assert counts.sum() > flat
    got, err = _gather(res[d1], qlist, pp, pos)
    _check_gather(ix, values, qlist, pp, pos, got, err)
    # a refused query, then a refused position, at indices past the cap: the documented codes, nothing written
    nq = len(qlist)
    k = nq - 7
    bad = qlist.copy()
    bad[k] = ix.nlists
    got, err = _gather(res[d1], bad, pp, pos)
    assert k > flat and err == ix.nunits + k and (got == SENT).all()
    i = int(pp[-1]) - 11
    badpos = pos.copy()
    badpos[i] = ix.lens[int(ql[i - PTR0])]  # one past its list's last position
    got, err = _gather(res[d1], qlist, pp, badpos)
    assert i > flat and err == ix.nunits + nq + i and (got == SENT).all()


@pytest.mark.parametrize("d1", [True, False])
def test_many_values_gather(matrix, d1):
    """A handful of queries that total more positions than lists_flat_cap."""
    ix, tw, res = matrix
    flat, _ = _caps()
    values = tw.stream(d1)[2]
    targets = np.asarray([ix.of_len(n) for n in (256 * 130 + 77, 256 * 64 + 1, 256 * 63 + 255, 257, 256 * 130 + 77)])
    each = flat // len(targets) + 1013
    segs = [np.arange(each, dtype=np.int64) * ix.lens[j] // each for j in targets]  # every position or every few, in order, with repeats
    if (len(targets) * each - flat) % 256 == 0:
        segs[0] = np.concatenate([[0], segs[0]])  # the total past the cap is no multiple of 256
    counts = np.array([len(s) for s in segs])
    pos, pp = _lay(counts, 0xFFFFFFFF, 0xFFFFFFFF, np.concatenate(segs))
    assert counts.sum() > flat and (counts.sum() - flat) % 256 != 0
    got, err = _gather(res[d1], targets, pp, pos)
    _check_gather(ix, values, targets, pp, pos, got, err)


# ---- d. the item stride of k_ix_dec and k_ga_dec ---------------------------------------------------------
TAIL_ONLY = [5, 90, 200, 131]
LONG = 256 * 300 + 77


@pytest.fixture(scope="module")
def strided():
    """One list of 300 full blocks and a tail, four tail-only lists and the shape matrix; ascending, with its plain twin."""
    rng = np.random.default_rng(131)
    lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
    lens = lens[:6] + [LONG] + lens[6:] + TAIL_ONLY
    ix = li.Index(lens, rng, ptr0=11, start_bits=31)
    assert ix.ascends()
    tw = sc.Twin(ix, rng)
    return ix, tw, {True: Resident(ix, ix.packed, ix.offs, True), False: Resident(ix, tw.fpacked, tw.foffs, False)}


def _stride_queries(ix, rng):
    """Queries of one request value per unit: the long list's 300 full blocks
    again and again, until the full-block items exceed lists_item_cap by a
    quarter; groups of 8 tail-only queries, neighbours on different lists, near
    the start, around the cap and near the end (any 8 consecutive items hold an
    aligned run of 4); matrix lists in between.  -> (qlist, list-relative unit
    of every request value, values per query)"""
    _, icap = _caps()
    long_j = ix.of_len(LONG)
    tails = [ix.of_len(n) for n in TAIL_ONLY]
    target = icap + icap // 4 + 3
    nlong = -(-target // 300)
    groups = {2, max(icap // 300 - 8, 3), icap // 300 + 2, nlong - 2}
    qlist, units = [], []
    left = target
    for g in range(nlong):
        m = min(300, left)
        left -= m
        qlist.append(long_j)
        units.append(np.arange(m))
        if g in groups:
            for t in range(8):
                qlist.append(tails[t % 4])
                units.append(np.zeros(1, np.int64))
        if g % 9 == 4:
            j = int(rng.integers(0, len(ref.MATRIX)))
            j += j >= long_j  # the matrix lists lie around the long one
            if ix.lens[j]:
                qlist.append(j)
                units.append(np.arange(ix.units(j)))
    counts = np.array([len(u) for u in units])
    return np.asarray(qlist), np.concatenate(units), counts


def _assert_item_stride(ix, ql, units_abs):
    """The items of the request, computed from its own lists and units: more
    full-block items than one trip covers, a partial last trip, and runs of a
    wave's 4 items that are all tails on both sides of the cap."""
    _, icap = _caps()
    heads = sc.item_heads(ql, units_abs)
    tails = sc.tail_units(ix)[units_abs[heads]]
    nitems = len(heads)
    assert (~tails).sum() > icap + icap // 5 and nitems % icap != 0 and nitems < 2 * icap
    runs = np.nonzero(tails[: nitems // 4 * 4].reshape(-1, 4).all(axis=1))[0] * 4
    assert (runs < icap).any() and (runs >= icap).any()  # the `continue` of a run of tails only, in the first trip and in the second
    assert tpf.LISTS_IX_RUN == tpf.LISTS_GA_RUN == 4
    return nitems


def test_item_stride_intersect(strided):
    ix, _, res = strided
    rng = np.random.default_rng(137)
    qlist, urel, counts = _stride_queries(ix, rng)
    ql = np.repeat(qlist, counts)
    r0, n = sc.rel(ix)[ql], np.asarray(ix.lens)[ql]
    cnt = np.minimum(256, n - 256 * urel)  # values in the unit
    inside = np.where(cnt > 1, 1 + (rng.random(len(ql)) * (cnt - 1)).astype(np.int64), 0)
    at = r0 + 256 * urel + inside
    member = ix.vals[at].astype(np.int64)
    # about half members; the others one below a member, above the value before it: a non-member inside the unit's range
    gap = (inside > 0) & (member - ix.vals[np.maximum(at - 1, 0)] > 1)
    values = np.where(gap & (rng.random(len(ql)) < 0.5), member - 1, member).astype(np.uint32)
    probe, pp = _lay(counts, ix.vals[0], ix.vals[0], values)
    units_abs = sc.probe_units(ix, ql, values)
    assert np.array_equal(units_abs, ix.base[ql].astype(np.int64) + urel)  # every value lands in the unit it was made for
    nitems = _assert_item_stride(ix, ql, units_abs)
    assert nitems == len(ql)  # one item per probe value
    r = _intersect(res[True], qlist, pp, probe)
    hits = _check_hits(ix, qlist, pp, probe, r)
    assert 0.4 * len(ql) < hits < 0.7 * len(ql)


@pytest.mark.parametrize("d1", [True, False])
def test_item_stride_gather(strided, d1):
    ix, tw, res = strided
    rng = np.random.default_rng(139)
    qlist, urel, counts = _stride_queries(ix, rng)
    ql = np.repeat(qlist, counts)
    cnt = np.minimum(256, np.asarray(ix.lens)[ql] - 256 * urel)
    positions = 256 * urel + (rng.random(len(ql)) * cnt).astype(np.int64)
    pos, pp = _lay(counts, 0xFFFFFFFF, 0xFFFFFFFF, positions)
    _assert_item_stride(ix, ql, ix.base[ql].astype(np.int64) + (positions >> 8))
    got, err = _gather(res[d1], qlist, pp, pos)
    _check_gather(ix, tw.stream(d1)[2], qlist, pp, pos, got, err)
