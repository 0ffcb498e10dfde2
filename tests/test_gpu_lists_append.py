"""GPU checks of the append to a resident index (include/turbopfor_gpu.h
tpf_lists_append): the result must be byte for byte, offset for offset and
table for table what the encoder writes for the concatenated lists.  The old
index and the expected new one are both the oracle's composition
(tests/lists_ref.py) -- of the old lists and of old ++ added -- and the skip
tables are built from their definition (the last value of every unit), never
from the code under test.  Every output lies in a sentinel-filled buffer and
the C entry point is called directly, so that the tables are guarded too."""
import ctypes

import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
from lists_index import CLEAN, DEV, SENT, SENT64

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
OLD = [0, 1, 255, 256, 257, 511, 512, 513, 256 * 17 + 3]
ADD = [0, 1, 255, 256, 257, 600]
SENT8 = 0xA5
PTR0, APTR0, ATRAIL = 37, 5, 7  # d_list_ptr[0], d_add_ptr[0], unread values after the additions


def _table(lists):
    return np.array([v[min(256 * (i + 1), len(v)) - 1] for v in lists for i in range(ref.n_units(len(v)))], dtype=np.uint32)


class Case:
    """Old lists of the lengths `olds` (the old index has len(olds) lists), additions of the lengths `adds` (len(adds) >=
    len(olds)), both cut from one value sequence per list so that the concatenation is a proper list."""

    def __init__(self, olds, adds, d1, rng, start0=True, ptr0=PTR0, lists=None):
        self.d1, self.nlists, self.nout = d1, len(olds), len(adds)
        olds = list(olds) + [0] * (self.nout - self.nlists)
        self.start0 = rng.integers(0, 1 << 31, size=self.nout, dtype=np.uint64).astype(np.uint32) if (d1 and start0) else None
        s0 = self.start0 if self.start0 is not None else np.zeros(self.nout, np.uint32)
        if lists is None:
            lists = [ref.d1_values(o + a, int(s0[j]), rng, outliers=True) if d1 else ref.plain_values(o + a, rng)
                     for j, (o, a) in enumerate(zip(olds, adds))]
        self.full = lists
        self.old = [v[:o] for v, o in zip(lists, olds)][:self.nlists]
        self.adds = [v[o:] for v, o in zip(lists, olds)]
        self.packed, self.offs, self.ptr, _ = ref.compose(self.old, d1, self.start0, ptr0=ptr0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.nunits = len(self.offs) - 1
        self.table = _table(self.old)
        self.add = np.concatenate([np.full(APTR0, 0xDEADBEEF, np.uint32)] + self.adds + [np.full(ATRAIL, 0xDEADBEEF, np.uint32)])
        self.aptr = APTR0 + np.concatenate([[0], np.cumsum([len(a) for a in self.adds])]).astype(np.uint64)
        # the expected index
        self.xpacked, self.xoffs, self.xptr, _ = ref.compose(self.full, d1, self.start0)
        self.xbase = np.asarray(ref.units_loop(self.xptr)[1], dtype=np.uint32)
        self.xunits = len(self.xoffs) - 1
        self.xtable = _table(self.full)

    def bounds(self):
        L = tpf.lib()
        return (int(L.tpf_lists_append_bound(len(self.packed), self.nout, len(self.add))),
                int(L.tpf_lists_append_units_bound(self.nunits, self.nout, len(self.add))))


class Guarded8:
    """n bytes, `shift` bytes past a 16-byte boundary, inside a sentinel-filled buffer"""

    def __init__(self, n, shift):
        self.n = n
        self.big = torch.full((n + 96,), SENT8, dtype=torch.uint8, device=DEV)
        self.s = 32 + (shift - self.big.data_ptr() - 32) % 16
        self.view = self.big[self.s: self.s + n]
        assert self.view.data_ptr() % 16 == shift % 16

    def read(self):
        got = self.big.cpu().numpy()
        return got[self.s: self.s + self.n], bool((got[:self.s] == SENT8).all() and (got[self.s + self.n:] == SENT8).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _run(c, shift_in=0, shift_out=0, offs=None, ptr=None, base=None, table=None, aptr=None, in_bytes=None, nunits=None, out_cap=None,
         units_cap=None, add_values=None, null_old=False):
    """One call of the C entry point on case `c`, every output guarded; the keyword arguments replace one input each."""
    L = tpf.lib()
    bb, ub = c.bounds()
    out_cap = bb if out_cap is None else out_cap
    units_cap = ub if units_cap is None else units_cap
    nunits = c.nunits if nunits is None else nunits
    in_bytes = len(c.packed) if in_bytes is None else in_bytes
    add_values = len(c.add) if add_values is None else add_values
    out = Guarded8(out_cap, shift_out)
    off_out = li.Guarded64(torch, units_cap + 1)
    lptr_out = li.Guarded64(torch, c.nout + 1)
    lunit_out = li.Guarded32(torch, c.nout + 1)
    ulast_out = li.Guarded32(torch, units_cap)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_in = None if null_old else li.dev8(torch, c.packed, shift_in)
    d_off = None if null_old else li.dev64(torch, c.offs if offs is None else offs)
    d_ptr = None if null_old else li.dev64(torch, c.ptr if ptr is None else ptr)
    d_base = None if null_old else li.dev32(torch, c.base if base is None else base)
    d_tab = li.dev32(torch, np.concatenate([c.table if table is None else table, [0]])) if c.d1 else None
    d_st = li.dev32(torch, c.start0) if c.start0 is not None else None
    d_add = li.dev32(torch, c.add)
    d_aptr = li.dev64(torch, c.aptr if aptr is None else aptr)
    ws = torch.empty(max(int(L.tpf_lists_append_workspace_size(nunits, c.nout, add_values)), 1), dtype=torch.uint8, device=DEV)
    rc = L.tpf_lists_append(_p(d_in), in_bytes, _p(d_off), nunits, _p(d_ptr), _p(d_base), c.nlists, int(c.d1), _p(d_st), _p(d_tab),
                            _p(d_add), add_values, _p(d_aptr), c.nout, _p(out.view), out_cap, _p(off_out.view), units_cap,
                            _p(lptr_out.view), _p(lunit_out.view), _p(ulast_out.view), _p(ws), ws.numel(), _p(err),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, tpf.lib().tpf_last_error()
    torch.cuda.synchronize()
    r = dict(err=int(err.item()))
    for name, g in (("out", out), ("off", off_out), ("lptr", lptr_out), ("lunit", lunit_out), ("ulast", ulast_out)):
        r[name], ok = g.read()
        assert ok, "written outside " + name
    return r


def _check(c, r, table=True):
    """bytes, offsets, both directories and the table equal the expected index; nothing else is written inside the capacities"""
    assert r["err"] == CLEAN
    assert np.array_equal(r["lptr"].view(np.uint64), c.xptr)
    assert np.array_equal(r["lunit"], c.xbase)
    n, u = len(c.xpacked), c.xunits
    assert np.array_equal(r["off"][:u + 1].view(np.uint64), c.xoffs)
    assert (r["off"][u + 1:] == SENT64).all()
    assert np.array_equal(r["out"][:n], c.xpacked)
    assert (r["out"][n:] == SENT8).all()
    if c.d1 and table:
        assert np.array_equal(r["ulast"][:u], c.xtable)
    assert (r["ulast"][u if c.d1 else 0:] == SENT).all()


def _untouched(r, names=("out", "off", "lptr", "lunit", "ulast")):
    for k in names:
        sent = {"out": SENT8, "off": SENT64, "lptr": SENT64}.get(k, SENT)
        assert (r[k] == sent).all(), k + " was written"


# ---- 1. the matrix --------------------------------------------------------------------
def _matrix_lens(rng):
    pairs = [(o, a) for o in OLD for a in ADD]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    # empty lists with empty additions in rows: at the start, in the middle, at the end
    pairs = [(0, 0)] * 3 + pairs[:20] + [(0, 0)] * 70 + pairs[20:] + [(0, 0)] * 2
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.fixture(scope="module")
def matrix():
    cases = {}
    for d1, st in ((True, True), (True, False), (False, False)):
        rng = np.random.default_rng(1234 + 2 * d1 + st)
        olds, adds = _matrix_lens(rng)
        cases[(d1, st)] = Case(olds, adds, d1, rng, start0=st)
    return cases


def test_matrix_holds_the_cases(matrix):
    c = matrix[(True, True)]
    got = {(len(o), len(a)) for o, a in zip(c.old, c.adds)}
    assert {(o, a) for o in OLD for a in ADD} <= got
    # the tail filling exactly, no old tail, a list with nothing at all
    assert {(255, 1), (1, 255), (257, 255), (256, 257), (0, 0)} <= got
    assert int(c.ptr[0]) == PTR0 and int(c.aptr[0]) == APTR0
    for cc in matrix.values():
        kinds = ref.block_kinds(cc.xpacked, cc.xoffs, cc.xptr)
        assert kinds["plain"] > 0 and kinds["bitmap"] > 0 and kinds["vbyte"] > 0, kinds


@pytest.mark.parametrize("shift_in,shift_out", [(0, 0), (1, 7), (7, 15), (15, 1)])
@pytest.mark.parametrize("d1,st", [(True, True), (True, False), (False, False)])
def test_matrix(matrix, d1, st, shift_in, shift_out):
    c = matrix[(d1, st)]
    _check(c, _run(c, shift_in=shift_in, shift_out=shift_out))


# ---- 2. new lists, and the empty old index -------------------------------------------------
@pytest.mark.parametrize("d1", [True, False])
def test_new_lists(d1):
    rng = np.random.default_rng(77 + d1)
    olds = [300, 0, 612, 256, 90]
    c = Case(olds, [10, 0, 0, 5, 0] + [0, 1, 256, 700, 0], d1, rng)
    assert c.nout == c.nlists + 5
    _check(c, _run(c))


@pytest.mark.parametrize("d1", [True, False])
def test_empty_old_index(d1):
    rng = np.random.default_rng(78 + d1)
    c = Case([], [0, 1, 256, 700, 0, 255, 513], d1, rng)
    assert c.nlists == 0 and c.nunits == 0
    r = _run(c, null_old=True)
    _check(c, r)
    # ... which is the encoder with the tables
    vals = li.dev32(torch, c.add)
    packed, offs = tpf.encn256v32_lists(vals, li.dev64(torch, c.aptr), d1=d1, start0=li.dev32(torch, c.start0) if d1 else None,
                                        nunits=c.xunits)
    assert np.array_equal(packed.cpu().numpy(), r["out"][:len(c.xpacked)])
    assert np.array_equal(offs.cpu().numpy(), r["off"][:c.xunits + 1])
    lp = li.dev64(torch, c.aptr)
    assert np.array_equal(tpf.lists_unit_base(lp).cpu().numpy().view(np.uint32), r["lunit"])
    if d1:
        ul = tpf.lists_unit_last(packed, offs, lp, start0=li.dev32(torch, c.start0))
        assert np.array_equal(ul.cpu().numpy().view(np.uint32), r["ulast"][:c.xunits])


# ---- 3. the stitch pass's tiles -------------------------------------------------------------
@pytest.mark.parametrize("d1", [True, False])
def test_stitch_tiling(d1):
    rng = np.random.default_rng(99 + d1)
    olds = [1] * 300 + [256 * 130 + 77] + [1] * 300
    adds = [(3 if j % 3 == 0 else 0) for j in range(len(olds))]
    s0 = np.zeros(len(olds), np.uint32)
    lists = [ref.d1_values(o + a, 0, rng) if d1 else ref.plain_values(o + a, rng) for o, a in zip(olds, adds)]
    c = Case(olds, adds, d1, rng, start0=False, lists=lists)
    assert (s0 == 0).all()
    j = 300
    kept = int(c.offs[c.base[j] + 130]) - int(c.offs[c.base[j]])
    assert kept > 3 * tpf.LISTS_APPEND_TILE  # the long list's copied bytes cross several tiles ...
    assert int(c.offs[c.base[300]]) < tpf.LISTS_APPEND_TILE // 8  # ... and 300 lists' segments lie inside one
    assert adds[300] == 3 and adds[301] == 0 and adds[303] == 3
    for shift in (0, 9):
        _check(c, _run(c, shift_in=shift, shift_out=(16 - shift) % 16))


# ---- 4. chaining -----------------------------------------------------------------------------
def test_chaining():
    rng = np.random.default_rng(5)
    olds = [300, 0, 612, 256, 90, 256 * 3 + 250]
    a_len = [10, 3, 0, 300, 166, 6]
    b_len = [500, 0, 7, 0, 256, 256]
    start0 = rng.integers(0, 1 << 20, size=len(olds), dtype=np.uint64).astype(np.uint32)
    lists = [ref.d1_values(o + a + b, int(s), rng) for o, a, b, s in zip(olds, a_len, b_len, start0)]
    old = [v[:o] for v, o in zip(lists, olds)]
    A = [v[o:o + a] for v, o, a in zip(lists, olds, a_len)]
    B = [v[o + a:] for v, o, a in zip(lists, olds, a_len)]
    packed, offs, ptr, _ = ref.compose(old, True, start0)
    xp, xo, xptr, xvals = ref.compose(lists, True, start0)
    st = li.dev32(torch, start0)
    cat = lambda xs: np.concatenate(xs).astype(np.uint32)
    csr = lambda xs: li.dev64(torch, np.concatenate([[0], np.cumsum([len(x) for x in xs])]))
    d_ptr = li.dev64(torch, ptr)
    d_unit = tpf.lists_unit_base(d_ptr)
    d_packed, d_offs = li.dev8(torch, packed), li.dev64(torch, offs)
    d_last = tpf.lists_unit_last(d_packed[:len(packed)], d_offs, d_ptr, start0=st)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    # A then B: the second call consumes the first's outputs as they lie on the device
    o1 = tpf.lists_append(d_packed[:len(packed)], d_offs, d_ptr, d_unit, li.dev32(torch, cat(A)), csr(A), d1=True, start0=st,
                          unit_last=d_last, err=err)
    assert int(err.item()) == CLEAN
    o2 = tpf.lists_append(o1[0], o1[1], o1[2], o1[3], li.dev32(torch, cat(B)), csr(B), d1=True, start0=st, unit_last=o1[4], err=err)
    assert int(err.item()) == CLEAN
    # A ++ B at once
    AB = [np.concatenate([a, b]) for a, b in zip(A, B)]
    o3 = tpf.lists_append(d_packed[:len(packed)], d_offs, d_ptr, d_unit, li.dev32(torch, cat(AB)), csr(AB), d1=True, start0=st,
                          unit_last=d_last, err=err)
    assert int(err.item()) == CLEAN
    nu = len(xo) - 1
    for o in (o2, o3):
        assert np.array_equal(o[0].cpu().numpy()[:len(xp)], xp)
        assert np.array_equal(o[1].cpu().numpy()[:nu + 1].view(np.uint64), xo)
        assert np.array_equal(o[2].cpu().numpy().view(np.uint64), xptr)
        assert np.array_equal(o[3].cpu().numpy().view(np.uint32), np.asarray(ref.units_loop(xptr)[1], dtype=np.uint32))
        assert np.array_equal(o[4].cpu().numpy()[:nu].view(np.uint32), _table(lists))
    # the readers take the result as it is: its offsets array is longer than the stream's units
    offs2 = o2[1][:nu + 1]
    dec = tpf.decn256v32_lists(o2[0], offs2, o2[2], d1=True, start0=st, out=torch.zeros(len(xvals), dtype=torch.int32, device=DEV), err=err)
    assert int(err.item()) == CLEAN
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), xvals)
    # ids of the old part, of A and of B, found at their positions through d_unit_last_out
    j = 5
    pos = np.array([0, 255, 256 * 3 + 249, olds[j], olds[j] + 5, olds[j] + a_len[j], len(lists[j]) - 1])
    probe = lists[j][pos]
    assert (np.diff(lists[j].astype(np.int64)) > 0).all()
    nq = 1
    out = torch.zeros(len(probe), dtype=torch.int32, device=DEV)
    tpos = torch.zeros(len(probe), dtype=torch.int32, device=DEV)
    pidx = torch.zeros(len(probe), dtype=torch.int32, device=DEV)
    res = tpf.lists_intersect(o2[0], offs2, o2[2], o2[3], o2[4][:nu], li.dev32(torch, probe), li.dev64(torch, [0, len(probe)]),
                              li.dev32(torch, [j]), start0=st, out=out, pidx=pidx, tpos=tpos, err=err)
    assert int(err.item()) == CLEAN and nq == 1
    assert int(res[1].cpu().numpy()[-1]) == len(probe)
    assert np.array_equal(tpos.cpu().numpy().view(np.uint32), pos.astype(np.uint32))


# ---- 5. what is parsed -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    out = {}
    for d1 in (True, False):
        rng = np.random.default_rng(31 + d1)
        #      untouched 17 units + tail | touched, 2 full + tail | tail-only touched | untouched tail-only | touched, no tail
        out[d1] = Case([256 * 17 + 3, 612, 90, 40, 512, 300], [0, 5, 300, 0, 9, 0], d1, rng)
    return out


@pytest.mark.parametrize("d1", [True, False])
def test_only_the_touched_tails_are_parsed(small, d1):
    c = small[d1]
    for u in (int(c.base[0]) + 9, int(c.base[1])):  # an interior unit of an untouched list, a full block of a touched one
        offs = c.offs.copy()
        offs[u + 1] += 1
        r = _run(c, offs=offs)
        assert r["err"] == CLEAN
        assert np.array_equal(r["out"][:len(c.xpacked)], c.xpacked)
        want = c.xoffs.copy()
        want[u + 1] += 1  # the units before list 1's tail keep their numbers
        assert np.array_equal(r["off"][:c.xunits + 1].view(np.uint64), want)
    # the end of the old tail of a touched list
    u = int(c.base[1]) + 2
    offs = c.offs.copy()
    offs[u + 1] += 1
    assert _run(c, offs=offs)["err"] == u
    # the same tail with an empty addition is copied, not parsed
    # (so is list 2's, which starts at the moved offset)
    c0 = Case([len(v) for v in c.old], [0, 0, 0, 0, 9, 0], d1, np.random.default_rng(0), lists=[
        v[:len(c.old[j])] if j in (1, 2) else v for j, v in enumerate(c.full)])
    c0 = _same_start(c0, c)
    r = _run(c0, offs=offs)
    assert r["err"] == CLEAN
    assert np.array_equal(r["lunit"], c0.xbase) and np.array_equal(r["lptr"].view(np.uint64), c0.xptr)
    want = c0.xoffs.copy()
    want[u + 1] += 1  # nothing but list 4's tail is encoded again, and the units keep their numbers up to it
    assert np.array_equal(r["off"][:u + 2].view(np.uint64), want[:u + 2])


def _same_start(c0, c):
    """c0 rebuilt with c's start0 (Case draws its own)"""
    c0.start0 = c.start0
    c0.packed, c0.offs, c0.ptr, _ = ref.compose(c0.old, c0.d1, c0.start0, ptr0=PTR0)
    c0.xpacked, c0.xoffs, c0.xptr, _ = ref.compose(c0.full, c0.d1, c0.start0)
    assert np.array_equal(c0.packed, c.packed) and np.array_equal(c0.offs, c.offs)
    return c0


# ---- 6. refusals -----------------------------------------------------------------------------
def test_structure_faults_are_refused_and_nothing_is_written(small):
    c = small[True]
    n = c.nunits

    def refused(j, nunits=n, **kw):
        r = _run(c, nunits=nunits, **kw)
        assert r["err"] == nunits + j, (r["err"], nunits + j, kw.keys())
        _untouched(r)

    ptr = c.ptr.copy()
    ptr[3] = ptr[2] - 1  # list 2 runs backwards (and list 3 is longer than its units)
    refused(2, ptr=ptr)
    ptr = c.ptr.copy()
    ptr[5], ptr[2] = ptr[4] - 1, ptr[1] - 1  # the lowest list wins
    refused(1, ptr=ptr)
    base = c.base.copy()
    base[3] += 1  # the span of list 2 is not its unit count
    refused(2, base=base)
    refused(5, nunits=n - 1, offs=c.offs[:-1])  # list_unit[6] > nunits
    offs = c.offs.copy()
    offs[c.base[3]] = offs[c.base[4]] + 1  # the copied range of list 3 runs backwards; list 2's parsed tail ends there, in bounds
    refused(3, offs=offs)
    refused(5, in_bytes=len(c.packed) - 1)  # the last copied range ends past the stream
    aptr = c.aptr.copy()
    aptr[3] = aptr[2] - 1
    refused(2, aptr=aptr)
    refused(2, add_values=int(c.aptr[3]) - 1)  # add_ptr[3] > add_values


@pytest.mark.parametrize("d1", [True, False])
def test_capacities(small, d1):
    c = small[d1]
    r = _run(c, units_cap=c.xunits - 1)
    assert r["err"] == c.nunits + c.nout
    _untouched(r, ("out", "off", "ulast"))
    assert np.array_equal(r["lptr"].view(np.uint64), c.xptr) and np.array_equal(r["lunit"], c.xbase)
    r = _run(c, units_cap=c.xunits, out_cap=len(c.xpacked))  # exactly enough
    _check(c, r)
    r = _run(c, out_cap=len(c.xpacked) - 1)
    assert r["err"] == c.nunits + c.nout + 1
    _untouched(r, ("out",))
    assert np.array_equal(r["lptr"].view(np.uint64), c.xptr) and np.array_equal(r["lunit"], c.xbase)
    assert np.array_equal(r["off"][:c.xunits + 1].view(np.uint64), c.xoffs)  # off[nunits_out]: what to allocate
    if d1:
        assert np.array_equal(r["ulast"][:c.xunits], c.xtable)


def test_no_lists_is_a_no_op():
    c = Case([], [], True, np.random.default_rng(1))
    r = _run(c, null_old=True)
    assert r["err"] == CLEAN
    assert r["lptr"].tolist() == [0] and r["lunit"].tolist() == [0] and r["off"][0] == 0
    _untouched(r, ("out", "ulast"))
    assert (r["off"][1:] == SENT64).all()


# ---- 7. a wrong table ------------------------------------------------------------------------
def test_wrong_table_is_harmless(matrix):
    c = matrix[(True, True)]
    r = _run(c, table=np.full(c.nunits, 0xFFFFFFFF, np.uint32))
    assert r["err"] == CLEAN
    assert np.array_equal(r["lptr"].view(np.uint64), c.xptr) and np.array_equal(r["lunit"], c.xbase)
    # lists with fewer than 256 old values start from start0: byte-exact, wherever the stream puts them
    seen = 0
    for j, o in enumerate(c.old):
        if len(o) < 256 and len(c.full[j]):
            u0, u1 = int(c.xbase[j]), int(c.xbase[j + 1])
            want = c.xpacked[int(c.xoffs[u0]): int(c.xoffs[u1])]
            g0, g1 = int(r["off"][u0]), int(r["off"][u1])
            assert g1 - g0 == len(want) and np.array_equal(r["out"][g0:g1], want), j
            seen += 1
    assert seen >= 15


# ---- 8. the rest of the index does not matter --------------------------------------------------
def test_index_independence():
    rng = np.random.default_rng(8)
    olds = [int(x) for x in rng.integers(0, 700, size=40)]
    adds = [int(x) for x in rng.integers(0, 300, size=40)]
    c = Case(olds, adds, True, rng)
    r = _run(c)
    _check(c, r)
    # the same 40 lists, every tenth list of an index ten times larger
    olds10, adds10, lists10 = [], [], []
    s0 = np.zeros(400, np.uint32)
    for j in range(40):
        for k in range(10):
            if k == 4:
                olds10.append(olds[j]), adds10.append(adds[j]), lists10.append(c.full[j])
                s0[len(olds10) - 1] = c.start0[j]
            else:
                o = int(rng.integers(0, 700))
                olds10.append(o), adds10.append(0 if k % 2 else int(rng.integers(0, 50)))
                lists10.append(ref.d1_values(o + adds10[-1], 0, rng))
    big = Case(olds10, adds10, True, rng, lists=lists10)
    big.start0 = s0
    big.packed, big.offs, big.ptr, _ = ref.compose(big.old, True, s0, ptr0=PTR0)
    big.table = _table(big.old)
    big.xpacked, big.xoffs, big.xptr, _ = ref.compose(big.full, True, s0)
    rb = _run(big)
    _check(big, rb)
    for j in range(40):
        jb = 10 * j + 4
        a = r["out"][int(r["off"][c.xbase[j]]): int(r["off"][c.xbase[j + 1]])]
        b = rb["out"][int(rb["off"][big.xbase[jb]]): int(rb["off"][big.xbase[jb + 1]])]
        assert np.array_equal(a, b), j
