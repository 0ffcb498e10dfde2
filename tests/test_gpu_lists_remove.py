"""GPU checks of the delete from a resident index (include/turbopfor_gpu.h
tpf_lists_remove): the result must be byte for byte, offset for offset and
table for table what the encoder writes for the shortened lists.  The old index
and the expected new one are both the oracle's composition (tests/lists_ref.py,
through tests/lists_remove_ref.py) -- of the old lists and of np.delete of them
-- and the skip tables are built from their definition (the last value of every
unit), never from the code under test.  Every output lies in a sentinel-filled
buffer and the C entry point is called directly, so that the tables are guarded
too."""
import ctypes

import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
import lists_remove_ref as rr
import lists_scale as sc
from lists_index import CLEAN, DEV, SENT, SENT64

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SENT8 = 0xA5


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


def _run(c, shift_in=0, shift_out=0, packed=None, offs=None, ptr=None, base=None, table=None, pos=None, pptr=None, qlist=None, nq=None,
         in_bytes=None, nunits=None, out_cap=None, units_cap=None, pos_values=None, stage=None, nlists=None):
    """One call of the C entry point on case `c`, every output guarded; the keyword arguments replace one input each."""
    L = tpf.lib()
    nq = c.nq if nq is None else nq
    stage = c.targeted if stage is None else stage
    nunits = c.nunits if nunits is None else nunits
    nlists = c.nlists if nlists is None else nlists
    in_bytes = len(c.packed) if in_bytes is None else in_bytes
    pos_values = len(c.pos) if pos_values is None else pos_values
    out_cap = int(L.tpf_lists_remove_bound(len(c.packed), nq, stage)) if out_cap is None else out_cap
    units_cap = c.nunits if units_cap is None else units_cap
    out = Guarded8(out_cap, shift_out)
    off_out = li.Guarded64(torch, units_cap + 1)
    lptr_out = li.Guarded64(torch, nlists + 1)
    lunit_out = li.Guarded32(torch, nlists + 1)
    ulast_out = li.Guarded32(torch, units_cap)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_in = li.dev8(torch, c.packed if packed is None else packed, shift_in)
    d_off = li.dev64(torch, c.offs if offs is None else offs)
    d_ptr = li.dev64(torch, c.ptr if ptr is None else ptr)
    d_base = li.dev32(torch, c.base if base is None else base)
    d_tab = li.dev32(torch, np.concatenate([c.table if table is None else table, [0]])) if c.d1 else None
    d_st = li.dev32(torch, c.start0) if c.start0 is not None else None
    d_pos = li.dev32(torch, c.pos if pos is None else pos)
    d_pptr = li.dev64(torch, c.pptr if pptr is None else pptr)
    d_ql = li.dev32(torch, np.concatenate([c.qlist if qlist is None else qlist, [0]]))
    ws = torch.empty(max(int(L.tpf_lists_remove_workspace_size(nunits, nlists, nq, pos_values, stage)), 1), dtype=torch.uint8, device=DEV)
    rc = L.tpf_lists_remove(_p(d_in), in_bytes, _p(d_off), nunits, _p(d_ptr), _p(d_base), nlists, int(c.d1), _p(d_st), _p(d_tab),
                            _p(d_pos), pos_values, _p(d_pptr), _p(d_ql), nq, stage, _p(out.view), out_cap, _p(off_out.view), units_cap,
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


def _dirs(c, r):
    assert np.array_equal(r["lptr"].view(np.uint64), c.xptr) and np.array_equal(r["lunit"], c.xbase)


def _untouched(r, names=("out", "off", "lptr", "lunit", "ulast")):
    for k in names:
        sent = {"out": SENT8, "off": SENT64, "lptr": SENT64}.get(k, SENT)
        assert (r[k] == sent).all(), k + " was written"


# ---- 1. the matrix --------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix():
    return {k: rr.matrix_case(*k) for k in ((True, True), (True, False), (False, False))}


def test_matrix_holds_the_cases(matrix):
    c = matrix[(True, True)]
    got = {(n, p) for n, p in c.plan if p is not None}
    assert got == {(n, p) for n in rr.LENS for p in rr.PATTERNS if rr.positions(p, n, np.random.default_rng(0)) is not None}
    u0s = set(c.u0.values())
    assert 0 in u0s and max(u0s) > 0                                                      # u0 == 0 and u0 > 0
    old, new = [len(v) for v in c.lists], [len(v) for v in c.new]
    assert any(o and not n for o, n in zip(old, new))                                     # a list emptied
    assert any(o % 256 == 0 and n % 256 for o, n in zip(old, new) if n)                   # a tail created
    assert any(o % 256 and n % 256 == 0 for o, n in zip(old, new) if n)                   # a tail removed
    touched = [j in c.u0 for j in range(c.nlists)]
    assert any(touched[j - 1] and not touched[j] and old[j] and touched[j + 1] for j in range(1, c.nlists - 1))
    assert int(c.ptr[0]) == rr.PTR0 != 0 and int(c.pptr[0]) == rr.POS0 != 0 and len(c.pos) > int(c.pptr[-1])


@pytest.mark.parametrize("shift_in,shift_out", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("d1,st", [(True, True), (True, False), (False, False)])
def test_matrix(matrix, d1, st, shift_in, shift_out):
    c = matrix[(d1, st)]
    _check(c, _run(c, shift_in=shift_in, shift_out=shift_out))


@pytest.mark.parametrize("d1", [True, False])
def test_exact_staging_and_capacities(matrix, d1):
    c = matrix[(d1, False)]
    _check(c, _run(c, stage=c.staged, out_cap=len(c.xpacked), units_cap=c.xunits))


# ---- 2. what is parsed -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    out = {}
    for d1 in (True, False):
        rng = np.random.default_rng(31 + d1)
        lens = [256 * 17 + 3, 612, 90, 40, 512 + 256, 300]
        s0 = rng.integers(0, 1 << 31, size=len(lens), dtype=np.uint64).astype(np.uint32)
        lists = [rr.values(n, d1, s0[j], rng) for j, n in enumerate(lens)]
        # list 0 untargeted | list 1: u0 = 1 | list 2: tail-only | list 3 targeted, nothing removed | list 4: u0 = 1 | list 5
        # untargeted
        rem = {1: np.array([300, 301, 611]), 2: np.array([0, 89]), 3: np.zeros(0, np.int64), 4: np.array([511, 600])}
        out[d1] = rr.Case(lists, rem, d1, s0)
    return out


def _flip(c, u):
    """the stream with the header byte of unit u changed: its parse no longer ends where its offsets say"""
    p = c.packed.copy()
    p[int(c.offs[u])] ^= 1
    return p, int(c.offs[u])


@pytest.mark.parametrize("d1", [True, False])
def test_kept_ranges_are_never_parsed(small, d1):
    c = small[d1]
    assert c.u0 == {1: 1, 2: 0, 4: 1}
    # a unit before u0 of a touched list, a unit and the tail of an untargeted list, the tail of a targeted list that loses nothing
    for u in (int(c.base[1]), int(c.base[4]), int(c.base[0]) + 9, int(c.base[1]) - 1, int(c.base[3]), int(c.base[5]) + 1):
        p, at = _flip(c, u)
        r = _run(c, packed=p)
        assert r["err"] == CLEAN, u
        # the byte is carried over to where the unit went; every other byte is the expected one
        j = int(np.searchsorted(c.base, u, side="right") - 1)
        xat = int(c.xoffs[int(c.xbase[j]) + (u - int(c.base[j]))])
        want = c.xpacked.copy()
        assert want[xat] == c.packed[at]
        want[xat] ^= 1
        assert np.array_equal(r["out"][:len(want)], want), u
        assert np.array_equal(r["off"][:c.xunits + 1].view(np.uint64), c.xoffs)
    # the same inside a unit at or after u0: the unit is reported
    for u in (int(c.base[1]) + 1, int(c.base[1]) + 2, int(c.base[2]), int(c.base[4]) + 1, int(c.base[4]) + 2):
        p, _ = _flip(c, u)
        assert _run(c, packed=p)["err"] == u, u
    # offsets outside the stream, of a decoded unit: the lowest one is reported
    offs = c.offs.copy()
    u = int(c.base[4]) + 1
    offs[u + 1: int(c.base[5])] = len(c.packed) + 100
    assert _run(c, offs=offs)["err"] == u


# ---- 3. chaining -----------------------------------------------------------------------------
def test_chaining():
    rng = np.random.default_rng(5)
    ix = li.Index([300, 0, 612, 256, 90, 256 * 3 + 250, 7], rng, start_bits=20)
    assert ix.ascends()
    tw = sc.Twin(ix, rng)
    d_ptr = li.dev64(torch, ix.ptr)
    d_unit = tpf.lists_unit_base(d_ptr)
    st = li.dev32(torch, ix.start0)
    d_packed, d_offs = li.dev8(torch, ix.packed)[:len(ix.packed)], li.dev64(torch, ix.offs)
    f_packed, f_offs = li.dev8(torch, tw.fpacked)[:len(tw.fpacked)], li.dev64(torch, tw.foffs)
    d_last = tpf.lists_unit_last(d_packed, d_offs, d_ptr, start0=st)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    # the (term, doc id) pairs of deleted documents: queries ascending by list, sorted probes, some ids in no list
    qlist = np.array([0, 2, 3, 5, 6])
    segs, rem = [], {}
    for j in qlist:
        v = ix.lists[j]
        at = np.unique(rng.integers(0, len(v), size=max(1, len(v) // 7)))
        rem[int(j)] = at
        segs.append(np.unique(np.concatenate([v[at], v[at[:3]] + np.uint32(1) if j != 6 else v[:0]])))
    rem[6] = np.arange(7)  # the whole list
    segs[-1] = ix.lists[6].copy()
    for j, s in zip(qlist, segs):
        rem[int(j)] = np.nonzero(np.isin(ix.lists[j], s))[0]
    probe = np.concatenate(segs)
    pp = sc._starts([len(s) for s in segs])
    d_probe, d_pp, d_ql = li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist)
    tpos = torch.zeros(len(probe), dtype=torch.int32, device=DEV)
    hits, hptr = tpf.lists_intersect(d_packed, d_offs, d_ptr, d_unit, d_last, d_probe, d_pp, d_ql, start0=st, tpos=tpos, err=err)
    assert int(err.item()) == CLEAN
    nh = int(hptr.cpu().numpy()[-1])
    assert nh == sum(len(x) for x in rem.values()) < len(probe)
    want = rr.Case(ix.lists, rem, True, ix.start0, ptr0=0)
    fwant = rr.Case(tw.freqs, rem, False, ptr0=0)
    stage = want.targeted
    # the intersection's outputs feed the call unchanged, on the doc-id stream and on the frequency twin
    o = tpf.lists_remove(d_packed, d_offs, d_ptr, d_unit, tpos, hptr, d_ql, stage, d1=True, start0=st, unit_last=d_last, err=err)
    assert int(err.item()) == CLEAN
    f = tpf.lists_remove(f_packed, f_offs, d_ptr, d_unit, tpos, hptr, d_ql, stage, d1=False, err=err)
    assert int(err.item()) == CLEAN
    for got, w in ((o, want), (f, fwant)):
        nu = w.xunits
        assert np.array_equal(got[0].cpu().numpy()[:len(w.xpacked)], w.xpacked)
        assert np.array_equal(got[1].cpu().numpy()[:nu + 1].view(np.uint64), w.xoffs)
        assert np.array_equal(got[2].cpu().numpy().view(np.uint64), w.xptr)
        assert np.array_equal(got[3].cpu().numpy().view(np.uint32), w.xbase)
    nu = want.xunits
    assert np.array_equal(o[4].cpu().numpy()[:nu].view(np.uint32), want.xtable)
    assert np.array_equal(f[2].cpu().numpy(), o[2].cpu().numpy()) and np.array_equal(f[3].cpu().numpy(), o[3].cpu().numpy())
    # the new index holds none of the removed ids ...
    offs2, last2 = o[1][:nu + 1], o[4][:nu]
    _, hptr2 = tpf.lists_intersect(o[0], offs2, o[2], o[3], last2, d_probe, d_pp, d_ql, start0=st, err=err)
    assert int(err.item()) == CLEAN and int(hptr2.cpu().numpy()[-1]) == 0
    # ... and the surviving (doc id, frequency) pairs at every position of the targeted lists
    gpos = np.concatenate([np.arange(len(want.new[j])) for j in qlist]).astype(np.uint32)
    gptr = sc._starts([len(want.new[j]) for j in qlist])
    d_gpos, d_gptr = li.dev32(torch, gpos), li.dev64(torch, gptr)
    ids = tpf.lists_gather(o[0], offs2, o[2], o[3], d_gpos, d_gptr, d_ql, d1=True, start0=st, unit_last=last2, err=err)
    assert int(err.item()) == CLEAN
    fr = tpf.lists_gather(f[0], f[1][:nu + 1], f[2], f[3], d_gpos, d_gptr, d_ql, d1=False, err=err)
    assert int(err.item()) == CLEAN
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), np.concatenate([want.new[j] for j in qlist]))
    assert np.array_equal(fr.cpu().numpy().view(np.uint32), np.concatenate([fwant.new[j] for j in qlist]))
    # an append to the new index equals the oracle's composition
    adds = [(v[-1] if len(v) else np.uint32(s)) + np.arange(1, 1 + n, dtype=np.uint32) * np.uint32(3)
            for v, s, n in zip(want.new, ix.start0, [5, 2, 0, 300, 1, 7, 4])]
    full = [np.concatenate([v, a]).astype(np.uint32) for v, a in zip(want.new, adds)]
    xp, xo, xptr, _ = ref.compose(full, True, ix.start0)
    a = tpf.lists_append(o[0], o[1], o[2], o[3], li.dev32(torch, np.concatenate(adds)), li.dev64(torch, sc._starts([len(x) for x in adds])),
                         d1=True, start0=st, unit_last=o[4], err=err)
    assert int(err.item()) == CLEAN
    assert np.array_equal(a[0].cpu().numpy()[:len(xp)], xp) and np.array_equal(a[1].cpu().numpy()[:len(xo)].view(np.uint64), xo)
    assert np.array_equal(a[2].cpu().numpy().view(np.uint64), xptr)
    assert np.array_equal(a[4].cpu().numpy()[:len(xo) - 1].view(np.uint32), rr.table(full))


# ---- 4. refusals -----------------------------------------------------------------------------
def test_structure_faults_are_refused_and_nothing_is_written(small):
    c = small[True]
    n = c.nunits

    def refused(j, nunits=n, **kw):
        r = _run(c, nunits=nunits, **kw)
        assert r["err"] == nunits + j, (r["err"], nunits + j, kw.keys())
        _untouched(r)

    ptr = c.ptr.copy()
    ptr[1] = ptr[0] - 1  # list 0 runs backwards: the lowest index
    refused(0, ptr=ptr)
    ptr = c.ptr.copy()
    ptr[6] = ptr[5] - 1  # the highest
    refused(5, ptr=ptr)
    ptr = c.ptr.copy()
    ptr[5], ptr[2] = ptr[4] - 1, ptr[1] - 1  # the lowest list wins
    refused(1, ptr=ptr)
    base = c.base.copy()
    base[3] += 1  # the span of list 2 is not its unit count
    refused(2, base=base)
    refused(5, nunits=n - 1, offs=c.offs[:-1])  # list_unit[6] > nunits
    offs = c.offs.copy()
    offs[c.base[0]] = offs[c.base[1]] + 1  # the copied range of list 0 runs backwards
    refused(0, offs=offs)
    refused(5, in_bytes=len(c.packed) - 1)  # the last copied range ends past the stream


@pytest.mark.parametrize("k", [0, 3])
def test_refused_queries(small, k):
    """every refusal of a query, at the lowest and the highest index"""
    c = small[True]
    assert c.nq == 4 and c.qlist.tolist() == [1, 2, 3, 4]
    code = c.nunits + c.nlists + k

    def refused(kk=k, **kw):
        r = _run(c, **kw)
        assert r["err"] == c.nunits + c.nlists + kk, (r["err"], kw.keys())
        _untouched(r)

    ql = c.qlist.copy()
    ql[k] = c.nlists  # no such list
    refused(qlist=ql)
    ql = c.qlist.copy()
    if k == 0:
        ql[1] = ql[0]  # a list named twice: the second query is the refused one, query 1 the lowest that can be
        refused(kk=1, qlist=ql)
        ql[0], ql[1] = 2, 1  # descending, each segment inside its list
        refused(kk=1, qlist=ql, pos=_pos_for(c, {0: [1, 2, 3]}))
    else:
        ql[k] = ql[k - 1]
        refused(qlist=ql)
    pptr = c.pptr.copy()
    pptr[k + 1] = pptr[k] - 1  # a segment that runs backwards (the next one is then too long for its list, or ascends no more)
    r = _run(c, pptr=pptr)
    assert r["err"] == code
    _untouched(r)
    if k == 3:
        refused(pos_values=int(c.pptr[4]) - 1)  # pos_ptr[nq] > pos_values
    else:
        pptr = c.pptr.copy()
        pptr[1:] += len(c.pos)  # pos_ptr[1] > pos_values
        refused(pptr=pptr)
    j = int(c.qlist[k])
    seg = slice(int(c.pptr[k]), int(c.pptr[k + 1]))
    pos = c.pos.copy()
    pos[seg.stop - 1] = len(c.lists[j])  # a position that is not in the list
    refused(pos=pos)
    pos = c.pos.copy()
    pos[seg.start] = 0xFFFFFFFF  # ... as the first of its segment
    refused(pos=pos)
    pos = c.pos.copy()
    pos[seg.stop - 1] = pos[seg.stop - 2]  # a position twice
    refused(pos=pos)
    pos = c.pos.copy()
    pos[seg.start], pos[seg.start + 1] = pos[seg.start + 1], pos[seg.start]  # descending
    refused(pos=pos)


def _pos_for(c, first):
    """c.pos with the segments of the queries in `first` beginning with the given positions"""
    pos = c.pos.copy()
    for k, vals in first.items():
        pos[int(c.pptr[k]): int(c.pptr[k]) + len(vals)] = vals
    return pos


@pytest.mark.parametrize("d1", [True, False])
def test_capacities(small, d1):
    c = small[d1]
    base = c.nunits + c.nlists + c.nq
    r = _run(c, stage=c.staged - 1)
    assert r["err"] == base
    _untouched(r, ("out", "off", "ulast"))
    _dirs(c, r)
    _check(c, _run(c, stage=c.staged))  # exactly enough
    r = _run(c, units_cap=c.xunits - 1)
    assert r["err"] == base + 1
    _untouched(r, ("out", "off", "ulast"))
    _dirs(c, r)
    _check(c, _run(c, units_cap=c.xunits, out_cap=len(c.xpacked)))  # exactly enough
    r = _run(c, out_cap=len(c.xpacked) - 1)
    assert r["err"] == base + 2
    _untouched(r, ("out",))
    _dirs(c, r)
    assert np.array_equal(r["off"][:c.xunits + 1].view(np.uint64), c.xoffs)  # off[nunits_out]: what to allocate
    if d1:
        assert np.array_equal(r["ulast"][:c.xunits], c.xtable)


def test_no_lists_is_a_no_op(small):
    c = small[True]
    r = _run(c, nlists=0, nq=0)
    assert r["err"] == CLEAN
    assert r["lptr"].tolist() == [0] and r["lunit"].tolist() == [0] and r["off"][0] == 0
    _untouched(r, ("out", "ulast"))
    assert (r["off"][1:] == SENT64).all()
    r = _run(c, nlists=0)  # queries on no lists: the same no-op
    assert r["err"] == CLEAN and r["lptr"].tolist() == [0]


@pytest.mark.parametrize("d1", [True, False])
def test_no_queries_reproduce_the_index(small, d1):
    c = small[d1]
    same = rr.Case(c.lists, {}, d1, c.start0)
    assert np.array_equal(same.xpacked, c.packed) and np.array_equal(same.xoffs, c.offs)
    _check(same, _run(same, stage=0))
    _check(same, _run(same, stage=0, shift_in=1, out_cap=len(c.packed), units_cap=c.nunits))
    # ... and so do queries whose segments are all empty
    empty = rr.Case(c.lists, {j: np.zeros(0, np.int64) for j in (0, 2, 5)}, d1, c.start0)
    _check(empty, _run(empty, stage=0))


# ---- 5. a wrong table ------------------------------------------------------------------------
def test_wrong_table_is_harmless(matrix):
    c = matrix[(True, True)]
    r = _run(c, table=np.full(c.nunits, 0xFFFFFFFF, np.uint32))
    assert r["err"] == CLEAN
    _dirs(c, r)
    # a list that is copied, or whose one decoded unit starts from start0, never meets the table: byte-exact
    seen = 0
    for j in range(c.nlists):
        if (j not in c.u0 or len(c.lists[j]) <= 256) and len(c.new[j]):
            u0, u1 = int(c.xbase[j]), int(c.xbase[j + 1])
            want = c.xpacked[int(c.xoffs[u0]): int(c.xoffs[u1])]
            g0, g1 = int(r["off"][u0]), int(r["off"][u1])
            assert g1 - g0 == len(want) and np.array_equal(r["out"][g0:g1], want), j
            seen += 1
    assert seen >= 40
    assert not np.array_equal(r["out"][:len(c.xpacked)], c.xpacked)  # every other decoded unit starts from the table: wrong bytes


# ---- 6. the rest of the index does not matter --------------------------------------------------
def test_index_independence():
    rng = np.random.default_rng(8)
    lens = [int(x) for x in rng.integers(0, 900, size=30)]
    s0 = rng.integers(0, 1 << 31, size=30, dtype=np.uint64).astype(np.uint32)
    lists = [rr.values(n, True, s0[j], rng) for j, n in enumerate(lens)]
    rem = {j: np.unique(rng.integers(0, lens[j], size=1 + lens[j] // 9)) for j in range(30) if lens[j] and j % 4 != 3}
    c = rr.Case(lists, rem, True, s0)
    r = _run(c)
    _check(c, r)
    # the same 30 lists, every tenth list of an index ten times larger
    lists10, rem10, s10 = [], {}, np.zeros(300, np.uint32)
    for j in range(30):
        for k in range(10):
            jb = len(lists10)
            if k == 4:
                lists10.append(lists[j])
                s10[jb] = s0[j]
                if j in rem:
                    rem10[jb] = rem[j]
            else:
                n = int(rng.integers(0, 700))
                lists10.append(ref.d1_values(n, 0, rng))
                if k % 3 == 0 and n:
                    rem10[jb] = np.unique(rng.integers(0, n, size=3))
    big = rr.Case(lists10, rem10, True, s10)
    rb = _run(big)
    _check(big, rb)
    for j in range(30):
        jb = 10 * j + 4
        a = r["out"][int(r["off"][c.xbase[j]]): int(r["off"][c.xbase[j + 1]])]
        b = rb["out"][int(rb["off"][big.xbase[jb]]): int(rb["off"][big.xbase[jb + 1]])]
        assert np.array_equal(a, b), j
