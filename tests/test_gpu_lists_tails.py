"""Every lists entry point on the tail families (tests/lists_tails.py): indexes
whose tail units -- the horizontal p4Enc32 / p4D1Enc32 block of a list's last
n % 256 values -- hold every mode at every count 1..255, behind start0 and
behind a full block, with lists that wrap 2^32 in the "wide" family.  The
expected values are the original lists, the numpy restatements of the
definitions and the oracle's bytes (tests/test_lists_tails_cpu.py holds those to
the reference), never the code under test.  Every output lies in a
sentinel-filled buffer; the append and the remove are called through the C
entry points, so that their directories and tables are guarded too."""
import ctypes
import functools

import numpy as np
import pytest

import lists_difference_ref as dr
import lists_index as li
import lists_ref as ref
import lists_remove_ref as rr
import lists_scale as sc
import lists_tails as lt
import lists_union_ref as ur
from lists_index import CLEAN, DEV, SENT, SENT64

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SENT8 = 0xA5
FORMS = [("wide", False), ("wide", True), ("ascending", True)]


class Guarded8:
    """n bytes, `shift` bytes past a 16-byte boundary, inside a sentinel-filled buffer"""

    def __init__(self, n, shift=0):
        self.n = n
        self.big = torch.full((n + 96,), SENT8, dtype=torch.uint8, device=DEV)
        self.s = 32 + (shift - self.big.data_ptr() - 32) % 16
        self.view = self.big[self.s: self.s + n]
        assert self.view.data_ptr() % 16 == shift % 16

    def read(self):
        got = self.big.cpu().numpy()
        return got[self.s: self.s + self.n], bool((got[:self.s] == SENT8).all() and (got[self.s + self.n:] == SENT8).all())


def _read(g, what):
    got, ok = g.read()
    assert ok, "written outside " + what
    return got.view(np.uint32) if got.dtype == np.int32 else got


class Resident:
    """A stream of a family on the device with the directory and the skip table of its DEFINITION (lists_index.Index)."""

    def __init__(self, s, d1, ix):
        self.s, self.d1, self.ix = s, d1, ix
        self.packed = li.dev8(torch, s.packed)[:len(s.packed)]
        self.offs = li.dev64(torch, s.offs)
        self.ptr = li.dev64(torch, s.ptr)
        self.unit = li.dev32(torch, s.base)
        self.start0 = li.dev32(torch, ix.start0) if d1 else None
        self.last = li.dev32(torch, ix.table) if d1 else None
        self.err = torch.zeros(1, dtype=torch.int64, device=DEV)

    def clean(self):
        torch.cuda.synchronize()
        assert int(self.err.item()) == CLEAN, int(self.err.item())
        self.err.zero_()


@functools.lru_cache(maxsize=None)
def _twin():
    """the plain stream stored in parallel to the ascending index (lists_scale.Twin)"""
    tw = sc.Twin(lt.family("ascending").index(), np.random.default_rng(77))
    ix = tw.ix
    return type("TwinStream", (), dict(packed=tw.fpacked, offs=tw.foffs, ptr=ix.ptr, vals=tw.fvals, base=ix.base, lists=tw.freqs,
                                       nlists=ix.nlists, nunits=ix.nunits))


@functools.lru_cache(maxsize=None)
def _res(name, d1):
    if name == "twin":
        return Resident(_twin(), False, lt.family("ascending").index())
    fam = lt.family(name)
    return Resident(fam.form(d1), d1, fam.index())


# ---- decode side ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d1", FORMS)
def test_full_decode(name, d1):
    r = _res(name, d1)
    out = li.Guarded32(torch, len(r.s.vals))
    tpf.decn256v32_lists(r.packed, r.offs, r.ptr, d1=d1, start0=r.start0, out=out.view, err=r.err)
    r.clean()
    assert np.array_equal(_read(out, "out"), r.s.vals)


@pytest.mark.parametrize("name", lt.FAMILIES)
def test_directory_and_skip_table(name):
    """tpf_lists_unit_base equals units_loop; tpf_lists_unit_last equals the last value of every unit -- k_ul_tails' sum at every
    count and mode, over lists that wrap for "wide"."""
    r = _res(name, True)
    ix = r.ix
    unit = li.Guarded32(torch, ix.nlists + 1)
    tpf.lists_unit_base(r.ptr, out=unit.view, err=r.err)
    r.clean()
    assert _read(unit, "list_unit").tolist() == ref.units_loop(ix.ptr)[1]
    last = li.Guarded32(torch, ix.nunits)
    tpf.lists_unit_last(r.packed, r.offs, r.ptr, start0=r.start0, out=last.view, err=r.err)
    r.clean()
    got = _read(last, "unit_last")
    bad = np.nonzero(got != ix.table)[0]
    assert len(bad) == 0, (name, len(bad), _where(lt.family(name), ix, bad[:5]))


def _where(fam, ix, units):
    """(list, count, mode, block in front) of the lists that hold `units`, for a failure's message"""
    js = np.searchsorted(ix.base, units, side="right") - 1
    return [(int(j), int(fam.cnt[j]), fam.mode[j], bool(fam.front[j])) for j in js]


@pytest.mark.parametrize("d1", [False, True])
def test_select(d1):
    """all lists in a seeded permutation, some twice"""
    fam, r = lt.family("wide"), _res("wide", d1)
    perm = np.random.default_rng(11).permutation(fam.nlists)
    sel = np.concatenate([perm, perm[:300], perm[-50:]])
    want, wptr = sc.want_select(r.s, sel)
    out, optr = li.Guarded32(torch, len(want)), li.Guarded64(torch, len(sel) + 1)
    tpf.decn256v32_lists_select(r.packed, r.offs, r.ptr, r.unit, li.dev32(torch, sel), d1=d1, start0=r.start0, out=out.view,
                                out_ptr=optr.view, err=r.err)
    r.clean()
    assert np.array_equal(_read(optr, "out_ptr"), wptr)
    assert np.array_equal(_read(out, "out"), want)


@pytest.mark.parametrize("d1", [False, True])
def test_unit_ranges(d1):
    """every list's whole unit range and, behind a full block, the tail unit alone -- from the directory and the table the
    device built"""
    fam, r = lt.family("wide"), _res("wide", d1)
    unit = tpf.lists_unit_base(r.ptr, err=r.err)
    r.clean()
    last = None
    if d1:
        last = tpf.lists_unit_last(r.packed, r.offs, r.ptr, start0=r.start0, err=r.err)
        r.clean()
    units = np.diff(r.s.base.astype(np.int64))
    front = np.nonzero(fam.front)[0]
    sel = np.concatenate([np.arange(fam.nlists), front])
    ufirst = np.concatenate([np.zeros(fam.nlists, np.int64), np.ones(len(front), np.int64)])
    ucount = np.concatenate([units, np.ones(len(front), np.int64)])
    order = np.random.default_rng(12).permutation(len(sel))
    sel, ufirst, ucount = sel[order], ufirst[order], ucount[order]
    want, wptr = sc.want_units(r.s, sel, ufirst, ucount)
    assert len(want) == len(r.s.vals) + int(fam.cnt[front].sum())
    out, optr = li.Guarded32(torch, len(want)), li.Guarded64(torch, len(sel) + 1)
    tpf.decn256v32_lists_units(r.packed, r.offs, r.ptr, unit, li.dev32(torch, sel), li.dev32(torch, ufirst), li.dev32(torch, ucount),
                               d1=d1, start0=r.start0, unit_last=last, out=out.view, out_ptr=optr.view, err=r.err)
    r.clean()
    assert np.array_equal(_read(optr, "out_ptr"), wptr)
    assert np.array_equal(_read(out, "out"), want)


@pytest.mark.parametrize("name,d1", FORMS + [("twin", False)])
def test_gather(name, d1):
    """per list every position of the tail in ascending order; then reversed, with the tail's last and first position and
    the list's first repeated"""
    fam = lt.family("ascending" if name == "twin" else name)
    r = _res(name, d1)
    qlist = np.nonzero(fam.cnt)[0]
    for rev in (False, True):
        segs = []
        for j in qlist:
            n, cnt = int(fam.lens[j]), int(fam.cnt[j])
            p = np.arange(n - cnt, n)
            segs.append(np.concatenate([p[::-1], [n - 1, n - 1, n - cnt, n - cnt, 0, n - 1]]) if rev else p)
        pos, pptr = np.concatenate(segs), sc._starts([len(x) for x in segs])
        want = sc.want_gather(r.s.ptr, r.s.vals, qlist, pptr, pos)
        out = li.Guarded32(torch, len(pos))
        tpf.lists_gather(r.packed, r.offs, r.ptr, r.unit, li.dev32(torch, pos), li.dev64(torch, pptr), li.dev32(torch, qlist), d1=d1,
                         start0=r.start0, unit_last=r.last, out=out.view, err=r.err)
        r.clean()
        got = _read(out, "out")
        bad = np.nonzero(got != want)[0]
        ql = np.repeat(qlist, np.diff(pptr))
        assert len(bad) == 0, (name, d1, rev, len(bad), [(int(ql[i]), int(fam.cnt[ql[i]]), fam.mode[ql[i]], int(pos[i])) for i in bad[:5]])


# ---- the set operations on "ascending" ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probe():
    """One query per non-empty list: the sorted unique {v - 1, v, v + 1} over the tail's values, the value the tail starts
    from, start0, the last value + 1 and 0xFFFFFFFF (the pad word of item_tail_units), clipped to [0, 2^32).
    -> (qlist, probe, probe_ptr)"""
    fam = lt.family("ascending")
    ix = fam.index()
    qlist = np.nonzero(fam.cnt)[0]
    segs = []
    for j in qlist:
        t = ix.lists[j][-int(fam.cnt[j]):].astype(np.int64)
        marks = np.concatenate([t - 1, t, t + 1, [fam.tail_start(j), int(ix.start0[j]), int(t[-1]) + 1, 0xFFFFFFFF]])
        segs.append(np.unique(np.clip(marks, 0, 0xFFFFFFFF)).astype(np.uint32))
    return qlist, np.concatenate(segs), sc._starts([len(x) for x in segs])


_SETOPS = {"intersect": (lambda: tpf.lists_intersect, lambda ix, q, pp, p: sc.want_hits(ix, q, pp, p)),
           "union": (lambda: tpf.lists_union, lambda ix, q, pp, p: ur.want_union_keys(ix, q, pp, p)),
           "difference": (lambda: tpf.lists_difference, lambda ix, q, pp, p: dr.want_difference_keys(ix, q, pp, p))}


@functools.lru_cache(maxsize=None)
def _setop(kind):
    """One call of the entry point on _probe(), every output guarded.  -> ((values, out_ptr, pidx, tpos) the device wrote, the
    same by the numpy restatement)"""
    r = _res("ascending", True)
    qlist, probe, pp = _probe()
    want = _SETOPS[kind][1](r.ix, qlist, pp, probe)
    cap = len(probe) + (int(r.ix.ptr[-1]) if kind == "union" else 0)
    out, pidx, tpos = (li.Guarded32(torch, cap) for _ in range(3))
    optr = li.Guarded64(torch, len(qlist) + 1)
    _SETOPS[kind][0]()(r.packed, r.offs, r.ptr, r.unit, r.last, li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist),
                       start0=r.start0, out=out.view, out_ptr=optr.view, pidx=pidx.view, tpos=tpos.view, err=r.err)
    r.clean()
    gptr = _read(optr, "out_ptr")
    n = int(gptr[-1])
    return (_read(out, "out")[:n], gptr, _read(pidx, "pidx")[:n], _read(tpos, "tpos")[:n]), want


def _probe_census():
    """what the probe holds: every tail value (a hit at its exact position), misses below, inside and above every tail, and
    the pad word"""
    fam = lt.family("ascending")
    qlist, probe, pp = _probe()
    (_, wptr, _, _) = _setop("intersect")[1]
    assert int(wptr[-1]) >= int(fam.cnt.sum())                      # every tail value is in its probe
    assert len(probe) - int(wptr[-1]) >= 2 * len(qlist)             # at least the last value + 1 and the pad word miss
    assert (probe[pp[1:] - 1] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("kind", ["intersect", "union", "difference"])
def test_set_operation(kind):
    _probe_census()
    got, want = _setop(kind)
    fam = lt.family("ascending")
    qlist = _probe()[0]
    assert np.array_equal(got[1], want[1]), (kind, "out_ptr")
    for g, w, what in zip((got[0], got[2], got[3]), (want[0], want[2], want[3]), ("values", "pidx", "tpos")):
        bad = np.nonzero(g != w)[0]
        qs = qlist[np.searchsorted(want[1], bad[:5], side="right") - 1]
        assert len(bad) == 0, (kind, what, len(bad), [(int(j), int(fam.cnt[j]), fam.mode[j], bool(fam.front[j])) for j in qs])


def test_intersection_and_difference_partition_the_probe():
    """the complement law on the device's own outputs of the same call arguments"""
    qlist, probe, pp = _probe()
    (hv, hptr, hidx, _), (dv, dptr, didx, _) = _setop("intersect")[0], _setop("difference")[0]
    assert np.array_equal(np.diff(hptr) + np.diff(dptr), np.diff(pp))
    assert np.array_equal(np.sort(np.concatenate([hidx, didx])), np.arange(len(probe)))
    assert np.array_equal(probe[hidx], hv) and np.array_equal(probe[didx], dv)
    # both are in probe order
    assert (np.diff(hidx.astype(np.int64)) > 0).all() and (np.diff(didx.astype(np.int64)) > 0).all()


# ---- encode side --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoded(name, d1, shift):
    """tpf_p4nenc256v32_lists of the family's values.  -> (bytes, offsets) as written"""
    r = _res(name, d1)
    s = r.s
    out = Guarded8(tpf.lists_enc_bound(len(s.vals), s.nlists), shift)
    offs = li.Guarded64(torch, s.nunits + 1)
    tpf.encn256v32_lists(li.dev32(torch, s.vals), r.ptr, d1=d1, start0=r.start0, nunits=s.nunits, out=out.view, offsets=offs.view,
                         err=r.err)
    r.clean()
    return _read(out, "out"), _read(offs, "offsets").view(np.uint64)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name,d1", FORMS)
def test_encode(name, d1, shift):
    """the device's p4Bits32 choice and horizontal pack, byte for byte at every (count, mode)"""
    s = lt.family(name).form(d1)
    got, offs = _encoded(name, d1, shift)
    _same_stream(lt.family(name), s, got, offs)


def _same_stream(fam, s, got, offs, what="encode"):
    """offsets and bytes equal the oracle's composition `s`; a failure names the first lists that differ"""
    if not np.array_equal(offs[:s.nunits + 1], s.offs):
        u = int(np.nonzero(offs[:s.nunits + 1] != s.offs)[0][0]) - 1
        raise AssertionError((what, "offsets", u, _where(fam, s, [u])))
    n = len(s.packed)
    bad = np.nonzero(got[:n] != s.packed)[0]
    units = np.unique(np.searchsorted(s.offs, bad, side="right") - 1)
    assert len(bad) == 0, (what, "bytes", len(units), _where(fam, s, units[:5]))


@pytest.mark.parametrize("name,d1", FORMS)
def test_device_stream_meets_the_census(name, d1):
    """the mode floor of tests/test_lists_tails_cpu.py, on the bytes the device wrote"""
    fam = lt.family(name)
    got, offs = _encoded(name, d1, 0)
    assert lt.check_floor(fam, lt.census(fam, got, offs, fam.form(d1).base)) >= 1


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Old:
    """the oracle's composition of the old lists of an append or a remove, with the table of its definition"""

    def __init__(self, lists, d1, start0):
        self.lists, self.d1 = lists, d1
        self.packed, self.offs, self.ptr, _ = ref.compose(lists, d1, start0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.nunits = len(self.offs) - 1
        self.table = rr.table(lists)


def _outputs(out_cap, units_cap, nlists):
    return dict(out=Guarded8(out_cap), off=li.Guarded64(torch, units_cap + 1), lptr=li.Guarded64(torch, nlists + 1),
                lunit=li.Guarded32(torch, nlists + 1), ulast=li.Guarded32(torch, units_cap))


def _same_index(fam, d1, g, what):
    """bytes, offsets, list_ptr, list_unit and with delta-1 the skip table are the family's own index"""
    s = fam.form(d1)
    r = {k: _read(v, k) for k, v in g.items()}
    assert np.array_equal(r["lptr"].view(np.uint64), s.ptr), what
    assert np.array_equal(r["lunit"], s.base), what
    _same_stream(fam, s, r["out"], r["off"].view(np.uint64), what)
    assert (r["off"][s.nunits + 1:] == SENT64).all()
    if d1:
        bad = np.nonzero(r["ulast"][:s.nunits] != fam.index().table)[0]
        assert len(bad) == 0, (what, "table", len(bad), _where(fam, s, bad[:5]))
    assert (r["ulast"][s.nunits if d1 else 0:] == SENT).all()


def _inputs(old, d1, start0):
    return (li.dev8(torch, old.packed), li.dev64(torch, old.offs), li.dev64(torch, old.ptr), li.dev32(torch, old.base),
            li.dev32(torch, start0) if d1 else None, li.dev32(torch, np.concatenate([old.table, [0]])) if d1 else None)


@pytest.mark.parametrize("name,d1", FORMS)
def test_append(name, d1):
    """every list L of the family cut at o: the old index holds L[:o], the addition is L[o:], o cycling over 0, 1, len // 2,
    len - 1 and behind a full block also 255, 256, 257 -- the result is the family's own index"""
    fam = lt.family(name)
    lists = fam.values(d1)
    turn, cuts = [0, 0], []
    for j, v in enumerate(lists):
        n, f = len(v), int(fam.front[j])
        opts = [0, 1, n // 2, n - 1] + ([255, 256, 257] if f else [])
        cuts.append(min(max(opts[turn[f] % len(opts)], 0), n))
        turn[f] += n > 0
    assert {c for c, f in zip(cuts, fam.front) if f} >= {0, 1, 255, 256, 257}
    old = Old([v[:o] for v, o in zip(lists, cuts)], d1, fam.start0)
    adds = [v[o:] for v, o in zip(lists, cuts)]
    add, aptr = np.concatenate(adds + [np.full(7, 0xDEADBEEF, np.uint32)]), sc._starts([len(a) for a in adds])
    L = tpf.lib()
    out_cap = int(L.tpf_lists_append_bound(len(old.packed), fam.nlists, len(add)))
    units_cap = int(L.tpf_lists_append_units_bound(old.nunits, fam.nlists, len(add)))
    g = _outputs(out_cap, units_cap, fam.nlists)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_in, d_off, d_ptr, d_base, d_st, d_tab = _inputs(old, d1, fam.start0)
    d_add, d_aptr = li.dev32(torch, add), li.dev64(torch, aptr)
    ws = torch.empty(max(int(L.tpf_lists_append_workspace_size(old.nunits, fam.nlists, len(add))), 1), dtype=torch.uint8, device=DEV)
    rc = L.tpf_lists_append(_p(d_in), len(old.packed), _p(d_off), old.nunits, _p(d_ptr), _p(d_base), fam.nlists, int(d1), _p(d_st),
                            _p(d_tab), _p(d_add), len(add), _p(d_aptr), fam.nlists, _p(g["out"].view), out_cap, _p(g["off"].view),
                            units_cap, _p(g["lptr"].view), _p(g["lunit"].view), _p(g["ulast"].view), _p(ws), ws.numel(), _p(err),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tpf_last_error()
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    _same_index(fam, d1, g, "append")


def _inserted(fam, j, v, idx, d1, rng):
    """Values to insert before v[idx[i]] (idx ascending, distinct).  Plain, and delta-1 in "wide" whose lists wrap: any value
    is a valid predecessor mod 2^32.  "ascending": a value strictly between its neighbours where there is one, so the old
    list ascends too; between consecutive doc ids there is none, and the predecessor's value is repeated -- a gap of
    0xFFFFFFFF, consistent mod 2^32, which the remove never orders by."""
    if not d1 or fam.name == "wide":
        return rng.integers(0, 1 << 32, size=len(idx), dtype=np.uint64).astype(np.uint32)
    ext = np.concatenate([[int(fam.start0[j])], v.astype(np.int64), [int(v[-1]) + 1000]])
    lo, hi = ext[idx], ext[idx + 1]
    room = hi - lo - 1
    return np.where(room > 0, lo + 1 + rng.integers(0, 1 << 30, size=len(idx)) % np.maximum(room, 1), lo).astype(np.uint32)


@pytest.mark.parametrize("name,d1", FORMS)
def test_remove(name, d1):
    """the old index holds the family's lists with extra values; the request removes exactly those: one at position 0, one at
    the last position, every other position from the tail's first on, and behind a full block one inside the block, one at
    255 and one at 256 -- the result is the family's own index"""
    fam = lt.family(name)
    lists = fam.values(d1)
    rng = np.random.default_rng(13)
    turn, olds, removals, used = [0, 0], [], {}, set()
    for j, v in enumerate(lists):
        n, cnt, f = len(v), int(fam.cnt[j]), int(fam.front[j])
        if n == 0:
            olds.append(v)
            continue
        pats = ["first", "last", "alt"] + (["inblock", "p255", "p256"] if f else [])
        pat = pats[turn[f] % len(pats)]
        turn[f] += 1
        used.add((pat, f))
        at = {"first": [0], "last": [n], "alt": (n - cnt) + 2 * np.arange(cnt), "inblock": [100], "p255": [255], "p256": [256]}[pat]
        at = np.asarray(at, dtype=np.int64)            # positions in the OLD list
        idx = at - np.arange(len(at))                  # each lands before v[idx]
        olds.append(np.insert(v, idx, _inserted(fam, j, v, idx, d1, rng)))
        removals[j] = at
    assert len(used) == 9
    c = rr.Case(olds, removals, d1, fam.start0, ptr0=0, pos0=0)
    s = fam.form(d1)
    assert np.array_equal(c.xpacked, s.packed) and np.array_equal(c.xoffs, s.offs)  # np.delete gives the family's lists back
    if name == "ascending":
        assert sum(np.all(np.diff(np.concatenate([[st], o]).astype(np.int64)) > 0) for o, st in zip(olds, fam.start0)) > fam.nlists // 2
    L = tpf.lib()
    stage = c.targeted
    out_cap = int(L.tpf_lists_remove_bound(len(c.packed), c.nq, stage))
    g = _outputs(out_cap, c.nunits, fam.nlists)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_in, d_off, d_ptr, d_base, d_st, d_tab = _inputs(c, d1, fam.start0)
    d_pos, d_pptr, d_ql = li.dev32(torch, c.pos), li.dev64(torch, c.pptr), li.dev32(torch, np.concatenate([c.qlist, [0]]))
    ws = torch.empty(max(int(L.tpf_lists_remove_workspace_size(c.nunits, fam.nlists, c.nq, len(c.pos), stage)), 1), dtype=torch.uint8,
                     device=DEV)
    rc = L.tpf_lists_remove(_p(d_in), len(c.packed), _p(d_off), c.nunits, _p(d_ptr), _p(d_base), fam.nlists, int(d1), _p(d_st),
                            _p(d_tab), _p(d_pos), len(c.pos), _p(d_pptr), _p(d_ql), c.nq, stage, _p(g["out"].view), out_cap,
                            _p(g["off"].view), c.nunits, _p(g["lptr"].view), _p(g["lunit"].view), _p(g["ulast"].view), _p(ws),
                            ws.numel(), _p(err), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tpf_last_error()
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    _same_index(fam, d1, g, "remove")
