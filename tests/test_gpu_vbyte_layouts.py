"""Every route that parses compressed vbyte exceptions, on the layout families of
tests/vbyte_layouts.py: V past two 64-byte windows, values that end on and around
every window boundary, the short form of the phase-A lane sums at every run
length and parity, up to 129 exceptions from the encoder and up to 255 in 16
windows in the decode-only family.  Everything is bit-exact against the oracle
(tests/test_vbyte_layouts_cpu.py holds the families to their classes and the
oracle to the reference); the packed bytes stand at byte shifts 0..3 past a
16-byte boundary so that every V meets every dword residue; every output lies
in a sentinel-guarded buffer and every call reports a clean d_err."""
import ctypes
import functools
import types

import numpy as np
import pytest

import lists_difference_ref as dr
import lists_index as li
import lists_ref as ref
import lists_remove_ref as rr
import lists_scale as sc
import lists_union_ref as ur
import vbyte_layouts as vl
from guarded import Guarded
from lists_index import CLEAN, DEV

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SHIFTS = (0, 1, 2, 3)
FILL8 = 0xA5
KINDS = ("reachable", "decode_only")


def to_dev(arr, W):
    if W == 32:
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(DEV)


@functools.lru_cache(maxsize=None)
def _src(kind, fmt, n):
    """One family in both forms: packed / off (the same bytes serve both), gaps, chained (the one delta-1 list from start0),
    starts (the value before each unit), names(units) for a failure's message."""
    if kind == "decode_only":
        d = vl.decode_only(fmt, n)
        return types.SimpleNamespace(fmt=fmt, n=n, W=32, nu=d.nu, packed=d.packed, off=d.off, gaps=d.gaps, chained=d.chained, starts=d.starts,
                                     start0=d.start0, names=d.names, width=d.units.shape[1])
    c, cd = vl.layout_case(fmt, n, False), vl.layout_case(fmt, n, True)
    return types.SimpleNamespace(fmt=fmt, n=n, W=c.W, nu=c.nu, packed=c.packed, off=c.off, gaps=c.gaps, chained=cd.vals, starts=cd.starts,
                                 start0=cd.start0, names=c.names, width=c.units.shape[1])


class Out:
    """a guarded output of `count` values of W bits and a guarded d_err"""

    def __init__(self, count, W):
        self.W = W
        self.vals = Guarded(count * W // 8, mis=16)
        self.err = Guarded(8, mis=8)
        self.err.view.zero_()
        self.tensor = self.vals.as_(torch.int32 if W == 32 else torch.int64)
        self.d_err = self.err.as_(torch.int64)

    def read(self, what):
        torch.cuda.synchronize()
        err, ok_e = self.err.read(np.int64)
        got, ok_v = self.vals.read(np.uint32 if self.W == 32 else np.uint64)
        assert ok_e and ok_v, ("written outside the output", what)
        assert int(err[0]) == CLEAN, (what, "d_err", int(err[0]))
        return got


def _same_units(s, got, want, what):
    got = got.reshape(s.nu, -1)[:, :s.n]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), s.names(bad))


# ---- the decode routes of the 256v32 hot path ------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_256v32_batch_decodes(kind, shift):
    """tpf_p4dec256v32_batch, its D1 form with per-block starts, tpf_dec_batch("256v32") in both forms"""
    s = _src(kind, "256v32", 256)
    packed, offs, starts = li.dev8(torch, s.packed, shift), li.dev64(torch, s.off), to_dev(s.starts, 32)
    for name, call in (("dec256v32", lambda o, st: tpf.dec256v32(packed, offs, s.nu, out=o.tensor.view(s.nu, 256), starts=st, err=o.d_err)),
                       ("dec_batch", lambda o, st: tpf.dec_batch("256v32", packed, offs, s.nu, 256, starts=st, err=o.d_err, out=o.tensor))):
        for st, want in ((None, s.gaps), (starts, s.chained)):
            o = Out(s.nu * 256, 32)
            call(o, st)
            _same_units(s, o.read(name), want, (name, kind, shift, "d1" if st is not None else "plain"))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_256v32_chained_decode(kind, shift):
    """tpf_p4d1dec256v32_chained, and chain_sums + chain_decode on their own: the phase-A lane sums (short form, general
    walk, and the wave decoder for what they decline) give every block's start and the list's total"""
    s = _src(kind, "256v32", 256)
    packed, offs = li.dev8(torch, s.packed, shift), li.dev64(torch, s.off)
    o = Out(s.nu * 256, 32)
    tpf.dec256v32_chained(packed, offs, s.nu, start0=s.start0, out=o.tensor.view(s.nu, 256), err=o.d_err)
    _same_units(s, o.read("chained"), s.chained, ("chained", kind, shift))
    o, total = Out(s.nu * 256, 32), Guarded(4, mis=4)
    ch = tpf.D1Chain(packed, offs, s.nu, total=total.as_(torch.int32))
    ch.sums(err=o.d_err)
    torch.cuda.synchronize()
    got_total, ok = total.read(np.uint32)
    assert ok and int(got_total[0]) == (int(s.chained[-1, -1]) - s.start0) & 0xFFFFFFFF, ("d_total", kind, shift)
    ch.decode(s.start0, out=o.tensor.view(s.nu, 256), err=o.d_err)
    _same_units(s, o.read("chain_decode"), s.chained, ("chain_sums + chain_decode", kind, shift))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_256v32_nstream_decode(kind, d1, shift):
    """tpf_p4ndec256v32: the family's full blocks and one p4Enc32 tail of the ("32", 255) family as one stream"""
    s, t = _src(kind, "256v32", 256), _src(kind, "32", 255)
    tail = t.nu // 2
    stream = np.concatenate([s.packed, t.packed[int(t.off[tail]): int(t.off[tail + 1])]])
    off = np.concatenate([s.off, [len(stream)]]).astype(np.uint64)
    gaps = np.concatenate([s.gaps.ravel(), t.gaps[tail]])
    want = (np.cumsum(gaps.astype(np.uint64) + np.uint64(1)) + np.uint64(s.start0)).astype(np.uint32) if d1 else gaps
    o = Out(len(gaps), 32)
    tpf.decn256v32(li.dev8(torch, stream, shift), li.dev64(torch, off), len(gaps), d1=d1, start0=s.start0, out=o.tensor, err=o.d_err)
    got = o.read("decn256v32")
    bad = np.unique(np.nonzero(got != want)[0] // 256)
    assert len(bad) == 0, ("decn256v32", kind, d1, shift, s.names(bad[bad < s.nu]), bad[bad >= s.nu])


# ---- every case through the generic decoder -------------------------------------------------------
CASES_KINDS = [(f, n, "reachable") for f, n in vl.CASES if (f, n) != ("256v32", 256)] + [("32", 255, "decode_only")]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("fmt,n,kind", CASES_KINDS)
def test_dec_batch(fmt, n, kind, shift):
    """tpf_dec_batch: vbyte_exceptions_g of every format, plain and with per-unit starts"""
    s = _src(kind, fmt, n)
    packed, offs = li.dev8(torch, s.packed, shift), li.dev64(torch, s.off)
    for st, want in ((None, s.gaps), (to_dev(s.starts, s.W), s.chained)):
        o = Out(s.nu * s.width, s.W)
        tpf.dec_batch(fmt, packed, offs, s.nu, n, starts=st, err=o.d_err, out=o.tensor)
        _same_units(s, o.read("dec_batch"), want, ("dec_batch", fmt, n, kind, shift, "d1" if st is not None else "plain"))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("named", [False, True])
@pytest.mark.parametrize("fmt,n", [("128v64", 128), ("256v64", 256)])
def test_chained64_decode(fmt, n, named, shift):
    """tpf_d1dec64_chained and the formats' own entry points, then chain_sums + chain_decode: the 64-bit lane sums"""
    s = _src("reachable", fmt, n)
    packed, offs = li.dev8(torch, s.packed, shift), li.dev64(torch, s.off)
    o = Out(s.nu * s.width, 64)
    tpf.dec64_chained(fmt, packed, offs, s.nu, start0=s.start0, out=o.tensor.view(s.nu, s.width), err=o.d_err, named=named)
    _same_units(s, o.read("chained64"), s.chained, ("chained64", fmt, named, shift))
    if named:
        return
    o, total = Out(s.nu * s.width, 64), Guarded(8, mis=8)
    ch = tpf.D1Chain64(fmt, packed, offs, s.nu, total=total.as_(torch.int64))
    ch.sums(err=o.d_err)
    torch.cuda.synchronize()
    got_total, ok = total.read(np.uint64)
    assert ok and int(got_total[0]) == (int(s.chained[-1, -1]) - s.start0) & 0xFFFFFFFFFFFFFFFF, ("d_total", fmt, shift)
    ch.decode(s.start0, out=o.tensor.view(s.nu, s.width), err=o.d_err)
    _same_units(s, o.read("chain_decode64"), s.chained, ("chain_sums + chain_decode", fmt, shift))


# ---- the lists routes --------------------------------------------------------------------------
class Resident:
    """vbyte_layouts.LayoutLists on the device, `shift` bytes past a 16-byte boundary, in one form"""

    def __init__(self, kind, d1, shift):
        ll = self.ll = vl.layout_lists(kind)
        self.d1 = d1
        self.lists = ll.lists(d1)
        self.s = types.SimpleNamespace(ptr=ll.ptr, vals=np.concatenate(self.lists), base=ll.base, nlists=ll.nlists, nunits=ll.nunits)
        self.table = np.array([v[min(256 * (i + 1), len(v)) - 1] for v in ll.lists(True) for i in range(-(-len(v) // 256))], dtype=np.uint32)
        self.packed = li.dev8(torch, ll.packed, shift)[:len(ll.packed)]
        self.offs, self.ptr, self.unit = li.dev64(torch, ll.offs), li.dev64(torch, ll.ptr), li.dev32(torch, ll.base)
        self.start0 = li.dev32(torch, ll.start0) if d1 else None
        self.last = li.dev32(torch, self.table) if d1 else None
        self.err = torch.zeros(1, dtype=torch.int64, device=DEV)

    def clean(self, what):
        torch.cuda.synchronize()
        assert int(self.err.item()) == CLEAN, (what, int(self.err.item()))

    def units_of_values(self, at):
        """the units that hold the values at the stream positions `at`"""
        ll = self.ll
        j = np.searchsorted(ll.ptr, np.asarray(at).astype(np.uint64), side="right") - 1
        return np.unique(ll.base[j].astype(np.int64) + (np.asarray(at, dtype=np.int64) - ll.ptr[j].astype(np.int64)) // 256)


def _read32(g, what):
    got, ok = g.read()
    assert ok, "written outside " + what
    return got.view(np.uint32) if got.dtype == np.int32 else got


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_lists_decode_select_units(kind, d1, shift):
    """tpf_p4ndec256v32_lists, tpf_lists_unit_last, ..._lists_select (every list, in a seeded order) and ..._lists_units
    (every list's whole range and every tail unit alone)"""
    r = Resident(kind, d1, shift)
    ll, s = r.ll, r.s
    out = li.Guarded32(torch, len(s.vals))
    tpf.decn256v32_lists(r.packed, r.offs, r.ptr, d1=d1, start0=r.start0, out=out.view, err=r.err)
    r.clean("lists decode")
    bad = np.nonzero(_read32(out, "out") != s.vals)[0]
    assert len(bad) == 0, ("lists decode", kind, d1, shift, ll.names(r.units_of_values(bad)))
    if d1:
        last = li.Guarded32(torch, ll.nunits)
        tpf.lists_unit_last(r.packed, r.offs, r.ptr, start0=r.start0, out=last.view, err=r.err)
        r.clean("unit_last")
        bad = np.nonzero(_read32(last, "unit_last") != r.table)[0]
        assert len(bad) == 0, ("unit_last", kind, shift, ll.names(bad))
    sel = np.random.default_rng(21).permutation(ll.nlists)
    want, wptr = sc.want_select(s, sel)
    out, optr = li.Guarded32(torch, len(want)), li.Guarded64(torch, len(sel) + 1)
    tpf.decn256v32_lists_select(r.packed, r.offs, r.ptr, r.unit, li.dev32(torch, sel), d1=d1, start0=r.start0, out=out.view,
                                out_ptr=optr.view, err=r.err)
    r.clean("select")
    assert np.array_equal(_read32(optr, "out_ptr"), wptr)
    got = _read32(out, "out")
    assert np.array_equal(got, want), ("select", kind, d1, shift, [int(sel[k]) for k in np.unique(np.searchsorted(wptr, np.nonzero(got != want)[0], "right") - 1)[:5]])
    units = np.diff(ll.base.astype(np.int64))
    tails = np.nonzero((np.diff(ll.ptr.astype(np.int64)) % 256 != 0) & (units > 1))[0]
    sel = np.concatenate([np.arange(ll.nlists), tails])
    ufirst = np.concatenate([np.zeros(ll.nlists, np.int64), units[tails] - 1])
    ucount = np.concatenate([units, np.ones(len(tails), np.int64)])
    order = np.random.default_rng(22).permutation(len(sel))
    sel, ufirst, ucount = sel[order], ufirst[order], ucount[order]
    want, wptr = sc.want_units(s, sel, ufirst, ucount)
    out, optr = li.Guarded32(torch, len(want)), li.Guarded64(torch, len(sel) + 1)
    tpf.decn256v32_lists_units(r.packed, r.offs, r.ptr, r.unit, li.dev32(torch, sel), li.dev32(torch, ufirst), li.dev32(torch, ucount), d1=d1,
                               start0=r.start0, unit_last=r.last, out=out.view, out_ptr=optr.view, err=r.err)
    r.clean("units")
    assert np.array_equal(_read32(optr, "out_ptr"), wptr)
    got = _read32(out, "out")
    assert np.array_equal(got, want), ("units", kind, d1, shift, [(int(sel[k]), int(ufirst[k])) for k in np.unique(np.searchsorted(wptr, np.nonzero(got != want)[0], "right") - 1)[:5]])


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_lists_gather(kind, d1, shift):
    """tpf_lists_gather: per list the first, the last and every 37th position, ascending and reversed -- every unit of
    every list is named, so every vbyte block is decoded by the item decoder"""
    r = Resident(kind, d1, shift)
    ll, s = r.ll, r.s
    qlist = np.arange(ll.nlists)
    for rev in (False, True):
        segs = []
        for g in ll.gaps:
            p = np.unique(np.concatenate([np.arange(0, len(g), 37), np.arange(255, len(g), 256), [len(g) - 1]]))
            segs.append(p[::-1] if rev else p)
        pos, pptr = np.concatenate(segs), sc._starts([len(x) for x in segs])
        want = sc.want_gather(ll.ptr, s.vals, qlist, pptr, pos)
        out = li.Guarded32(torch, len(pos))
        tpf.lists_gather(r.packed, r.offs, r.ptr, r.unit, li.dev32(torch, pos), li.dev64(torch, pptr), li.dev32(torch, qlist), d1=d1,
                         start0=r.start0, unit_last=r.last, out=out.view, err=r.err)
        r.clean("gather")
        got = _read32(out, "out")
        bad = np.nonzero(got != want)[0]
        ql = np.repeat(qlist, np.diff(pptr))
        assert len(bad) == 0, ("gather", kind, d1, shift, rev, len(bad), ll.names(np.unique(ll.base[ql[bad]].astype(np.int64) + pos[bad] // 256)))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_lists_unit_offsets(kind, shift):
    """tpf_lists_unit_offsets -- unit_size_serial and unit_size_wave's marker loop -- on the lists as they are and on
    every unit as a list of its own (a full block: 256 values; a tail: its count)"""
    ll = vl.layout_lists(kind)
    packed = li.dev8(torch, ll.packed, shift)[:len(ll.packed)]
    counts = np.concatenate([np.minimum(256, len(g) - 256 * np.arange(-(-len(g) // 256))) for g in ll.gaps])
    singles = (np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), ll.offs)
    for what, (ptr, lbyte) in (("lists", (ll.ptr, ll.list_byte)), ("one-unit lists", singles)):
        off, unit = li.Guarded64(torch, ll.nunits + 1), li.Guarded32(torch, len(ptr))
        err = torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.lists_unit_offsets(packed, li.dev64(torch, ptr), li.dev64(torch, lbyte), nunits=ll.nunits, out=off.view, list_unit=unit.view, err=err)
        torch.cuda.synchronize()
        assert int(err.item()) == CLEAN, (what, kind, shift, int(err.item()))
        got = _read32(off, "d_off").astype(np.uint64)
        bad = np.nonzero(np.diff(got.astype(np.int64)) != np.diff(ll.offs.astype(np.int64)))[0]
        assert len(bad) == 0 and np.array_equal(got, ll.offs), (what, kind, shift, ll.names(bad))
        want_unit = ll.base if what == "lists" else np.arange(ll.nunits + 1)
        assert np.array_equal(_read32(unit, "list_unit"), want_unit)


# ---- the set operations: probes that land in the vbyte blocks -----------------------------------------
@functools.lru_cache(maxsize=None)
def _ascending(kind):
    """vbyte_layouts.ascending_lists(kind) as a resident index -- the units' own bytes end to end, the directory and the
    skip table of its definition -- with one query per list: {v - 1, v, v + 1} over every third value, start0, the last
    value + 1 and 0xFFFFFFFF.  -> (index, label, qlist, probe, probe_ptr)"""
    lists, start0, label, fam = vl.ascending_lists(kind)
    if kind == "reachable":
        ix = li.Index(None, None, start0=start0, lists=lists)  # the oracle's composition: the same bytes
    else:
        ix = object.__new__(li.Index)
        ix.start0, ix.lists, ix.lens = start0, lists, [len(v) for v in lists]
        ix.vals = np.concatenate(lists)
        ix.ptr = np.concatenate([[0], np.cumsum(ix.lens)]).astype(np.uint64)
        ix.base = np.concatenate([[0], np.cumsum([len(lab) for lab in label])]).astype(np.uint32)
        ix.nlists, ix.nunits = len(lists), int(ix.base[-1])
        ix.table = np.array([v[min(256 * (i + 1), len(v)) - 1] for v in lists for i in range(-(-len(v) // 256))], dtype=np.uint32)
    parts = [fam[n].packed[int(fam[n].off[i]): int(fam[n].off[i + 1])] for lab in label for n, i in lab]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    if kind == "reachable":
        assert np.array_equal(ix.packed, np.concatenate(parts)) and np.array_equal(ix.offs, offs)
        held = {t for lab in label for n, i in lab if n == 256 for t in fam[256].tags[i]}
        need = set(vl.required_classes("256v32", 256))
        assert len(held & need) >= len(need) - 6 and {("W", w) for w in range(1, 6)} | {("xn", 127), ("xn", 128), ("xn", 129)} <= held
    else:
        ix.packed, ix.offs = np.concatenate(parts), offs
        held = {fam[n].label[i][:2] for lab in label for n, i in lab}
        assert held == {(x, k) for x in vl.DO_XN for k in vl.DO_KINDS} and max(fam[n].label[i][2] for lab in label for n, i in lab) == 16
    assert ix.ascends()
    segs = []
    for j, v in enumerate(lists):
        t = v[::3].astype(np.int64)
        marks = np.concatenate([t - 1, t, t + 1, [int(start0[j]), int(v[-1]) + 1, 0xFFFFFFFF]])
        segs.append(np.unique(np.clip(marks, 0, 0xFFFFFFFF)).astype(np.uint32))
    return ix, label, np.arange(len(lists)), np.concatenate(segs), sc._starts([len(x) for x in segs])


_SETOPS = {"intersect": (lambda: tpf.lists_intersect, lambda ix, q, pp, p: sc.want_hits(ix, q, pp, p)),
           "union": (lambda: tpf.lists_union, lambda ix, q, pp, p: ur.want_union_keys(ix, q, pp, p)),
           "difference": (lambda: tpf.lists_difference, lambda ix, q, pp, p: dr.want_difference_keys(ix, q, pp, p))}


@pytest.mark.parametrize("shift", (0, 3))
@pytest.mark.parametrize("op", list(_SETOPS))
@pytest.mark.parametrize("kind", KINDS)
def test_set_operation(kind, op, shift):
    """tpf_lists_intersect / union / difference on lists that ascend: the reachable units whose gaps stay below 2^28
    (all but a handful of the classes of each family: what needs an outlier past 25 bits over a wide base is left), and
    decode-only units of every exception count and kind, up to 16 windows: values, out_ptr, pidx and tpos against the
    numpy definitions"""
    ix, label, qlist, probe, pp = _ascending(kind)
    want = _SETOPS[op][1](ix, qlist, pp, probe)
    cap = len(probe) + (int(ix.ptr[-1]) if op == "union" else 0)
    out, pidx, tpos = (li.Guarded32(torch, cap) for _ in range(3))
    optr = li.Guarded64(torch, len(qlist) + 1)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    _SETOPS[op][0]()(li.dev8(torch, ix.packed, shift)[:len(ix.packed)], li.dev64(torch, ix.offs), li.dev64(torch, ix.ptr), li.dev32(torch, ix.base),
                     li.dev32(torch, ix.table), li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist), start0=li.dev32(torch, ix.start0),
                     out=out.view, out_ptr=optr.view, pidx=pidx.view, tpos=tpos.view, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    gptr = _read32(optr, "out_ptr")
    assert np.array_equal(gptr, want[1]), (op, "out_ptr")
    n = int(gptr[-1])
    for g, w, what in zip((out, pidx, tpos), (want[0], want[2], want[3]), ("values", "pidx", "tpos")):
        bad = np.nonzero(_read32(g, what)[:n] != w)[0]
        assert len(bad) == 0, (kind, op, what, shift, len(bad), [label[int(j)] for j in qlist[np.searchsorted(want[1], bad[:3], side="right") - 1]])


# ---- append and remove: the rebuilt stream is the families' own -----------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Old:
    """the oracle's composition of the old lists of an append or a remove, with the table of its definition"""

    def __init__(self, lists, d1, start0):
        self.packed, self.offs, self.ptr, _ = ref.compose(lists, d1, start0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.nunits = len(self.offs) - 1
        self.table = rr.table(lists)


def _outputs(out_cap, units_cap, nlists):
    return dict(out=torch.full((out_cap,), FILL8, dtype=torch.uint8, device=DEV), off=li.Guarded64(torch, units_cap + 1),
                lptr=li.Guarded64(torch, nlists + 1), lunit=li.Guarded32(torch, nlists + 1), ulast=li.Guarded32(torch, max(units_cap, 1)))


def _same_index(ll, d1, g, table, what):
    """bytes, offsets, list_ptr, list_unit and with delta-1 the skip table are those of the families' stream"""
    off = _read32(g["off"], "d_off").astype(np.uint64)[:ll.nunits + 1]
    bad = np.nonzero(np.diff(off.astype(np.int64)) != np.diff(ll.offs.astype(np.int64)))[0]
    assert len(bad) == 0 and np.array_equal(off, ll.offs), (what, "offsets", ll.names(bad))
    got = g["out"].cpu().numpy()
    diff = np.nonzero(got[:len(ll.packed)] != ll.packed)[0]
    assert len(diff) == 0, (what, "bytes", ll.names(np.unique(np.searchsorted(ll.offs, diff.astype(np.uint64), side="right") - 1)))
    assert np.array_equal(_read32(g["lptr"], "list_ptr").astype(np.uint64), ll.ptr), what
    assert np.array_equal(_read32(g["lunit"], "list_unit"), ll.base), what
    if d1:
        bad = np.nonzero(_read32(g["ulast"], "unit_last")[:ll.nunits] != table)[0]
        assert len(bad) == 0, (what, "table", ll.names(bad))


@pytest.mark.parametrize("d1", [False, True])
def test_append_rebuilds_the_stream(d1):
    """every list without its last value, which the append adds: the last unit of every list is re-encoded (a tail, or
    a tail of 255 values that becomes a full block) and every unit before it is carried over"""
    ll = vl.layout_lists("reachable")
    lists = ll.lists(d1)
    old = _Old([v[:-1] for v in lists], d1, ll.start0)
    add = np.concatenate([np.array([v[-1] for v in lists], dtype=np.uint32), np.full(7, 0xDEADBEEF, np.uint32)])
    aptr = np.arange(ll.nlists + 1, dtype=np.uint64)
    L = tpf.lib()
    out_cap = int(L.tpf_lists_append_bound(len(old.packed), ll.nlists, len(add)))
    units_cap = int(L.tpf_lists_append_units_bound(old.nunits, ll.nlists, len(add)))
    g = _outputs(out_cap, units_cap, ll.nlists)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_st = li.dev32(torch, ll.start0) if d1 else None
    d_tab = li.dev32(torch, np.concatenate([old.table, [0]])) if d1 else None
    d_in, d_off, d_ptr, d_base = li.dev8(torch, old.packed), li.dev64(torch, old.offs), li.dev64(torch, old.ptr), li.dev32(torch, old.base)
    d_add, d_aptr = li.dev32(torch, add), li.dev64(torch, aptr)
    ws = torch.empty(max(int(L.tpf_lists_append_workspace_size(old.nunits, ll.nlists, len(add))), 1), dtype=torch.uint8, device=DEV)
    rc = L.tpf_lists_append(_p(d_in), len(old.packed), _p(d_off), old.nunits, _p(d_ptr), _p(d_base), ll.nlists, int(d1), _p(d_st), _p(d_tab),
                            _p(d_add), len(add), _p(d_aptr), ll.nlists, _p(g["out"]), out_cap, _p(g["off"].view), units_cap, _p(g["lptr"].view),
                            _p(g["lunit"].view), _p(g["ulast"].view), _p(ws), ws.numel(), _p(err),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tpf_last_error()
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    _same_index(ll, d1, g, rr.table(ll.lists(True)), "append")


@pytest.mark.parametrize("d1", [False, True])
def test_remove_rebuilds_the_stream(d1):
    """every list with one extra value at a seeded position, which the remove deletes: every unit from that position
    on is decoded from the old stream and re-encoded into the families' own bytes"""
    ll = vl.layout_lists("reachable")
    lists = ll.lists(d1)
    rng = np.random.default_rng(23)
    at = [int(rng.integers(0, len(v) + 1)) for v in lists]
    at[:3] = (0, len(lists[1]), len(lists[2]) // 2)
    extra = rng.integers(0, 1 << 32, size=ll.nlists, dtype=np.uint64).astype(np.uint32)
    olds = [np.insert(v, p, x) for v, p, x in zip(lists, at, extra)]
    c = rr.Case(olds, {j: np.array([p], dtype=np.uint32) for j, p in enumerate(at)}, d1, ll.start0, ptr0=0, pos0=0)
    assert np.array_equal(c.xpacked, ll.packed) and np.array_equal(c.xoffs, ll.offs)
    L = tpf.lib()
    stage = c.targeted
    out_cap = int(L.tpf_lists_remove_bound(len(c.packed), c.nq, stage))
    g = _outputs(out_cap, c.nunits, ll.nlists)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_in, d_off, d_ptr, d_base = li.dev8(torch, c.packed), li.dev64(torch, c.offs), li.dev64(torch, c.ptr), li.dev32(torch, c.base)
    d_st = li.dev32(torch, ll.start0) if d1 else None
    d_tab = li.dev32(torch, np.concatenate([c.table, [0]])) if d1 else None
    d_pos, d_pptr, d_ql = li.dev32(torch, c.pos), li.dev64(torch, c.pptr), li.dev32(torch, np.concatenate([c.qlist, [0]]))
    ws = torch.empty(max(int(L.tpf_lists_remove_workspace_size(c.nunits, ll.nlists, c.nq, len(c.pos), stage)), 1), dtype=torch.uint8, device=DEV)
    rc = L.tpf_lists_remove(_p(d_in), len(c.packed), _p(d_off), c.nunits, _p(d_ptr), _p(d_base), ll.nlists, int(d1), _p(d_st), _p(d_tab),
                            _p(d_pos), len(c.pos), _p(d_pptr), _p(d_ql), c.nq, stage, _p(g["out"]), out_cap, _p(g["off"].view), c.nunits,
                            _p(g["lptr"].view), _p(g["lunit"].view), _p(g["ulast"].view), _p(ws), ws.numel(), _p(err),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tpf_last_error()
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    _same_index(ll, d1, g, rr.table(ll.lists(True)), "remove")


# ---- the encode routes (reachable families) ---------------------------------------------------------
def _same_stream(c, packed, offs, what):
    """offsets and bytes are the oracle's; a failure names the classes of the units that differ"""
    offs = np.asarray(offs).astype(np.uint64)
    if not np.array_equal(offs, c.off):
        bad = [0] if len(offs) != len(c.off) else np.nonzero(np.diff(offs.astype(np.int64)) != np.diff(c.off.astype(np.int64)))[0]
        raise AssertionError((what, "offsets", c.names(bad)))
    packed = np.asarray(packed)
    assert len(packed) == len(c.packed), what
    bad = np.nonzero(packed != c.packed)[0]
    assert len(bad) == 0, (what, "bytes", c.names(c.units_of_bytes(bad)))


@pytest.mark.parametrize("d1", [False, True])
def test_enc256v32_batch_entry(d1):
    """tpf_p4enc256v32_batch, plain, as one chained delta-1 list and with per-block starts; the buffer past the stream
    keeps its fill byte"""
    c = vl.layout_case("256v32", 256, d1)
    vals = to_dev(c.units, 32)
    cap = int(tpf.lib().tpf_p4enc256v32_bound(c.nu))
    kws = [dict(d1=True, start0=c.start0), dict(d1=True, starts=to_dev(c.starts, 32))] if d1 else [dict()]
    for kw in kws:
        out = torch.full((cap,), FILL8, dtype=torch.uint8, device=DEV)
        _, offs = tpf.enc256v32(vals, out=out, **kw)
        got, total = out.cpu().numpy(), int(offs[-1].item())
        _same_stream(c, got[:total], offs.cpu().numpy(), "enc256v32 " + ",".join(kw))
        assert (got[total:] == FILL8).all()


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("mode", [3, 4, 5])
def test_enc256v32_forced_routes(mode, d1):
    """3 = the two-pass encoder, 4 = the slot encoder with the fused planner, 5 = without"""
    c = vl.layout_case("256v32", 256, d1)
    cap = int(tpf.lib().tpf_p4enc256v32_bound(c.nu))
    out = torch.full((cap,), FILL8, dtype=torch.uint8, device=DEV)
    offs = tpf.enc256v32_path(mode, to_dev(c.units, 32), out, d1=d1, start0=c.start0 if d1 else 0)
    got, total = out.cpu().numpy(), int(offs[-1].item())
    _same_stream(c, got[:total], offs.cpu().numpy(), f"route {mode} d1={d1}")
    assert (got[total:total + 4096] == FILL8).all()


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("fmt,n", vl.CASES)
def test_enc_batch(fmt, n, d1):
    """tpf_enc_batch at every case, the hot path's included"""
    c = vl.layout_case(fmt, n, d1)
    kws = [dict(d1=True, start0=c.start0), dict(d1=True, starts=to_dev(c.starts, c.W))] if d1 else [dict()]
    for kw in kws:
        packed, offs = tpf.enc_batch(fmt, to_dev(c.units.ravel(), c.W), c.nu, n, **kw)
        _same_stream(c, packed.cpu().numpy(), offs.cpu().numpy(), f"{fmt} n={n} " + ",".join(kw))


@pytest.mark.parametrize("d1", [False, True])
def test_nstream_encoder(d1):
    """tpf_p4nenc256v32: the 256v32 family's blocks and a tail of the ("32", 255) family as one list"""
    c, t = vl.layout_case("256v32", 256, False), vl.layout_case("32", 255, False)
    tail = t.nu // 2
    gaps = np.concatenate([c.gaps.ravel(), t.gaps[tail]])
    want = np.concatenate([c.packed, t.packed[int(t.off[tail]): int(t.off[tail + 1])]])
    woff = np.concatenate([c.off, [len(want)]]).astype(np.uint64)
    vals = (np.cumsum(gaps.astype(np.uint64) + np.uint64(1)) + np.uint64(c.start0)).astype(np.uint32) if d1 else gaps
    packed, offs = tpf.encn256v32(to_dev(vals, 32), d1=d1, start0=c.start0)
    goff = offs.cpu().numpy().astype(np.uint64)
    bad = np.nonzero(np.diff(goff.astype(np.int64)) != np.diff(woff.astype(np.int64)))[0] if len(goff) == len(woff) else [0]
    assert len(bad) == 0, ("offsets", c.names([u for u in bad if u < c.nu]))
    diff = np.nonzero(packed.cpu().numpy() != want)[0]
    assert len(diff) == 0, ("bytes", c.names([u for u in np.unique(np.searchsorted(woff, diff.astype(np.uint64), side="right") - 1) if u < c.nu]))


@pytest.mark.parametrize("d1", [False, True])
def test_lists_encoder(d1):
    """tpf_p4nenc256v32_lists on the lists of the reachable families: full blocks through plan_block256, tails through
    plan_block_g"""
    ll = vl.layout_lists("reachable")
    vals = np.concatenate(ll.lists(d1))
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    cap = tpf.lists_enc_bound(len(vals), ll.nlists)
    out = torch.full((cap,), FILL8, dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(ll.nunits + 1, dtype=torch.int64, device=DEV)
    tpf.encn256v32_lists(li.dev32(torch, vals), li.dev64(torch, ll.ptr), d1=d1, start0=li.dev32(torch, ll.start0) if d1 else None,
                         nunits=ll.nunits, out=out, offsets=d_offs, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    got, goff = out.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    bad = np.nonzero(np.diff(goff.astype(np.int64)) != np.diff(ll.offs.astype(np.int64)))[0]
    assert len(bad) == 0 and np.array_equal(goff, ll.offs), ("offsets", ll.names(bad))
    diff = np.nonzero(got[:len(ll.packed)] != ll.packed)[0]
    assert len(diff) == 0, ("bytes", ll.names(np.unique(np.searchsorted(ll.offs, diff.astype(np.uint64), side="right") - 1)))
    assert (got[len(ll.packed):] == FILL8).all()


# ---- the per-block mirrors ----------------------------------------------------------------------
def _sample(c, limit=64):
    """units that hold every class of the case: the first unit of each class, then the units in order up to `limit`"""
    first = {}
    for i, tags in enumerate(c.tags):
        for t in tags:
            first.setdefault(t, i)
    need = vl.required_classes(c.fmt, c.n)
    picked = list(dict.fromkeys([first[t] for t in need]))
    return picked + [i for i in range(c.nu) if i not in picked][:max(0, limit - len(picked))]


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("fmt,n", vl.CASES)
def test_per_block_mirrors(fmt, n, d1):
    """tpf_p4Enc* / tpf_p4D1Enc* and the matching decoders, one unit per call: bytes, end pointer and values"""
    L = tpf.lib()
    c = vl.layout_case(fmt, n, d1)
    vt = ctypes.c_uint32 if c.W == 32 else ctypes.c_uint64
    enc_f = getattr(L, f"tpf_p4{'D1' if d1 else ''}Enc{fmt}")
    dec_f = getattr(L, f"tpf_p4{'D1' if d1 else ''}Dec{fmt}")
    for f in (enc_f, dec_f):
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p] + ([vt] if d1 else [])
        f.restype = ctypes.c_void_p
    for i in _sample(c):
        exp = c.packed[int(c.off[i]): int(c.off[i + 1])]
        st = [int(c.starts[i])] if d1 else []
        src = np.zeros(256 + 64, dtype=c.vals.dtype)
        src[:n] = c.vals[i]
        out = np.zeros(len(exp) + 4096, dtype=np.uint8)
        end = enc_f(src.ctypes.data, n, out.ctypes.data, *st)
        assert end is not None, L.tpf_last_error()
        assert end - out.ctypes.data == len(exp) and np.array_equal(out[: len(exp)], exp), (fmt, n, c.names([i]))
        enc = np.concatenate([exp, np.zeros(64, dtype=np.uint8)])
        dec = np.zeros(256 + 64, dtype=c.vals.dtype)
        end = dec_f(enc.ctypes.data, n, dec.ctypes.data, *st)
        assert end is not None, L.tpf_last_error()
        assert end - enc.ctypes.data == len(exp) and np.array_equal(dec[:n], c.vals[i]), (fmt, n, c.names([i]))


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("fmt,n", vl.DECODE_ONLY_CASES)
def test_per_block_decoders_on_decode_only_units(fmt, n, d1):
    """tpf_p4Dec* / tpf_p4D1Dec* on every unit of the decode-only family"""
    L = tpf.lib()
    d = vl.decode_only(fmt, n)
    dec_f = getattr(L, f"tpf_p4{'D1' if d1 else ''}Dec{fmt}")
    dec_f.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p] + ([ctypes.c_uint32] if d1 else [])
    dec_f.restype = ctypes.c_void_p
    for i in range(d.nu):
        enc = np.concatenate([d.packed[int(d.off[i]): int(d.off[i + 1])], np.zeros(64, dtype=np.uint8)])
        dec = np.zeros(256 + 64, dtype=np.uint32)
        end = dec_f(enc.ctypes.data, n, dec.ctypes.data, *([int(d.starts[i])] if d1 else []))
        assert end is not None, L.tpf_last_error()
        assert end - enc.ctypes.data == len(enc) - 64 and np.array_equal(dec[:n], d.chained[i] if d1 else d.gaps[i]), (fmt, n, d.names([i]))
