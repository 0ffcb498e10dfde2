"""GPU checks of the sub-index of a resident index (include/turbopfor_gpu.h
tpf_lists_extract): all six outputs -- bytes, offsets, both directories, the
delta-1 starts and the skip table -- are compared exactly with the numpy
definition (tests/lists_extract_ref.py: a byte slice of the oracle's
composition, held against the oracle's encoding of the sliced values in
tests/test_lists_extract_cpu.py).  Every output is a view between sentinels
and the C entry point is called directly, so the tables are guarded too."""
import ctypes
import types

import numpy as np
import pytest

import guarded
import lists_extract_ref as xr
import lists_index as li
import lists_ref as ref
import lists_scale as sc
from lists_index import CLEAN, DEV, SENT, SENT64

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SENT8 = 0xA5
TILE = 16384  # kListsAppendTile (csrc/p4_lists.h)
MODES = [(True, True), (True, False), (False, False)]  # (d1, with d_start0)
MODE_IDS = ["d1-start0", "d1-null", "plain"]


class Guarded8:
    """n bytes, `shift` bytes past a 16-byte boundary, inside a sentinel-filled buffer"""

    def __init__(self, n, shift):
        self.n = n
        self.big = torch.full((n + 96,), SENT8, dtype=torch.uint8, device=DEV)
        self.s = 32 + (shift - self.big.data_ptr() - 32) % 16
        self.view = self.big[self.s: self.s + n]
        assert self.view.data_ptr() % 16 == shift % 16 or n == 0

    def read(self):
        got = self.big.cpu().numpy()
        return got[self.s: self.s + self.n], bool((got[:self.s] == SENT8).all() and (got[self.s + self.n:] == SENT8).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _u32(a):
    return np.asarray(a, dtype=np.int64).astype(np.uint32)


class Call:
    """One call of the C entry point on index `src` (an xr.Source, an
    xr.Result or a lists_index.Index), every output guarded.  want: the
    definition's Result (default: computed); the keyword arguments replace one
    input each."""

    def __init__(self, src, sel, uf=None, uc=None, d1=None, want=None, shift_in=0, shift_out=0, out_cap=None, units_cap=None,
                 table=True, ulast_out=True, null_out=False, packed=None, offs=None, ptr=None, base=None, in_bytes=None, nunits=None,
                 nlists=None, ws=None):
        self.d1 = d1 = getattr(src, "d1", True) if d1 is None else d1
        self.want = want
        self.nsel = nsel = len(sel)
        self.nunits = len(src.offs) - 1 if nunits is None else nunits
        self.out_cap = len(want.packed) if out_cap is None else out_cap
        self.units_cap = want.nunits if units_cap is None else units_cap
        self.out = Guarded8(self.out_cap, shift_out)
        self.off = li.Guarded64(torch, self.units_cap + 1)
        self.lptr = li.Guarded64(torch, nsel + 1)
        self.lunit = li.Guarded32(torch, nsel + 1)
        self.st = li.Guarded32(torch, nsel)
        self.ulast = li.Guarded32(torch, self.units_cap)
        self.err = torch.zeros(1, dtype=torch.int64, device=DEV)
        start0 = getattr(src, "start0", None)
        self.keep = [
            li.dev8(torch, src.packed if packed is None else packed, shift_in),
            li.dev64(torch, src.offs if offs is None else offs),
            li.dev64(torch, src.ptr if ptr is None else ptr),
            li.dev32(torch, src.base if base is None else base),
            li.dev32(torch, start0) if d1 and start0 is not None else None,
            li.dev32(torch, np.concatenate([src.table, [0]])) if d1 and table else None,
            li.dev32(torch, np.concatenate([_u32(sel), [0]])),
            li.dev32(torch, np.concatenate([_u32(uf), [0]])) if uf is not None else None,
            li.dev32(torch, np.concatenate([_u32(uc), [0]])) if uf is not None else None,
        ]
        L = tpf.lib()
        self.ws = torch.empty(max(int(L.tpf_lists_extract_workspace_size(nsel)), 1), dtype=torch.uint8, device=DEV) if ws is None else ws
        k = self.keep
        self.args = [_p(k[0]), len(src.packed) if in_bytes is None else in_bytes, _p(k[1]), self.nunits, _p(k[2]), _p(k[3]),
                     len(src.ptr) - 1 if nlists is None else nlists, int(d1), _p(k[4]), _p(k[5]), _p(k[6]), _p(k[7]), _p(k[8]), nsel,
                     None if null_out else _p(self.out.view), self.out_cap, _p(self.off.view), self.units_cap, _p(self.lptr.view),
                     _p(self.lunit.view), _p(self.st.view), _p(self.ulast.view) if ulast_out else None, _p(self.ws), self.ws.numel(),
                     _p(self.err)]

    def launch(self):
        rc = tpf.lib().tpf_lists_extract(*self.args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, tpf.lib().tpf_last_error()
        return self

    def read(self):
        torch.cuda.synchronize()
        r = dict(err=int(self.err.item()))
        for name in ("out", "off", "lptr", "lunit", "st", "ulast"):
            r[name], ok = getattr(self, name).read()
            assert ok, "written outside " + name
        return r

    def run(self):
        return self.launch().read()

    def refill(self):
        """every output back to its sentinel, d_err to junk"""
        self.out.big.fill_(SENT8)
        for g in (self.off, self.lptr):
            g.big.fill_(SENT64)
        for g in (self.lunit, self.st, self.ulast):
            g.big.fill_(SENT - (1 << 32))
        self.err.fill_(0x77)

    def dirs(self, r):
        w = self.want
        assert np.array_equal(r["lptr"].view(np.uint64), w.ptr) and np.array_equal(r["lunit"], w.base)
        if self.d1:
            assert np.array_equal(r["st"], w.start0)
        else:
            assert (r["st"] == SENT).all()

    def tables(self, r, table=True):
        w = self.want
        u = w.nunits
        assert np.array_equal(r["off"][:u + 1].view(np.uint64), w.offs)
        assert (r["off"][u + 1:] == SENT64).all()
        if self.d1 and table:
            assert np.array_equal(r["ulast"][:u], w.table)
        assert (r["ulast"][u if self.d1 and table else 0:] == SENT).all()

    def check(self, r=None, table=True):
        """all six outputs equal the definition; nothing else is written inside the capacities"""
        r = self.read() if r is None else r
        assert r["err"] == CLEAN, r["err"] - self.nunits
        self.dirs(r)
        self.tables(r, table)
        n = len(self.want.packed)
        assert np.array_equal(r["out"][:n], self.want.packed)
        assert (r["out"][n:] == SENT8).all()
        return r


def call(src, sel, uf=None, uc=None, d1=None, **kw):
    d1 = getattr(src, "d1", True) if d1 is None else d1
    return Call(src, sel, uf, uc, d1, want=kw.pop("want", None) or xr.extract(src, sel, uf, uc, d1), **kw)


def untouched(r, names):
    for k in names:
        sent = {"out": SENT8, "off": SENT64, "lptr": SENT64}.get(k, SENT)
        assert (r[k] == sent).all(), k + " was written"


ALL = ("out", "off", "lptr", "lunit", "st", "ulast")


# ---- 1. whole lists ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole():
    out = {}
    lens = [0] + ref.MATRIX + [0, 0]
    for d1, st in MODES:
        rng = np.random.default_rng(77 + 2 * d1 + st)
        start0 = rng.integers(0, 1 << 31, size=len(lens), dtype=np.uint64).astype(np.uint32) if d1 and st else None
        out[d1, st] = xr.Source([xr.values(n, d1, start0[j] if start0 is not None else 0, rng) for j, n in enumerate(lens)], d1, start0)
    return out


def selections(src):
    n = src.nlists
    rng = np.random.default_rng(5)
    return {"identity": list(range(n)), "reversed": list(range(n))[::-1], "twice": [j for j in range(n) for _ in range(2)],
            "sparse": sorted(rng.choice(n, size=n // 3, replace=False).tolist()),
            "empties": [j for j, v in enumerate(src.lists) if len(v) == 0] * 2}


@pytest.mark.parametrize("which", ["identity", "reversed", "twice", "sparse", "empties"])
@pytest.mark.parametrize("d1,st", MODES, ids=MODE_IDS)
def test_whole_lists(whole, d1, st, which):
    src = whole[d1, st]
    sel = selections(src)[which]
    assert len(sel) >= 3
    shift = ["identity", "reversed", "twice", "sparse", "empties"].index(which) % 4
    c = call(src, sel, shift_in=shift, shift_out=(5 * shift + 1) % 16)
    c.launch().check()
    if which == "identity":
        assert np.array_equal(c.want.packed, src.packed) and np.array_equal(c.want.offs, src.offs)


def test_without_the_table_nothing_is_written_to_unit_last_out(whole):
    src = whole[True, True]
    sel = selections(src)["sparse"]
    call(src, sel, table=False).launch().check(table=False)
    call(src, sel, ulast_out=False).launch().check(table=False)


# ---- 2. unit ranges ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix():
    out = {}
    for d1, st in MODES:
        src = xr.matrix_source(d1, st)
        sel = xr.matrix_selection(src)
        out[d1, st] = (src, sel, xr.extract(src, *sel))
    return out


@pytest.mark.parametrize("shift_in", [0, 1, 2, 3])
@pytest.mark.parametrize("d1,st", MODES, ids=MODE_IDS)
def test_unit_ranges(matrix, d1, st, shift_in):
    src, sel, want = matrix[d1, st]
    call(src, *sel, want=want, shift_in=shift_in, shift_out=3 * shift_in).launch().check()


@pytest.mark.parametrize("d1,st", MODES, ids=MODE_IDS)
def test_unit_ranges_decode_to_the_sliced_values(matrix, d1, st):
    """Through the binding: the result goes through decn256v32_lists with start0_out and equals the sliced values, and
    lists_unit_last of the result is unit_last_out."""
    src, (sel, uf, uc), want = matrix[d1, st]
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    args = [li.dev8(torch, src.packed)[:len(src.packed)], li.dev64(torch, src.offs), li.dev64(torch, src.ptr), li.dev32(torch, src.base),
            li.dev32(torch, sel), li.dev32(torch, uf), li.dev32(torch, uc)]
    out, offs, lptr, lunit, st_out, ulast = tpf.lists_extract(
        *args, d1=d1, start0=li.dev32(torch, src.start0) if src.start0 is not None else None,
        unit_last=li.dev32(torch, src.table) if d1 else None, err=err)
    assert int(err.item()) == CLEAN and out.numel() == len(want.packed) and offs.numel() == want.nunits + 1
    assert np.array_equal(out.cpu().numpy(), want.packed)
    vals = tpf.decn256v32_lists(out, offs, lptr, d1=d1, start0=st_out, err=err)
    assert int(err.item()) == CLEAN
    sliced = np.concatenate(want.lists)
    assert np.array_equal(vals.cpu().numpy().view(np.uint32)[:len(sliced)], sliced)
    if d1:
        tab = tpf.lists_unit_last(out, offs, lptr, start0=st_out, err=err)
        assert int(err.item()) == CLEAN
        assert np.array_equal(tab.cpu().numpy().view(np.uint32)[:want.nunits], ulast.cpu().numpy().view(np.uint32)[:want.nunits])
        assert np.array_equal(ulast.cpu().numpy().view(np.uint32)[:want.nunits], want.table)
    else:
        assert st_out is None and ulast is None


# ---- 3. tile edges -----------------------------------------------------------------------------
class Pool:
    """Plain lists of known byte sizes: one-value lists of every size a value's width gives, a list of exactly 128 and
    one of exactly 129 bytes (the last a lane moves, the first wave_move takes), lists of 257 and 513 values and one
    that spans three tiles."""

    def __init__(self):
        rng = np.random.default_rng(99)
        one = [np.array([v], dtype=np.uint32) for v in (0, 200, 60000, (1 << 24) + 5, (1 << 31) + 5)]
        byte_lists = [rng.integers(128, 256, size=n, dtype=np.uint64).astype(np.uint32) for n in range(120, 134)]
        lists = one + byte_lists + [ref.plain_values(n, rng) for n in (257, 513, 256 * 130 + 77)]
        self.src = xr.Source(lists, False)
        self.size = [int(self.src.offs[self.src.base[j + 1]] - self.src.offs[self.src.base[j]]) for j in range(len(lists))]
        self.ones = list(range(len(one)))
        self.j128, self.j129 = self.size.index(128), self.size.index(129)
        self.j257, self.j513, self.jlong = len(lists) - 3, len(lists) - 2, len(lists) - 1
        assert self.size[self.jlong] > 3 * TILE and {2, 3} <= {self.size[j] for j in self.ones}

    def fill(self, nbytes):
        """one-value lists of exactly nbytes bytes together, the 2-byte ones by far the most"""
        by = sorted(((self.size[j], j) for j in self.ones), reverse=True)
        sel, left, turn = [], nbytes, 0
        while left:
            fits = [(s, j) for s, j in by if s <= left and left - s != 1]
            assert fits, left
            # a larger list now and then, 2-byte lists otherwise
            s, j = fits[0] if turn % 97 == 0 else [f for f in fits if f[0] <= 3][0]
            sel.append(j)
            left -= s
            turn += 1
        return sel


@pytest.fixture(scope="module")
def pool():
    return Pool()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_list_boundaries_at_a_tile_edge(pool, delta):
    """A list ends `delta` bytes from a multiple of 16,384 output bytes, after several thousand one-value lists (more
    than 64 lists of at most 128 bytes in one tile: further batches of the walk) with the 128- and the 129-byte list
    among them; a list of 513 values starts there, then the list that spans three tiles, then small ones again."""
    p = pool
    head = [p.j129, p.j128] + p.fill(300) + [p.j129]
    sel = head + p.fill(TILE + delta - sum(p.size[j] for j in head))
    assert sum(p.size[j] for j in sel) == TILE + delta and len(sel) > 4000
    sel += [p.j513, p.jlong] + p.fill(2 * TILE - (sum(p.size[j] for j in sel) + p.size[p.j513] + p.size[p.jlong]) % TILE + delta)
    sel += [p.j257, p.j128, p.j129]
    c = call(p.src, sel, shift_in=delta % 4, shift_out=(7 * delta) % 16)
    starts = c.want.offs[c.want.base[:-1]].astype(np.int64)
    assert (starts == TILE + delta).any() and ((starts % TILE == delta % TILE) & (starts > 4 * TILE)).any()
    c.launch().check()


@pytest.mark.parametrize("shift_out", range(16))
def test_every_alignment_of_d_out(pool, shift_out):
    p = pool
    sel = [p.j129, 1, p.j128, p.j257, 2, 0, p.j513, p.j129]
    call(p.src, sel, shift_in=shift_out % 4, shift_out=shift_out).launch().check()


# ---- 4. chains with no host step -----------------------------------------------------------------
@pytest.fixture(scope="module")
def index():
    rng = np.random.default_rng(31)
    ix = li.Index([0, 1, 255, 256, 257, 513, 256 * 17 + 3, 700, 0, 1500], rng, ptr0=11, start_bits=20)
    assert ix.ascends()
    return ix, sc.Twin(ix, rng)


def dev_index(ix, packed=None, offs=None):
    return [li.dev8(torch, ix.packed if packed is None else packed)[:len(ix.packed if packed is None else packed)],
            li.dev64(torch, ix.offs if offs is None else offs), li.dev64(torch, ix.ptr), li.dev32(torch, ix.base)]


def test_doc_id_window_of_both_streams(index):
    """lists_range_units -> lists_extract on the doc ids and on the frequencies stored in parallel, no host step between:
    each equals the definition for the ranges the search must give."""
    ix, twin = index
    qlist = [j for j in range(ix.nlists)] + [6, 9]
    qlo = [int(v[len(v) // 3]) if len(v) else 5 for v in ix.lists] + [0, int(ix.lists[9][-1]) + 1]
    qhi = [int(v[2 * len(v) // 3]) if len(v) else 9 for v in ix.lists] + [0xFFFFFFFF, 0xFFFFFFFF]
    uf, uc = sc.want_range(ix, qlist, qlo, qhi)
    assert (uc > 1).any() and (uf > 0).any() and (uc == 0).any()
    d_ql, d_tab, d_st = li.dev32(torch, qlist), li.dev32(torch, ix.table), li.dev32(torch, ix.start0)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_uf, d_uc = tpf.lists_range_units(li.dev32(torch, ix.base), d_tab, d_ql, li.dev32(torch, qlo), li.dev32(torch, qhi))
    units_cap = int(uc.sum())
    for d1 in (True, False):
        packed, offs, _ = twin.stream(d1)
        src = types.SimpleNamespace(d1=d1, lists=ix.lists if d1 else twin.freqs, start0=ix.start0 if d1 else None, packed=packed, offs=offs,
                                    ptr=ix.ptr, base=ix.base, table=ix.table if d1 else None)
        want = xr.extract(src, qlist, uf, uc)
        got = tpf.lists_extract(*dev_index(ix, packed, offs), d_ql, d_uf, d_uc, d1=d1, start0=d_st, unit_last=d_tab,
                                out=torch.empty(len(want.packed), dtype=torch.uint8, device=DEV), units_cap=units_cap, err=err)
        assert int(err.item()) == CLEAN
        for g, w in zip(got[:4], (want.packed, want.offs, want.ptr, want.base)):
            assert np.array_equal(g.cpu().numpy().view(w.dtype), w)
        if d1:
            assert np.array_equal(got[4].cpu().numpy().view(np.uint32), want.start0)
            assert np.array_equal(got[5].cpu().numpy().view(np.uint32)[:want.nunits], want.table)


def test_extract_of_an_extract_and_queries_on_the_result(index):
    """The result is an index like any other: a second extract of it equals the definition applied twice, and
    lists_intersect and lists_gather on it answer as they do on the source lists."""
    ix, _ = index
    sel1, uf1 = [9, 6, 2, 6, 0, 5, 7], [1, 3, 0, 0, 0, 1, 0]
    uc1 = [4, 12, 1, 18, 0, 2, 3]
    w1 = xr.extract(ix, sel1, uf1, uc1)
    d_tab, d_st = li.dev32(torch, ix.table), li.dev32(torch, ix.start0)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    r1 = tpf.lists_extract(*dev_index(ix), li.dev32(torch, sel1), li.dev32(torch, uf1), li.dev32(torch, uc1), d1=True, start0=d_st,
                           unit_last=d_tab, err=err)
    assert int(err.item()) == CLEAN and np.array_equal(r1[0].cpu().numpy(), w1.packed)
    sel2, uf2, uc2 = [3, 1, 1, 6, 0], [2, 0, 5, 1, 3], [16, 12, 3, 2, 1]
    w2 = xr.extract(w1, sel2, uf2, uc2)
    r2 = tpf.lists_extract(r1[0], r1[1], r1[2], r1[3], li.dev32(torch, sel2), li.dev32(torch, uf2), li.dev32(torch, uc2), d1=True,
                           start0=r1[4], unit_last=r1[5], err=err)
    assert int(err.item()) == CLEAN
    for g, w in zip(r2, (w2.packed, w2.offs, w2.ptr, w2.base, w2.start0, w2.table)):
        assert np.array_equal(g.cpu().numpy().view(w.dtype)[:len(w)], w)
    # queries: every list of the first result is probed with members and non-members, and read at positions
    rng = np.random.default_rng(8)
    queries = [(k, np.unique(np.concatenate([rng.choice(v, size=min(len(v), 40), replace=False), v[:1] + 1, v[-1:] + 7])))
               for k, v in enumerate(w1.lists) if len(v)]
    fake = type("Lists", (), {"lists": w1.lists})
    vals, out_ptr, pidx, tpos = li.want_hits(fake, queries, 0)
    probe = np.concatenate([pv for _, pv in queries])
    pptr = np.concatenate([[0], np.cumsum([len(pv) for _, pv in queries])])
    qlist = [k for k, _ in queries]
    d_pidx, d_tpos = (torch.empty(len(probe), dtype=torch.int32, device=DEV) for _ in range(2))
    got = tpf.lists_intersect(r1[0], r1[1], r1[2], r1[3], r1[5], li.dev32(torch, probe), li.dev64(torch, pptr), li.dev32(torch, qlist),
                              start0=r1[4], pidx=d_pidx, tpos=d_tpos, err=err)
    assert int(err.item()) == CLEAN
    nh = len(vals)
    assert np.array_equal(got[1].cpu().numpy(), out_ptr)
    for g, w in zip((got[0], d_pidx, d_tpos), (vals, pidx, tpos)):
        assert np.array_equal(g.cpu().numpy().view(np.uint32)[:nh], w)
    pos = [np.sort(rng.choice(len(w1.lists[k]), size=min(len(w1.lists[k]), 50), replace=False)) for k in qlist]
    gptr = np.concatenate([[0], np.cumsum([len(x) for x in pos])])
    out = tpf.lists_gather(r1[0], r1[1], r1[2], r1[3], li.dev32(torch, np.concatenate(pos)), li.dev64(torch, gptr), li.dev32(torch, qlist),
                           d1=True, start0=r1[4], unit_last=r1[5], err=err)
    assert int(err.item()) == CLEAN
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.concatenate([w1.lists[k][x] for k, x in zip(qlist, pos)]))


# ---- 5. errors -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def triples():
    """Lists in groups of three, the first of each group selected: what is done to the second and the third of a group
    touches no selected list's own entries but the [j + 1] ones."""
    rng = np.random.default_rng(3)
    lens = [513, 300, 257] * 9
    start0 = rng.integers(0, 1 << 31, size=len(lens), dtype=np.uint64).astype(np.uint32)
    src = xr.Source([xr.values(n, True, start0[j], rng) for j, n in enumerate(lens)], True, start0)
    sel = list(range(0, len(lens), 3))
    return src, sel, [1] * len(sel), [2] * len(sel)


REASONS = ["sel", "range", "wrap", "ptr", "span", "nunits", "order", "in_bytes"]


@pytest.mark.parametrize("reason", REASONS)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_refused_selection(triples, where, reason):
    """nunits + k for the first refused selection k, whatever the reason, and nothing is written in any output."""
    src, sel, uf, uc = triples
    k = {"first": 0, "middle": len(sel) // 2, "last": len(sel) - 1}[where]
    j = sel[k]
    sel, uf, uc = list(sel), list(uf), list(uc)
    kw = {}
    if reason == "sel":
        sel[k] = src.nlists
    elif reason == "range":
        uf[k], uc[k] = 3, 1
    elif reason == "wrap":
        uf[k], uc[k] = 0xFFFFFFFF, 2
    elif reason == "ptr":
        kw["ptr"] = src.ptr.copy()
        kw["ptr"][j + 1] = src.ptr[j] - 1
    elif reason == "span":
        kw["base"] = src.base.copy()
        kw["base"][j + 1] += 1
    elif reason == "nunits":
        kw["nunits"] = int(src.base[j + 1]) - 1  # every later selection fails too: the lowest code wins
    else:
        hi = int(src.base[j]) + 3  # the end of the copied range [1, 3): the first offset of the unselected list behind
        kw["offs"] = src.offs.copy()
        kw["offs"][hi] = src.offs[hi - 2] - 1 if reason == "order" else len(src.packed) + 1
    want = xr.extract(src, triples[1], triples[2], triples[3])
    c = Call(src, sel, uf, uc, True, want=want, **kw)
    r = c.run()
    assert r["err"] == c.nunits + k
    untouched(r, ALL)


def test_corruption_in_an_unselected_list_is_not_seen(triples):
    src, sel, uf, uc = triples
    offs, packed = src.offs.copy(), src.packed.copy()
    for j in sel:
        u = int(src.base[j + 1])          # the unselected list behind: its interior and end offsets, its bytes
        offs[u + 1], offs[u + 2] = 1 << 40, 0
        packed[int(src.offs[u]): int(src.offs[u + 2])] ^= 0xFF
    offs[int(src.base[sel[0]]) + 2] = 1 << 41  # an interior offset of a copied range is carried over, not checked
    c = call(src, sel, uf, uc, offs=offs, packed=packed)
    r = c.run()
    assert r["err"] == CLEAN
    c.dirs(r)
    assert np.array_equal(r["out"], c.want.packed)
    got, want = r["off"].view(np.uint64), c.want.offs
    assert got[1] == (1 << 41) - src.offs[int(src.base[sel[0]]) + 1] and np.array_equal(got[2:], want[2:])


@pytest.mark.parametrize("d1,st", MODES, ids=MODE_IDS)
def test_capacities_and_the_sizing_call(matrix, d1, st):
    src, sel, want = matrix[d1, st]
    nsel = len(sel[0])
    # units_cap one short: the directories and the starts only, completely
    c = call(src, *sel, want=want, units_cap=want.nunits - 1)
    r = c.run()
    assert r["err"] == c.nunits + nsel
    c.dirs(r)
    untouched(r, ("out", "off", "ulast"))
    # out_cap one byte short, and the sizing call (no d_out at all): everything but d_out
    for kw in (dict(out_cap=len(want.packed) - 1), dict(out_cap=0, null_out=True)):
        c = call(src, *sel, want=want, **kw)
        r = c.run()
        assert r["err"] == c.nunits + nsel + 1
        c.dirs(r)
        c.tables(r)
        untouched(r, ("out",))
        assert int(r["off"][int(r["lunit"][-1])]) == len(want.packed)  # what to allocate
    # exact capacities
    call(src, *sel, want=want).launch().check()


def test_no_selection_is_a_no_op(triples):
    src = triples[0]
    c = call(src, [])
    c.err.fill_(0x77)
    r = c.run()
    assert r["err"] == CLEAN and r["lptr"][0] == 0 and r["lunit"][0] == 0 and r["off"][0] == 0
    untouched(r, ("out", "st", "ulast"))


# ---- 6. workspace and graph ----------------------------------------------------------------------
def test_exact_dirty_workspace_and_graph_replay(matrix):
    """The workspace is exactly its export between guards, 8 bytes past a 16-byte boundary, and starts as 0x00, 0xFF
    and another call's bytes; one byte less is refused; the call captured in a graph is replayed after the workspace
    was overwritten with 0xFF."""
    src, sel, want = matrix[True, True]
    L = tpf.lib()
    size = int(L.tpf_lists_extract_workspace_size(len(sel[0])))
    ws = guarded.Guarded(size, mis=8)
    c = call(src, *sel, want=want, ws=ws.view)
    other = call(src, sel[0][::-1], ws=ws.view).launch()
    other.check()
    leftovers = ws.view.clone()
    for fill in (0x00, 0xFF, leftovers):
        ws.fill(fill)
        c.refill()
        c.launch().check()
        assert ws.intact()
    short = list(c.args)
    short[23] = size - 1
    assert L.tpf_lists_extract(*short, None) == -1 and b"workspace" in L.tpf_last_error()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        assert L.tpf_lists_extract(*c.args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    for fill in (0xFF, 0x00):
        ws.fill(fill)
        c.refill()
        graph.replay()
        c.check()
        assert ws.intact()


# ---- 7. past one grid ----------------------------------------------------------------------------
def test_more_selections_than_one_grid_covers():
    """nsel above lists_flat_cap: the plan and the heads kernels take a second trip.  Repeats of the short lists (and a
    few long ones) of a lists_scale index; the definition is stated vectorised and held against xr.extract on a prefix."""
    rng = np.random.default_rng(12)
    kinds = sc.Kinds(rng)
    ix = sc.ScaleIndex(kinds, kinds.choose(rng, 3000), ptr0=5)
    packed, offs = ix.stream(True)
    nsel = tpf.lists_flat_cap(DEV) + 777
    sel = rng.integers(0, ix.nlists, size=nsel)
    long_ = np.nonzero(ix.lens > 3)[0]
    sel = np.where(np.isin(sel, long_) & (rng.random(nsel) > 0.02), (sel + 1) % ix.nlists, sel)  # long lists stay few
    base, o = ix.base.astype(np.int64), offs.astype(np.int64)
    units, b0 = (base[sel + 1] - base[sel]), o[base[sel]]
    blen = o[base[sel + 1]] - b0
    lstart = np.concatenate([[0], np.cumsum(blen)])
    want = xr.Result()
    want.packed = sc.gather_segments(packed, b0, blen)
    want.offs = np.concatenate([np.repeat(lstart[:-1] - b0, units) + sc.gather_segments(o, base[sel], units), lstart[-1:]]).astype(np.uint64)
    want.ptr = np.concatenate([[0], np.cumsum(ix.lens[sel])]).astype(np.uint64)
    want.base = np.concatenate([[0], np.cumsum(units)]).astype(np.uint32)
    want.start0, want.table = ix.start0[sel], sc.gather_segments(ix.table, base[sel], units)
    want.nunits = int(want.base[-1])
    assert len(want.packed) < (64 << 20)
    # the vectorised statement against the definition, on the first selections
    ix.packed, ix.offs, ix.d1 = packed, offs, True
    ix.lists = [ix.vals[int(a): int(b)] for a, b in zip(ix.ptr - ix.ptr[0], (ix.ptr - ix.ptr[0])[1:])]
    few = xr.extract(ix, sel[:500])
    assert np.array_equal(few.packed, want.packed[:len(few.packed)]) and np.array_equal(few.offs, want.offs[:few.nunits + 1])
    assert np.array_equal(few.table, want.table[:few.nunits]) and np.array_equal(few.start0, want.start0[:500])
    Call(ix, sel, d1=True, want=want, shift_in=1, shift_out=9).launch().check()
