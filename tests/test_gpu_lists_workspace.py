"""GPU checks of the workspace contract of the lists entry points
(include/turbopfor_gpu.h): a call needs `*_workspace_size(...)` bytes and
nothing more, at an 8-byte-aligned base, whatever the bytes hold, and is
enqueued on the caller's stream with no synchronisation of its own.

a. Every entry point that takes d_ws runs on a view of exactly its size export
   inside a larger buffer, 4 KiB of sentinel before and after it, pre-filled
   with 0x00, with 0xFF and with the bytes another entry point left behind,
   and once more with the view's base at 8 (mod 16).  Outputs and d_err equal
   the expected result every time and both sentinel regions stay intact.
b. Chains of calls on a stream of their own, sharing one workspace, with no
   synchronisation in between.

The streams are the oracle's composition (tests/lists_ref.py through
tests/lists_index.py); the expected results are slices of the original lists
and tests/lists_scale.py's numpy statements -- never the code under test --
bit for bit."""
import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
import lists_scale as sc
from guarded import Workspace
from lists_index import CLEAN, DEV, SENT, SENT64, Index

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SMALL = [300, 0, 612, 256, 90, 0, 256 * 17]
SENT8 = 0xA5


class Small:
    """SMALL as an ascending delta-1 index and its plain twin, both resident."""

    def __init__(self):
        rng = np.random.default_rng(13)
        self.ix = Index(SMALL, rng, ptr0=11, start_bits=31)
        assert self.ix.ascends()
        self.tw = sc.Twin(self.ix, rng)
        self.ptr, self.base = li.dev64(torch, self.ix.ptr), li.dev32(torch, self.ix.base)
        self.start0, self.table = li.dev32(torch, self.ix.start0), li.dev32(torch, self.ix.table)
        self.dev = {d1: (li.dev8(torch, self.tw.stream(d1)[0]), li.dev64(torch, self.tw.stream(d1)[1])) for d1 in (True, False)}

    def vals(self, d1):
        return self.tw.stream(d1)[2]

    def st(self, d1):
        return self.start0 if d1 else None

    def tb(self, d1):
        return self.table if d1 else None


@pytest.fixture(scope="module")
def small():
    return Small()


def _s32(n):
    return torch.full((n,), SENT - (1 << 32), dtype=torch.int32, device=DEV)


def _s64(n):
    return torch.full((n,), SENT64, dtype=torch.int64, device=DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pad(a, n, sent=SENT):
    """`a` followed by the sentinel up to n entries: what a sentinel-filled output of n entries holds afterwards"""
    a = np.asarray(a)
    return np.concatenate([a, np.full(n - len(a), sent, a.dtype)])


def _size(name, *args):
    return int(getattr(tpf.lib(), name)(*args))


# ---- the nine entry points: each case is (workspace size, call(ws) -> outputs, expected outputs) -----------
def case_decode(S, d1):
    ix = S.ix
    packed, offs = S.dev[d1]
    cap, lo = int(ix.ptr[-1]), int(ix.ptr[0])

    def call(ws):
        out, err = _s32(cap), torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.decn256v32_lists(packed, offs, S.ptr, d1=d1, start0=S.st(d1), out=out, err=err, ws=ws)
        return dict(out=_u32(out), err=int(err.item()))

    want = dict(out=np.concatenate([np.full(lo, SENT, np.uint32), S.vals(d1)]), err=CLEAN)
    return _size("tpf_p4ndec256v32_lists_workspace_size", ix.nunits, ix.nlists), call, want


def case_encode(S, d1):
    ix = S.ix
    packed, offs, _ = S.tw.stream(d1)
    values = li.dev32(torch, np.concatenate([np.full(int(ix.ptr[0]), 0xDEADBEEF, np.uint32), S.vals(d1)]))
    cap = len(packed) + 40

    def call(ws):
        out = torch.full((cap,), SENT8, dtype=torch.uint8, device=DEV)
        d_offs, err = _s64(ix.nunits + 1), torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.encn256v32_lists(values, S.ptr, d1=d1, start0=S.st(d1), nunits=ix.nunits, out=out, offsets=d_offs, err=err, ws=ws)
        return dict(out=out.cpu().numpy(), offs=d_offs.cpu().numpy().view(np.uint64), err=int(err.item()))

    want = dict(out=_pad(packed, cap, SENT8), offs=offs, err=CLEAN)
    return _size("tpf_p4nenc256v32_lists_workspace_size", ix.nunits, ix.nlists), call, want


def case_unit_base(S, d1):
    ix = S.ix

    def call(ws):
        out, err = _s32(ix.nlists + 1), torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.lists_unit_base(S.ptr, out=out, err=err, ws=ws)
        return dict(out=_u32(out), err=int(err.item()))

    return _size("tpf_lists_unit_base_workspace_size", ix.nlists), call, dict(out=ix.base, err=CLEAN)


def case_select(S, d1):
    ix = S.ix
    packed, offs = S.dev[d1]
    sel = np.array([6, 0, 2, 2, 1, 4, 3, 5, 0])
    want_vals, want_ptr = sc.want_select(S.tw.ix if d1 else _Plain(S), sel)
    cap = len(want_vals) + 7
    d_sel = li.dev32(torch, sel)

    def call(ws):
        out, out_ptr, err = _s32(cap), _s64(len(sel) + 1), torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.decn256v32_lists_select(packed, offs, S.ptr, S.base, d_sel, d1=d1, start0=S.st(d1), out=out, out_ptr=out_ptr, err=err, ws=ws)
        return dict(out=_u32(out), out_ptr=out_ptr.cpu().numpy(), err=int(err.item()))

    want = dict(out=_pad(want_vals, cap), out_ptr=want_ptr, err=CLEAN)
    return _size("tpf_p4ndec256v32_lists_select_workspace_size", len(sel), cap), call, want


class _Plain:
    """the plain twin seen as an index: the delta-1 index's pointers and directory over the twin's values"""

    def __init__(self, S):
        self.ptr, self.base, self.table, self.nlists, self.vals = S.ix.ptr, S.ix.base, S.ix.table, S.ix.nlists, S.tw.fvals


def case_unit_last(S, d1):
    ix = S.ix
    packed, offs = S.dev[True]

    def call(ws):
        out, err = _s32(ix.nunits), torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.lists_unit_last(packed, offs, S.ptr, start0=S.start0, out=out, err=err, ws=ws)
        return dict(out=_u32(out), err=int(err.item()))

    return _size("tpf_lists_unit_last_workspace_size", ix.nunits, ix.nlists), call, dict(out=ix.table, err=CLEAN)


SEL8 = [(6, 2, 3), (0, 0, 2), (1, 0, 0), (2, 1, 2), (4, 0, 1), (5, 0, 0), (3, 0, 1), (0, 1, 1)]


def case_units(S, d1, cap=None):
    """cap = 14,336 values: the host's cap on the virtual units is 14,336 / 256 + 8 = 64, so the records of the virtual
    units -- UnWs's last array, cleared up to the cap by the plan -- are exactly 256 bytes."""
    packed, offs = S.dev[d1]
    sels = np.asarray(SEL8)
    want_vals, want_ptr = sc.want_units(S.ix if d1 else _Plain(S), sels[:, 0], sels[:, 1], sels[:, 2])
    cap = len(want_vals) + 7 if cap is None else cap
    d_sel, d_uf, d_uc = (li.dev32(torch, sels[:, i]) for i in range(3))

    def call(ws):
        out, out_ptr, err = _s32(cap), _s64(len(sels) + 1), torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.decn256v32_lists_units(packed, offs, S.ptr, S.base, d_sel, d_uf, d_uc, d1=d1, start0=S.st(d1), unit_last=S.tb(d1), out=out,
                                   out_ptr=out_ptr, err=err, ws=ws)
        return dict(out=_u32(out), out_ptr=out_ptr.cpu().numpy(), err=int(err.item()))

    want = dict(out=_pad(want_vals, cap), out_ptr=want_ptr, err=CLEAN)
    return _size("tpf_p4ndec256v32_lists_units_workspace_size", len(sels), cap), call, want


def case_units_256(S, d1):
    size, call, want = case_units(S, d1, cap=14336)
    assert 14336 // 256 + len(SEL8) == 64
    return size, call, want


def _one_per_unit(ix, rounds):
    """Queries of one request per unit of their list, neighbours on different lists: every request index is an item of its
    own.  -> (qlist, list-relative unit of every request, requests per query)"""
    qlist = [j for _ in range(rounds) for j in (6, 2, 0, 3, 4)]
    units = [np.arange(ix.units(j)) for j in qlist]
    return np.asarray(qlist), np.concatenate(units), np.array([len(u) for u in units])


def _requests(S, full):
    """full: 64 request indices, every one an item, none before the first segment or after the last -- the per-item arrays
    (IxWs's and GaWs's last array is iend) are exactly 256 bytes and written to their last entry.  Else 3 leading and 5
    trailing entries that belong to no query."""
    ix = S.ix
    qlist, urel, counts = _one_per_unit(ix, 2)
    if full:
        qlist, urel, counts = np.append(qlist, 6), np.concatenate([urel, np.arange(16)]), np.append(counts, 16)
        assert counts.sum() == 64
    ql = np.repeat(qlist, counts)
    cnt = np.minimum(256, np.asarray(ix.lens)[ql] - 256 * urel)
    lead, trail = (0, 0) if full else (3, 5)
    return qlist, ql, urel, cnt, lead + sc._starts(counts), lead, trail


def case_intersect(S, d1, full=False):
    ix = S.ix
    packed, offs = S.dev[True]
    rng = np.random.default_rng(19)
    qlist, ql, urel, cnt, pp, lead, trail = _requests(S, full)
    assert cnt.min() > 1
    at = sc.rel(ix)[ql] + 256 * urel + 1 + (rng.random(len(ql)) * (cnt - 1)).astype(np.int64)
    member = ix.vals[at].astype(np.int64)
    # about half members; the others one below a member and above the value before it: a non-member of the same unit
    gap = member - ix.vals[at - 1] > 1
    values = np.where(gap & (rng.random(len(ql)) < 0.5), member - 1, member).astype(np.uint32)
    probe = np.concatenate([np.full(lead, ix.vals[0], np.uint32), values, np.full(trail, ix.vals[0], np.uint32)])
    units = sc.probe_units(ix, ql, values)
    assert len(sc.item_heads(ql, units)) == len(ql)  # one item per probe value
    want_vals, want_ptr, want_pidx, want_tpos = sc.want_hits(ix, qlist, pp, probe)
    assert 10 < len(want_vals) < len(values)
    cap = len(probe)
    d_probe, d_pp, d_ql = li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist)

    def call(ws):
        out, pidx, tpos, out_ptr = _s32(cap), _s32(cap), _s32(cap), _s64(len(qlist) + 1)
        err = torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.lists_intersect(packed, offs, S.ptr, S.base, S.table, d_probe, d_pp, d_ql, start0=S.start0, out=out, out_ptr=out_ptr, pidx=pidx,
                            tpos=tpos, err=err, ws=ws)
        return dict(out=_u32(out), pidx=_u32(pidx), tpos=_u32(tpos), out_ptr=out_ptr.cpu().numpy(), err=int(err.item()))

    want = dict(out=_pad(want_vals, cap), pidx=_pad(want_pidx, cap), tpos=_pad(want_tpos, cap), out_ptr=want_ptr, err=CLEAN)
    return _size("tpf_lists_intersect_workspace_size", len(qlist), cap), call, want


def case_intersect_256(S, d1):
    return case_intersect(S, d1, full=True)


def case_gather(S, d1, full=False):
    ix = S.ix
    packed, offs = S.dev[d1]
    rng = np.random.default_rng(23)
    qlist, ql, urel, cnt, pp, lead, trail = _requests(S, full)
    positions = 256 * urel + (rng.random(len(ql)) * cnt).astype(np.int64)
    pos = np.concatenate([np.full(lead, 0xFFFFFFFF, np.uint32), positions.astype(np.uint32), np.full(trail, 0xFFFFFFFF, np.uint32)])
    assert len(sc.item_heads(ql, ix.base[ql].astype(np.int64) + urel)) == len(ql)  # one item per request index
    want_vals = sc.want_gather(ix.ptr, S.vals(d1), qlist, pp, pos)
    d_pos, d_pp, d_ql = li.dev32(torch, pos), li.dev64(torch, pp), li.dev32(torch, qlist)

    def call(ws):
        out, err = _s32(len(pos)), torch.zeros(1, dtype=torch.int64, device=DEV)
        tpf.lists_gather(packed, offs, S.ptr, S.base, d_pos, d_pp, d_ql, d1=d1, start0=S.st(d1), unit_last=S.tb(d1), out=out, err=err, ws=ws)
        return dict(out=_u32(out), err=int(err.item()))

    want = dict(out=np.concatenate([np.full(lead, SENT, np.uint32), want_vals, np.full(trail, SENT, np.uint32)]), err=CLEAN)
    return _size("tpf_lists_gather_workspace_size", len(qlist), len(pos)), call, want


def case_gather_256(S, d1):
    return case_gather(S, d1, full=True)


def case_append(S, d1):
    """SMALL with additions to five of its lists and two new lists: the result is the composition of old ++ added."""
    ix = S.ix
    adds = [0, 5, 300, 0, 256, 1, 100, 40, 0, 257]
    olds = list(ix.lens) + [0] * (len(adds) - ix.nlists)
    rng = np.random.default_rng(29)
    start0 = np.concatenate([ix.start0, rng.integers(0, 1 << 31, size=len(adds) - ix.nlists, dtype=np.uint64).astype(np.uint32)])
    old = list(ix.lists if d1 else S.tw.freqs) + [np.zeros(0, np.uint32)] * (len(adds) - ix.nlists)
    if d1:
        added = [ref.d1_values(a, int(v[-1]) if len(v) else int(s), rng) for v, s, a in zip(old, start0, adds)]
    else:
        added = [ref.plain_values(a, rng) for a in adds]
    full = [np.concatenate([v, a]) for v, a in zip(old, added)]
    xpacked, xoffs, xptr, _ = ref.compose(full, d1, start0)
    xbase = np.asarray(ref.units_loop(xptr)[1], dtype=np.uint32)
    xtable = np.array([v[min(256 * (i + 1), len(v)) - 1] for v in full for i in range(ref.n_units(len(v)))], dtype=np.uint32)
    xunits, nout = len(xoffs) - 1, len(adds)
    add = np.concatenate([np.full(5, 0xDEADBEEF, np.uint32)] + added + [np.full(7, 0xDEADBEEF, np.uint32)])
    aptr = (5 + sc._starts(adds)).astype(np.uint64)
    packed, offs = S.dev[d1]
    packed = packed[: len(S.tw.stream(d1)[0])]
    d_add, d_aptr, d_st = li.dev32(torch, add), li.dev64(torch, aptr), li.dev32(torch, start0) if d1 else None
    bytes_cap = tpf.lists_append_bound(packed.numel(), nout, len(add))
    units_cap = tpf.lists_append_units_bound(ix.nunits, nout, len(add))

    def call(ws):
        out = torch.full((bytes_cap,), SENT8, dtype=torch.uint8, device=DEV)
        out_offs, err = _s64(units_cap + 1), torch.zeros(1, dtype=torch.int64, device=DEV)
        _, _, lptr, lunit, ulast = tpf.lists_append(packed, offs, S.ptr, S.base, d_add, d_aptr, d1=d1, start0=d_st, unit_last=S.tb(d1),
                                                    out=out, out_offsets=out_offs, err=err, ws=ws)
        r = dict(out=out.cpu().numpy(), offs=out_offs.cpu().numpy().view(np.uint64), lptr=lptr.cpu().numpy().view(np.uint64),
                 lunit=_u32(lunit), err=int(err.item()))
        if d1:
            r["ulast"] = _u32(ulast)[:xunits]
        return r

    want = dict(out=_pad(xpacked, bytes_cap, SENT8), offs=_pad(xoffs, units_cap + 1, np.uint64(SENT64)), lptr=xptr, lunit=xbase, err=CLEAN)
    if d1:
        want["ulast"] = xtable
    return _size("tpf_lists_append_workspace_size", ix.nunits, nout, len(add)), call, want


def _donor(S, other):
    """The bytes a call of another entry point leaves in its workspace: the intersection's, or for the intersection and the
    gather (`other`) the delta-1 many-lists decode's."""
    size, call, _ = (case_decode if other else case_intersect)(S, True)
    ws = torch.zeros(size, dtype=torch.uint8, device=DEV)
    call(ws)
    assert bool((ws != 0).any())
    return ws


CASES = [(case_decode, False), (case_decode, True), (case_encode, False), (case_encode, True), (case_unit_base, None),
         (case_select, False), (case_select, True), (case_unit_last, True), (case_units, False), (case_units, True),
         (case_units_256, False), (case_units_256, True), (case_intersect, True), (case_intersect_256, True), (case_gather, False),
         (case_gather, True), (case_gather_256, False), (case_gather_256, True), (case_append, False), (case_append, True)]


def _compare(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("case,d1", CASES, ids=[f"{c.__name__[5:]}-{'d1' if d else 'plain' if d is not None else 'any'}" for c, d in CASES])
def test_known_contents_exact_size_and_guards(small, case, d1):
    """The last carved array of a workspace is padded to 256 bytes like every
    other, so an overrun of it by less than its padding shows only when its
    raw size is a multiple of 256.  That can be arranged where the last array
    is sized by the arguments alone: the records of the units decode (UnWs:
    rec, units_256) and the per-item ends of the intersection and the gather
    (IxWs / GaWs: iend, intersect_256 / gather_256).  Every other workspace
    ends in a run scan's tile totals and 256 spare bytes (ListsWs and UlWs
    through the chained decode's layout, ListsEncWs, SelWs, AppWs through the
    encoder's, the unit directory's), which no argument fills."""
    size, call, want = case(small, d1)
    assert size > 0 and size % 256 == 0
    donor = _donor(small, other=case in (case_intersect, case_intersect_256, case_gather, case_gather_256))
    for mis, fills in ((0, (0x00, 0xFF, donor)), (8, (donor,))):  # 8: the least alignment the header promises
        ws = Workspace(size, mis)
        for fill in fills:
            ws.fill(fill)
            what = (mis, fill if isinstance(fill, int) else "donor")
            _compare(call(ws.view), want, what)
            assert ws.intact(), what


# ---- b. a stream of its own, one workspace, no synchronisation between the calls -----------------------------
@pytest.fixture(scope="module")
def matrix():
    rng = np.random.default_rng(117)
    ix = Index([ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))], rng, ptr0=37, start_bits=31)
    assert ix.ascends()
    return ix, sc.Twin(ix, rng)


def _mixed_probe(ix, rng, per_query):
    """sorted probes of members and of values one below a member, one query per list in random order -> (qlist, probe_ptr, probe)"""
    qlist = rng.permutation(ix.nlists)
    segs = []
    for j in qlist:
        v = ix.lists[j]
        take = v[rng.integers(0, len(v), size=per_query)] if len(v) else np.zeros(0, np.uint32)
        segs.append(np.sort(np.where(rng.random(len(take)) < 0.5, take, np.maximum(take, 1) - 1).astype(np.uint32)))
    return qlist, sc._starts([len(s) for s in segs]), np.concatenate(segs)


def _xor_halves(a, rng):
    """two device tensors whose xor is `a`: the input of a call, produced on the stream just before it"""
    key = rng.integers(0, 1 << 32, size=len(a), dtype=np.uint64).astype(np.uint32)
    return li.dev32(torch, np.asarray(a, dtype=np.uint32) ^ key), li.dev32(torch, key)


def test_chain_on_a_stream_intersect_gather_intersect(matrix):
    ix, tw = matrix
    rng = np.random.default_rng(31)
    packed, offs, ptr, base = li.dev8(torch, ix.packed), li.dev64(torch, ix.offs), li.dev64(torch, ix.ptr), li.dev32(torch, ix.base)
    fpacked, foffs = li.dev8(torch, tw.fpacked), li.dev64(torch, tw.foffs)
    table, st = li.dev32(torch, ix.table), li.dev32(torch, ix.start0)
    q1, pp1, probe1 = _mixed_probe(ix, rng, 700)
    q2, pp2, probe2 = _mixed_probe(ix, rng, 300)
    n1, n2, nq = len(probe1), len(probe2), ix.nlists
    # expected, from the definitions
    v1, op1, _, tpos1 = sc.want_hits(ix, q1, pp1, probe1)
    v2, op2, pidx2, _ = sc.want_hits(ix, q2, pp2, probe2)
    freq = sc.want_gather(ix.ptr, tw.fvals, q1, op1, tpos1)
    assert len(v1) > 3000 and len(v2) > 1000
    half_a, half_b = _xor_halves(probe1, rng)
    d_pp1, d_q1 = li.dev64(torch, pp1), li.dev32(torch, q1)
    d_probe2, d_pp2, d_q2 = li.dev32(torch, probe2), li.dev64(torch, pp2), li.dev32(torch, q2)
    L = tpf.lib()
    ws_bytes = max(int(L.tpf_lists_intersect_workspace_size(nq, n1)), int(L.tpf_lists_gather_workspace_size(nq, n1)),
                   int(L.tpf_lists_intersect_workspace_size(nq, n2)))

    def chain(ws1, ws2, ws3, sync):
        d_probe1 = torch.bitwise_xor(half_a, half_b)  # a device op queued on the current stream just before the first call
        err = torch.zeros(3, dtype=torch.int64, device=DEV)
        out1, ptr1, tpos = _s32(n1), _s64(nq + 1), torch.full((n1,), -1, dtype=torch.int32, device=DEV)
        tpf.lists_intersect(packed, offs, ptr, base, table, d_probe1, d_pp1, d_q1, start0=st, out=out1, out_ptr=ptr1, tpos=tpos,
                            err=err[0:1], ws=ws1)
        sync()
        fr = _s32(n1)
        tpf.lists_gather(fpacked, foffs, ptr, base, tpos, ptr1, d_q1, d1=False, out=fr, err=err[1:2], ws=ws2)
        sync()
        out2, ptr2, pidx = _s32(n2), _s64(nq + 1), _s32(n2)
        tpf.lists_intersect(packed, offs, ptr, base, table, d_probe2, d_pp2, d_q2, start0=st, out=out2, out_ptr=ptr2, pidx=pidx,
                            err=err[2:3], ws=ws3)
        return err, out1, ptr1, tpos, fr, out2, ptr2, pidx

    torch.cuda.synchronize()
    fresh = [torch.empty(ws_bytes, dtype=torch.uint8, device=DEV) for _ in range(3)]
    apart = [t.cpu().numpy() for t in chain(*fresh, sync=torch.cuda.synchronize)]  # separately, fresh workspaces
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        queued = chain(ws, ws, ws, sync=lambda: None)
    stream.synchronize()  # once, at the end
    queued = [t.cpu().numpy() for t in queued]
    for a, b in zip(apart, queued):
        assert np.array_equal(a, b)
    err, out1, ptr1, tpos, fr, out2, ptr2, pidx = queued
    assert err.tolist() == [CLEAN, CLEAN, CLEAN]
    assert np.array_equal(ptr1, op1) and np.array_equal(out1.view(np.uint32), _pad(v1, n1))
    assert np.array_equal(tpos.view(np.uint32)[: len(v1)], tpos1)
    assert np.array_equal(fr.view(np.uint32), _pad(freq, n1))
    assert np.array_equal(ptr2, op2) and np.array_equal(out2.view(np.uint32), _pad(v2, n2))
    assert np.array_equal(pidx.view(np.uint32), _pad(pidx2, n2))


@pytest.mark.parametrize("d1", [False, True])
def test_chain_on_a_stream_encode_table_units(matrix, d1):
    ix, tw = matrix
    rng = np.random.default_rng(37)
    xpacked, xoffs, vals = tw.stream(d1)
    lo = int(ix.ptr[0])
    half_a, half_b = _xor_halves(np.concatenate([np.full(lo, 0xDEADBEEF, np.uint32), vals]), rng)
    ptr, base, st = li.dev64(torch, ix.ptr), li.dev32(torch, ix.base), li.dev32(torch, ix.start0) if d1 else None
    sels = []
    for _ in range(120):
        j = int(rng.integers(0, ix.nlists))
        uc = int(rng.integers(0, min(3, ix.units(j)) + 1))
        sels.append((j, int(rng.integers(0, ix.units(j) - uc + 1)), uc))
    sels = np.asarray(sels)
    src = ix if d1 else type("Plain", (), dict(ptr=ix.ptr, vals=tw.fvals))
    want_vals, want_ptr = sc.want_units(src, sels[:, 0], sels[:, 1], sels[:, 2])
    d_sel, d_uf, d_uc = (li.dev32(torch, sels[:, i]) for i in range(3))
    cap, nsel, total = len(xpacked) + 64, len(sels), len(want_vals)
    L = tpf.lib()
    ws_bytes = max(int(L.tpf_p4nenc256v32_lists_workspace_size(ix.nunits, ix.nlists)),
                   int(L.tpf_lists_unit_last_workspace_size(ix.nunits, ix.nlists)),
                   int(L.tpf_p4ndec256v32_lists_units_workspace_size(nsel, total)))

    def chain(ws1, ws2, ws3, sync):
        values = torch.bitwise_xor(half_a, half_b)  # a device op queued on the current stream just before the first call
        err = torch.zeros(3, dtype=torch.int64, device=DEV)
        packed, offs = torch.full((cap,), SENT8, dtype=torch.uint8, device=DEV), _s64(ix.nunits + 1)
        tpf.encn256v32_lists(values, ptr, d1=d1, start0=st, nunits=ix.nunits, out=packed, offsets=offs, err=err[0:1], ws=ws1)
        sync()
        table = _s32(ix.nunits)
        if d1:
            tpf.lists_unit_last(packed, offs, ptr, start0=st, out=table, err=err[1:2], ws=ws2)
        else:
            err[1:2].fill_(-1)  # a plain stream has no skip table
        sync()
        out, out_ptr = _s32(total), _s64(nsel + 1)
        tpf.decn256v32_lists_units(packed, offs, ptr, base, d_sel, d_uf, d_uc, d1=d1, start0=st, unit_last=table if d1 else None, out=out,
                                   out_ptr=out_ptr, err=err[2:3], ws=ws3)
        return err, packed, offs, table, out, out_ptr

    torch.cuda.synchronize()
    fresh = [torch.empty(ws_bytes, dtype=torch.uint8, device=DEV) for _ in range(3)]
    apart = [t.cpu().numpy() for t in chain(*fresh, sync=torch.cuda.synchronize)]  # separately, fresh workspaces
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        queued = chain(ws, ws, ws, sync=lambda: None)
    stream.synchronize()  # once, at the end
    queued = [t.cpu().numpy() for t in queued]
    for a, b in zip(apart, queued):
        assert np.array_equal(a, b)
    err, packed, offs, table, out, out_ptr = queued
    assert err.tolist() == [CLEAN, CLEAN, CLEAN]
    assert np.array_equal(packed, _pad(xpacked, cap, SENT8)) and np.array_equal(offs.view(np.uint64), xoffs)
    if d1:
        assert np.array_equal(table.view(np.uint32), ix.table)
    assert np.array_equal(out_ptr, want_ptr) and np.array_equal(out.view(np.uint32), want_vals)
