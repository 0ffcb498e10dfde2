"""GPU checks of the difference with a resident index (include/turbopfor_gpu.h
tpf_lists_difference) past every cap of its launcher
(csrc/p4_lists_difference.hip), and of its workspace contract.

The caps, each crossed by a test below that asserts the count it means to cross:
  - flat_grid (csrc/p4_lists_host.h; turbopfor_amd.lists_flat_cap threads): the
    grid-stride kernels over the probe values -- the intersection's plan and the
    compaction k_df_out;
  - one scan tile of 4,096 run totals (csrc/p4_scan.h): the two run scans over
    the probe's 64-index runs take a second launch above 262,144 probe values;
  - one trip of the lookup's full-block kernel k_ix_dec
    (turbopfor_amd.lists_item_cap items);
  - many queries, above 4,096, most of them empty: nq sizes nothing, the
    segment of a probe index is a search over d_probe_ptr.

The many-lists index is tests/lists_scale.py's; the expected results are
tests/lists_difference_ref.py's whole-request numpy statement of the definition
(held against np.setdiff1d by tests/test_lists_difference_cpu.py) -- never the
code under test -- and every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import lists_difference_ref as dr
import lists_index as li
import lists_scale as sc
from guarded import Workspace
from lists_index import CLEAN, DEV, SENT, SENT64, Index

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
PTR0, TRAIL, SLACK = 3, 5, 91
SMALL = [300, 0, 612, 256, 90, 0, 256 * 17]


def _s32(n):
    return torch.full((n,), SENT - (1 << 32), dtype=torch.int32, device=DEV)


def _s64(n):
    return torch.full((n,), SENT64, dtype=torch.int64, device=DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pad(a, n):
    return np.concatenate([a, np.full(n - len(a), SENT, np.uint32)])


class Resident:
    def __init__(self, ix, packed, offs):
        self.ix = ix
        self.packed, self.offs = li.dev8(torch, packed), li.dev64(torch, offs)
        self.ptr, self.base = li.dev64(torch, ix.ptr), li.dev32(torch, ix.base)
        self.start0, self.table = li.dev32(torch, ix.start0), li.dev32(torch, ix.table)


def _difference(R, probe, pp, qlist, cap, ws=None):
    """one call into sentinel-filled outputs of `cap` values -> dict of what they hold afterwards"""
    out, pidx, tpos, out_ptr = _s32(cap + SLACK), _s32(cap + SLACK), _s32(cap + SLACK), _s64(len(qlist) + 1)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.lists_difference(R.packed, R.offs, R.ptr, R.base, R.table, li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist),
                         start0=R.start0, out=out[:cap], out_ptr=out_ptr, pidx=pidx[:cap], tpos=tpos[:cap], err=err, ws=ws)
    return dict(out=_u32(out), pidx=_u32(pidx), tpos=_u32(tpos), out_ptr=out_ptr.cpu().numpy(), err=int(err.item()))


def _want(ix, probe, pp, qlist, cap):
    vals, out_ptr, pidx, tpos = dr.want_difference_keys(ix, qlist, pp, probe)
    assert len(vals) <= cap
    return dict(out=_pad(vals, cap + SLACK), pidx=_pad(pidx, cap + SLACK), tpos=_pad(tpos, cap + SLACK), out_ptr=out_ptr, err=CLEAN)


def _compare(got, want, what=None):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def scale():
    """40,000 lists, most of 1 to 3 values, a few of up to 17 units"""
    rng = np.random.default_rng(103)
    kinds = sc.Kinds(rng)
    ix = sc.ScaleIndex(kinds, kinds.choose(rng, 40000, big=0.01), ptr0=37)
    return ix, Resident(ix, *ix.stream(True))


def test_many_queries_mostly_empty_and_many_items(scale):
    """Far more queries than 4,096, most segments empty; more items than one trip of k_ix_dec covers."""
    ix, R = scale
    items = tpf.lists_item_cap(DEV)
    rng = np.random.default_rng(107)
    nq = 10 * items + 4097
    small = np.nonzero((ix.lens > 0) & (ix.lens <= 3))[0]
    qlist = small[rng.integers(0, len(small), size=nq)]
    empties = np.nonzero(ix.lens == 0)[0]
    e = rng.random(nq) < 0.05
    qlist[e] = empties[rng.integers(0, len(empties), size=int(e.sum()))]
    big = np.nonzero(ix.lens >= 256)[0]  # full blocks: the items of k_ix_dec
    at = rng.permutation(nq)[:200]
    qlist[at] = big[rng.integers(0, len(big), size=200)]
    # one probe value for 19% of the queries: the list's first value (half of them), the value below it or one far above the
    # list (no unit); on an empty list any value; 40 values for the queries on long lists
    r = sc.rel(ix)
    has = rng.random(nq) < 0.19
    counts = has.astype(np.int64)
    counts[at] = 40
    segs = np.zeros(int(counts.sum()), np.uint32)
    pp = PTR0 + sc._starts(counts)
    first = np.where(ix.lens[qlist] > 0, ix.vals[np.minimum(r[qlist], len(ix.vals) - 1)], 9).astype(np.int64)
    pick = rng.integers(0, 4, size=nq)
    one = np.where(pick < 2, first, np.where(pick == 2, first - 1, 0xF0000000 + (first & 0xFFFF)))
    single = has.copy()
    single[at] = False
    segs[(pp[:-1] - PTR0)[single]] = one[single].astype(np.uint32)
    for k in at:
        j = qlist[k]
        v = ix.vals[r[j]: r[j + 1]]
        pick = np.unique(np.concatenate([v[rng.integers(0, len(v), size=60)], v[rng.integers(0, len(v), size=60)] - 1]))
        pick = pick[np.sort(rng.permutation(len(pick))[:40])]
        assert len(pick) == 40
        segs[pp[k] - PTR0: pp[k + 1] - PTR0] = pick
    probe = np.concatenate([np.full(PTR0, 0xF0000001, np.uint32), segs, np.full(TRAIL, ix.vals[0], np.uint32)])
    assert nq > 4096 and (counts == 0).mean() > 0.8
    lists_of = np.repeat(qlist, counts)
    units = sc.probe_units(ix, lists_of, segs)
    heads = sc.item_heads(lists_of, units)
    assert len(heads) > items
    assert int((~sc.tail_units(ix)[units[heads]]).sum()) > 200 and (units < 0).sum() > 1000  # full-block items; values without a unit
    cap = len(segs) + 7
    got, want = _difference(R, probe, pp, qlist, cap), _want(ix, probe, pp, qlist, cap)
    assert 1000 < want["out_ptr"][-1] < len(segs) - 1000  # members and non-members
    _compare(got, want)


def test_probe_past_one_scan_tile_and_one_grid(scale):
    """More probe values than flat_grid has threads and than 262,144: the grid-stride kernels over the probe take a second trip,
    the run scans over its 64-index runs a second launch."""
    ix, R = scale
    flat = tpf.lists_flat_cap(DEV)
    j = int(np.nonzero(ix.lens == 256 * 17 + 3)[0][0])
    other = int(np.nonzero(ix.lens == 513)[0][0])
    r = sc.rel(ix)
    v = ix.vals[r[j]: r[j + 1]]
    m = max(flat, 64 * 4096) + 70001
    run = np.arange(int(v[1000]) - 5, int(v[1000]) - 5 + m, dtype=np.uint32)  # consecutive integers across a few units
    w = ix.vals[r[other]: r[other + 1]]
    segs = [w[::3], run, v[-300:] + np.arange(300, dtype=np.uint32) % 2]
    qlist = np.array([other, j, j])
    probe = np.concatenate([np.full(PTR0, 0xF0000001, np.uint32)] + segs + [np.full(TRAIL, v[0], np.uint32)])
    pp = PTR0 + sc._starts([len(s) for s in segs])
    assert len(probe) > flat and len(probe) > 64 * 4096
    cap = sum(len(s) for s in segs)
    want = _want(ix, probe, pp, qlist, cap)
    assert want["out_ptr"][1] == 0 and want["out_ptr"][-1] > flat and want["out_ptr"][-1] > 64 * 4096  # the scatter crosses both too
    _compare(_difference(R, probe, pp, qlist, cap), want)


# ---- the workspace contract (tests/test_gpu_lists_workspace.py's) -------------------------------------
class Small:
    def __init__(self):
        rng = np.random.default_rng(13)
        self.ix = Index(SMALL, rng, ptr0=11, start_bits=31)
        assert self.ix.ascends()
        self.R = Resident(self.ix, self.ix.packed, self.ix.offs)


@pytest.fixture(scope="module")
def small():
    return Small()


def _small_request(S, rng):
    ix = S.ix
    qlist = np.array([6, 2, 0, 3, 4, 1, 2, 0])
    segs = []
    for j in qlist:
        v = ix.lists[j]
        take = v[rng.integers(0, len(v), size=50)] if len(v) else np.array([5, 9], np.uint32)
        segs.append(np.unique(np.where(rng.random(len(take)) < 0.5, take, np.maximum(take, 1) - 1).astype(np.uint32)))
    probe = np.concatenate([np.full(PTR0, 0xF0000001, np.uint32)] + segs + [np.full(TRAIL, ix.vals[0], np.uint32)])
    return qlist, PTR0 + sc._starts([len(s) for s in segs]), probe


def test_known_contents_exact_size_and_guards(small):
    """Exactly tpf_lists_difference_workspace_size bytes between guards, pre-filled with 0x00, 0xFF and the bytes an
    intersection left, and once more at base 8 (mod 16): the same outputs each time."""
    S = small
    rng = np.random.default_rng(19)
    qlist, pp, probe = _small_request(S, rng)
    cap = len(probe)
    want = _want(S.ix, probe, pp, qlist, cap)
    assert 50 < want["out_ptr"][-1] < pp[-1] - pp[0] - 50
    size = int(tpf.lib().tpf_lists_difference_workspace_size(len(qlist), len(probe)))
    assert size > 0 and size % 8 == 0
    donor = torch.zeros(int(tpf.lib().tpf_lists_intersect_workspace_size(len(qlist), len(probe))), dtype=torch.uint8, device=DEV)
    tpf.lists_intersect(S.R.packed, S.R.offs, S.R.ptr, S.R.base, S.R.table, li.dev32(torch, probe), li.dev64(torch, pp),
                        li.dev32(torch, qlist), start0=S.R.start0, ws=donor)
    assert bool((donor != 0).any())
    for mis, fills in ((0, (0x00, 0xFF, donor)), (8, (donor, 0xFF))):  # 8: the least alignment the header promises
        ws = Workspace(size, mis)
        for fill in fills:
            ws.fill(fill)
            what = (mis, fill if isinstance(fill, int) else "donor")
            _compare(_difference(S.R, probe, pp, qlist, cap, ws=ws.view), want, what)
            assert ws.intact(), what


def test_workspace_one_byte_short_is_refused(small):
    S = small
    qlist, pp, probe = _small_request(S, np.random.default_rng(19))
    cap = len(probe)
    L = tpf.lib()
    size = int(L.tpf_lists_difference_workspace_size(len(qlist), len(probe)))
    ws = Workspace(size - 1)
    out, out_ptr = _s32(cap), _s64(len(qlist) + 1)
    d_probe, d_pp, d_ql = li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.tpf_lists_difference(p(S.R.packed), S.R.packed.numel(), p(S.R.offs), S.ix.nunits, p(S.R.ptr), p(S.R.base), S.ix.nlists,
                                p(S.R.start0), p(S.R.table), p(d_probe), len(probe), p(d_pp), p(d_ql), len(qlist), p(out), cap,
                                p(out_ptr), None, None, p(ws.view), size - 1, None, None)
    assert rc == -1 and b"tpf_lists_difference" in L.tpf_last_error() and b"workspace" in L.tpf_last_error()
    torch.cuda.synchronize()
    assert (_u32(out) == SENT).all() and (out_ptr.cpu().numpy() == SENT64).all() and ws.intact()


class Chain:
    """A AND NOT B AND NOT C for three queries at once, as two chained calls that share one workspace: the first call's
    (out, out_ptr) is the second's probe.  Every buffer is allocated here, so the calls themselves allocate nothing."""

    def __init__(self, S, ws):
        ix, self.R = S.ix, S.R
        self.ix = ix
        self.q1, self.q2 = np.array([2, 6, 0]), np.array([6, 0, 3])

        def seg(a, b, phase):
            """ascending: every second value of list a, every third of list b, and a neighbour of each that is (mostly) in neither"""
            A, B = ix.lists[a], ix.lists[b]
            ia = np.minimum(np.arange(0, len(A), 2) + phase, len(A) - 1)
            ib = np.minimum(np.arange(0, len(B), 3) + phase, len(B) - 1)
            return np.sort(np.concatenate([A[ia], B[ib], A[ia] - np.uint32(1), B[ib] + np.uint32(1)]))

        # two probes of the same lengths with other members: a captured graph serves both
        self.probes = [np.concatenate([seg(a, b, phase) for a, b in zip(self.q1, self.q2)]) for phase in (0, 1)]
        self.pp1 = sc._starts([len(seg(a, b, 0)) for a, b in zip(self.q1, self.q2)])
        self.n = len(self.probes[0])
        L = tpf.lib()
        self.ws_bytes = int(L.tpf_lists_difference_workspace_size(3, self.n))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV) if ws is None else ws
        self.d_probe = li.dev32(torch, self.probes[0])
        self.d_pp1, self.d_q1, self.d_q2 = li.dev64(torch, self.pp1), li.dev32(torch, self.q1), li.dev32(torch, self.q2)
        self.err = torch.zeros(2, dtype=torch.int64, device=DEV)
        self.out1, self.ptr1 = _s32(self.n), _s64(4)
        self.out2, self.ptr2, self.pidx, self.tpos = _s32(self.n), _s64(4), _s32(self.n), _s32(self.n)

    def load(self, which, fill):
        """the probe `which`, sentinels in every output and `fill` over the whole workspace"""
        self.d_probe.copy_(li.dev32(torch, self.probes[which]))
        for t in (self.out1, self.out2, self.pidx, self.tpos):
            t.fill_(SENT - (1 << 32))
        for t in (self.ptr1, self.ptr2):
            t.fill_(SENT64)
        self.err.zero_()
        self.ws.fill_(fill)

    def seq(self):
        R = self.R
        tpf.lists_difference(R.packed, R.offs, R.ptr, R.base, R.table, self.d_probe, self.d_pp1, self.d_q1, start0=R.start0,
                             out=self.out1, out_ptr=self.ptr1, err=self.err[0:1], ws=self.ws)
        tpf.lists_difference(R.packed, R.offs, R.ptr, R.base, R.table, self.out1, self.ptr1, self.d_q2, start0=R.start0,
                             out=self.out2, out_ptr=self.ptr2, pidx=self.pidx, tpos=self.tpos, err=self.err[1:2], ws=self.ws)

    def check(self, which):
        ix, n = self.ix, self.n
        v1, op1, _, _ = dr.want_difference_keys(ix, self.q1, self.pp1, self.probes[which])
        v2, op2, pidx2, tpos2 = dr.want_difference_keys(ix, self.q2, op1, v1)
        assert 100 < len(v2) < len(v1) - 20 < n - 100
        assert self.err.tolist() == [CLEAN, CLEAN]
        assert np.array_equal(self.ptr1.cpu().numpy(), op1) and np.array_equal(_u32(self.out1), _pad(v1, n))
        assert np.array_equal(self.ptr2.cpu().numpy(), op2) and np.array_equal(_u32(self.out2), _pad(v2, n))
        assert np.array_equal(_u32(self.pidx), _pad(pidx2, n)) and np.array_equal(_u32(self.tpos), _pad(tpos2, n))
        for k in range(3):
            seg = self.probes[which][self.pp1[k]: self.pp1[k + 1]]
            a, b = int(op2[k]), int(op2[k + 1])
            assert np.array_equal(v2[a:b], seg[~np.isin(seg, ix.lists[self.q1[k]]) & ~np.isin(seg, ix.lists[self.q2[k]])])


def test_chain_on_a_stream_sharing_one_workspace(small):
    """Two chained calls on a stream of their own, one workspace, no synchronisation in between."""
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = Chain(small, None)
        c.load(0, 0xFF)
        c.seq()
    stream.synchronize()  # once, at the end
    c.check(0)


def test_chain_captured_and_replayed_on_a_dirty_workspace(small):
    """One linear sequence on a single stream, no parallel branches, as tests/test_gpu_codec_workspace.py captures the codec
    calls: the launches depend on the sizes alone, so the graph serves another probe of the same length."""
    c = Chain(small, None)
    c.load(0, 0x00)
    c.seq()  # warm-up outside the capture (library load, first-launch setup)
    torch.cuda.synchronize()
    c.check(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.seq()
    for which in (1, 0):
        c.load(which, 0xFF)
        graph.replay()
        torch.cuda.synchronize()
        c.check(which)
