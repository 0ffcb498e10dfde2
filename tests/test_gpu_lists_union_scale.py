"""GPU checks of the union with a resident index (include/turbopfor_gpu.h
tpf_lists_union) past every cap of its launcher (csrc/p4_lists_union.hip), and
of its workspace contract.

The caps, each crossed by a test below that asserts the count it means to cross:
  - flat_grid (csrc/p4_lists_host.h; turbopfor_amd.lists_flat_cap threads): the
    grid-stride kernels -- the intersection's plan and k_uo_probe over the probe
    values, k_uo_plan over the queries and the records of the virtual units up
    to the host's cap out_values / 256 + nq, k_uo_heads over the queries;
  - one scan tile of 4,096 run totals (csrc/p4_scan.h): the two run scans over
    the probe's 64-index runs take a second launch above 262,144 probe values,
    and the two run scans over the queries span several tiles above 4,096
    queries;
  - one trip of the lookup's full-block kernel k_ix_dec
    (turbopfor_amd.lists_item_cap items);
  - three steps of find_list over the virtual unit bases (64^3 queries).
k_uo_dec and k_uo_tails launch one wave per 4 virtual units and per 16 queries
of the host's cap, uncapped.

The many-lists index is tests/lists_scale.py's; the expected results are
tests/lists_union_ref.py's whole-request numpy statement of the definition
(held against np.union1d by tests/test_lists_union_cpu.py) -- never the code
under test -- and every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import lists_index as li
import lists_scale as sc
import lists_union_ref as ur
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


def _union(R, probe, pp, qlist, cap, ws=None, positions=True):
    """one call into sentinel-filled outputs of `cap` values -> dict of what they hold afterwards"""
    out, pidx, tpos, out_ptr = _s32(cap + SLACK), _s32(cap + SLACK), _s32(cap + SLACK), _s64(len(qlist) + 1)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.lists_union(R.packed, R.offs, R.ptr, R.base, R.table, li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist),
                    start0=R.start0, out=out[:cap], out_ptr=out_ptr, pidx=pidx[:cap] if positions else None,
                    tpos=tpos[:cap] if positions else None, err=err, ws=ws)
    return dict(out=_u32(out), pidx=_u32(pidx), tpos=_u32(tpos), out_ptr=out_ptr.cpu().numpy(), err=int(err.item()))


def _want(ix, probe, pp, qlist, cap):
    vals, out_ptr, pidx, tpos = ur.want_union_keys(ix, qlist, pp, probe)
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


def test_many_queries_mostly_empty(scale):
    """More queries than flat_grid has threads, than one scan tile holds and than three steps of find_list resolve; their virtual
    units exceed flat_grid's threads too; more items than one trip of k_ix_dec covers; most segments empty."""
    ix, R = scale
    flat, items = tpf.lists_flat_cap(DEV), tpf.lists_item_cap(DEV)
    rng = np.random.default_rng(107)
    nq = max(flat, 64 ** 3) + 70001
    nq += 1 if (nq - flat) % 256 == 0 else 0
    small = np.nonzero((ix.lens > 0) & (ix.lens <= 3))[0]
    qlist = small[rng.integers(0, len(small), size=nq)]
    empties = np.nonzero(ix.lens == 0)[0]
    e = rng.random(nq) < 0.05
    qlist[e] = empties[rng.integers(0, len(empties), size=int(e.sum()))]
    big = np.nonzero(ix.lens > 3)[0]
    at = rng.permutation(nq)[:200]
    qlist[at] = big[rng.integers(0, len(big), size=200)]
    # one probe value for 15% of the queries: the list's first value or the value below it; 40 values for the queries on long lists
    r = sc.rel(ix)
    has = (rng.random(nq) < 0.15) & (ix.lens[qlist] > 0)
    counts = has.astype(np.int64)
    counts[at] = 40
    segs = np.zeros(int(counts.sum()), np.uint32)
    pp = PTR0 + sc._starts(counts)
    first = ix.vals[r[qlist]].astype(np.int64)
    one = np.where(rng.random(nq) < 0.5, first, first - 1)
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
    probe = np.concatenate([np.full(PTR0, ix.vals[0], np.uint32), segs, np.full(TRAIL, ix.vals[0], np.uint32)])
    units = int(ix.units[qlist].sum())
    assert nq > flat and nq > 64 ** 3 and nq > 4096 and units > flat
    assert len(sc.item_heads(np.repeat(qlist, counts), sc.probe_units(ix, np.repeat(qlist, counts), segs))) > items
    assert (counts == 0).mean() > 0.8
    cap = int(ix.lens[qlist].sum()) + len(segs) + 7
    _compare(_union(R, probe, pp, qlist, cap), _want(ix, probe, pp, qlist, cap))


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
    segs = [w[::3], run, v[-300:]]
    qlist = np.array([other, j, j])
    probe = np.concatenate([np.full(PTR0, v[0], np.uint32)] + segs + [np.full(TRAIL, v[0], np.uint32)])
    pp = PTR0 + sc._starts([len(s) for s in segs])
    assert len(probe) > flat and len(probe) > 64 * 4096
    cap = int(ix.lens[qlist].sum()) + sum(len(s) for s in segs)
    _compare(_union(R, probe, pp, qlist, cap), _want(ix, probe, pp, qlist, cap))


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
    probe = np.concatenate([np.full(PTR0, ix.vals[0], np.uint32)] + segs + [np.full(TRAIL, ix.vals[0], np.uint32)])
    return qlist, PTR0 + sc._starts([len(s) for s in segs]), probe


@pytest.mark.parametrize("cap", [None, 14336])
def test_known_contents_exact_size_and_guards(small, cap):
    """Exactly tpf_lists_union_workspace_size bytes between guards, pre-filled with 0x00, 0xFF and the bytes an intersection
    left, and once more at base 8 (mod 16).  cap = 14,336 values: the host's cap on the virtual units is 14,336 / 256 + 8 = 64,
    so the records of the virtual units -- the workspace's last array, cleared up to the cap -- are exactly 256 bytes."""
    S = small
    rng = np.random.default_rng(19)
    qlist, pp, probe = _small_request(S, rng)
    total = len(ur.want_union_keys(S.ix, qlist, pp, probe)[0])
    cap = total + 7 if cap is None else cap
    assert total <= cap and (cap != 14336 or cap // 256 + len(qlist) == 64)
    want = _want(S.ix, probe, pp, qlist, cap)
    size = int(tpf.lib().tpf_lists_union_workspace_size(len(qlist), len(probe), cap))
    assert size > 0 and size % 256 == 0
    donor = torch.zeros(int(tpf.lib().tpf_lists_intersect_workspace_size(len(qlist), len(probe))), dtype=torch.uint8, device=DEV)
    tpf.lists_intersect(S.R.packed, S.R.offs, S.R.ptr, S.R.base, S.R.table, li.dev32(torch, probe), li.dev64(torch, pp),
                        li.dev32(torch, qlist), start0=S.R.start0, ws=donor)
    assert bool((donor != 0).any())
    for mis, fills in ((0, (0x00, 0xFF, donor)), (8, (donor,))):  # 8: the least alignment the header promises
        ws = Workspace(size, mis)
        for fill in fills:
            ws.fill(fill)
            what = (mis, fill if isinstance(fill, int) else "donor")
            _compare(_union(S.R, probe, pp, qlist, cap, ws=ws.view), want, what)
            assert ws.intact(), what


def test_workspace_one_byte_short_is_refused(small):
    S = small
    qlist, pp, probe = _small_request(S, np.random.default_rng(19))
    cap = 6000
    L = tpf.lib()
    size = int(L.tpf_lists_union_workspace_size(len(qlist), len(probe), cap))
    ws = Workspace(size - 1)
    out, out_ptr = _s32(cap), _s64(len(qlist) + 1)
    d_probe, d_pp, d_ql = li.dev32(torch, probe), li.dev64(torch, pp), li.dev32(torch, qlist)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.tpf_lists_union(p(S.R.packed), S.R.packed.numel(), p(S.R.offs), S.ix.nunits, p(S.R.ptr), p(S.R.base), S.ix.nlists,
                           p(S.R.start0), p(S.R.table), p(d_probe), len(probe), p(d_pp), p(d_ql), len(qlist), p(out), cap, p(out_ptr),
                           None, None, p(ws.view), size - 1, None, None)
    assert rc == -1 and b"workspace" in L.tpf_last_error()
    torch.cuda.synchronize()
    assert (_u32(out) == SENT).all() and (out_ptr.cpu().numpy() == SENT64).all() and ws.intact()


def test_chain_on_a_stream_sharing_one_workspace(small):
    """Two chained calls -- (A or B) or C -- on a stream of their own, one workspace, no synchronisation in between: equal to
    the same calls made apart on fresh workspaces, and to the numpy statement."""
    S = small
    ix, R = S.ix, S.R
    rng = np.random.default_rng(31)
    q1, q2 = np.array([2, 6, 0]), np.array([6, 0, 3])
    segs = []
    for j in (0, 2, 4):
        v = ix.lists[j]
        segs.append(np.unique(np.concatenate([v[::2], v[1::4] - 1])))
    probe1 = np.concatenate(segs)
    pp1 = sc._starts([len(s) for s in segs])
    v1, op1, _, _ = ur.want_union_keys(ix, q1, pp1, probe1)
    v2, op2, pidx2, tpos2 = ur.want_union_keys(ix, q2, op1, v1)
    n1, n2 = len(v1) + 5, len(v2) + 5
    key = rng.integers(0, 1 << 32, size=len(probe1), dtype=np.uint64).astype(np.uint32)
    half_a, half_b = li.dev32(torch, probe1 ^ key), li.dev32(torch, key)
    d_pp1, d_q1, d_q2 = li.dev64(torch, pp1), li.dev32(torch, q1), li.dev32(torch, q2)
    L = tpf.lib()
    ws_bytes = max(int(L.tpf_lists_union_workspace_size(3, len(probe1), n1)), int(L.tpf_lists_union_workspace_size(3, n1, n2)))

    def chain(ws1, ws2, sync):
        d_probe1 = torch.bitwise_xor(half_a, half_b)  # a device op queued on the current stream just before the first call
        err = torch.zeros(2, dtype=torch.int64, device=DEV)
        out1, ptr1 = _s32(n1), _s64(4)
        tpf.lists_union(R.packed, R.offs, R.ptr, R.base, R.table, d_probe1, d_pp1, d_q1, start0=R.start0, out=out1, out_ptr=ptr1,
                        err=err[0:1], ws=ws1)
        sync()
        out2, ptr2, pidx, tpos = _s32(n2), _s64(4), _s32(n2), _s32(n2)
        tpf.lists_union(R.packed, R.offs, R.ptr, R.base, R.table, out1, ptr1, d_q2, start0=R.start0, out=out2, out_ptr=ptr2, pidx=pidx,
                        tpos=tpos, err=err[1:2], ws=ws2)
        return err, out1, ptr1, out2, ptr2, pidx, tpos

    torch.cuda.synchronize()
    fresh = [torch.empty(ws_bytes, dtype=torch.uint8, device=DEV) for _ in range(2)]
    apart = [t.cpu().numpy() for t in chain(*fresh, sync=torch.cuda.synchronize)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        queued = chain(ws, ws, sync=lambda: None)
    stream.synchronize()  # once, at the end
    queued = [t.cpu().numpy() for t in queued]
    for a, b in zip(apart, queued):
        assert np.array_equal(a, b)
    err, out1, ptr1, out2, ptr2, pidx, tpos = queued
    assert err.tolist() == [CLEAN, CLEAN]
    assert np.array_equal(ptr1, op1) and np.array_equal(out1.view(np.uint32), _pad(v1, n1))
    assert np.array_equal(ptr2, op2) and np.array_equal(out2.view(np.uint32), _pad(v2, n2))
    assert np.array_equal(pidx.view(np.uint32), _pad(pidx2, n2)) and np.array_equal(tpos.view(np.uint32), _pad(tpos2, n2))
    for k in range(3):
        a, b = int(op2[k]), int(op2[k + 1])
        assert np.array_equal(v2[a:b], np.union1d(np.union1d(segs[k], ix.lists[q1[k]]), ix.lists[q2[k]]))
