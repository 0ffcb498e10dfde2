"""GPU checks of the delete from a resident index (include/turbopfor_gpu.h
tpf_lists_remove) past the caps of its launcher (csrc/p4_lists_remove.hip), and
of its workspace contract.

The scale index is tests/lists_scale.py's: a seeded choice out of a dictionary
of kinds, each composed once by the oracle.  Every kind gets one fixed removal
pattern, and the kind that is left -- np.delete of its values -- is composed by
the oracle once too, so the expected index of ~300,000 lists is again a
concatenation, never the code under test.  The list count forces a second
launch of the run scans over the lists' 64-runs (more than 262,144 lists), lists
lie in more than one stitch tile (the plain stream holds one of more bytes than
a tile), and thousands of lists share a tile.  The workspace tests are tests/test_gpu_lists_workspace.py's:
exactly the contract size between guards, dirty, at a base of 8 (mod 16); one
byte less is refused; a captured graph is replayed on a workspace of 0xFF."""
import ctypes

import numpy as np
import pytest

import lists_index as li
import lists_remove_ref as rr
import lists_scale as sc
from guarded import Workspace
from lists_index import CLEAN, DEV, SENT, SENT64

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
NLISTS = 300000
BIG = 256 * 17 + 3


def _pattern(i, n):
    """the removal pattern of kind i of n values: None = never targeted"""
    if n == 0:
        return np.zeros(0, np.int64) if i % 2 else None  # an empty list targeted with an empty segment
    if n <= 3:
        return [None, [0], [n - 1], list(range(n))][i % 4]
    return {255: [0, 100], 256: [255], 257: [256], 513: [300, 512], BIG: [256 * 16 + 1, BIG - 1]}[n]


class ResultKinds(sc.Kinds):
    """the kinds that `kinds` become under `patterns`: the same start0, np.delete of the values"""

    def __init__(self, kinds, patterns):
        self.values = [v if p is None else np.delete(v, np.asarray(p, dtype=np.int64)) for v, p in zip(kinds.values, patterns)]
        self.lens = np.asarray([len(v) for v in self.values], dtype=np.int64)
        self.units = self.lens // 256 + (self.lens % 256 != 0)
        self.start0 = kinds.start0
        self.vpool = np.concatenate(self.values)
        self.voff = sc._starts(self.lens)[:-1]
        self.tpool = rr.table(self.values)
        self.uoff = sc._starts(self.units)[:-1]
        self._streams = {}


def build_scale():
    rng = np.random.default_rng(211)
    kinds = sc.Kinds(rng)
    patterns = [_pattern(i, int(n)) for i, n in enumerate(kinds.lens)]
    after = ResultKinds(kinds, patterns)
    kind_of = kinds.choose(rng, NLISTS, big=0.002)
    old, new = sc.ScaleIndex(kinds, kind_of, ptr0=37), sc.ScaleIndex(after, kind_of)
    targeted = np.asarray([p is not None for p in patterns])[kind_of]
    qlist = np.nonzero(targeted)[0].astype(np.uint32)
    plen = np.asarray([0 if p is None else len(p) for p in patterns], dtype=np.int64)
    ppool = np.concatenate([np.asarray(p, dtype=np.uint32) for p in patterns if p is not None and len(p)])
    poff = sc._starts(plen)[:-1]
    kq = kind_of[qlist]
    pos = np.concatenate([np.full(5, 0xDEADBEEF, np.uint32), sc.gather_segments(ppool, poff[kq], plen[kq]), np.full(3, 0xDEADBEEF, np.uint32)])
    pptr = (5 + sc._starts(plen[kq])).astype(np.uint64)
    u0 = np.asarray([0 if p is None or not len(p) else int(p[0]) // 256 for p in patterns], dtype=np.int64)
    staged = int(np.where(plen[kq] > 0, kinds.lens[kq] - 256 * u0[kq], 0).sum())
    return dict(old=old, new=new, qlist=qlist, pos=pos, pptr=pptr, staged=staged, kinds=kinds, patterns=patterns)


@pytest.fixture(scope="module")
def scale():
    return build_scale()


def _call(old, packed, offs, d1, qlist, pos, pptr, stage, ws=None, out_cap=None):
    """one call through the Python wrapper -> (the five outputs, err)"""
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = None if out_cap is None else torch.full((out_cap,), 0xA5, dtype=torch.uint8, device=DEV)
    o = tpf.lists_remove(li.dev8(torch, packed)[:len(packed)], li.dev64(torch, offs), li.dev64(torch, old.ptr), li.dev32(torch, old.base),
                         li.dev32(torch, pos), li.dev64(torch, pptr), li.dev32(torch, qlist), stage, d1=d1,
                         start0=li.dev32(torch, old.start0) if d1 else None, unit_last=li.dev32(torch, old.table) if d1 else None,
                         out=out, err=err, ws=ws)
    torch.cuda.synchronize()
    return o, int(err.item())


def _same(o, new, xpacked, xoffs, d1):
    nu = new.nunits
    assert np.array_equal(o[2].cpu().numpy().view(np.uint64), new.ptr)
    assert np.array_equal(o[3].cpu().numpy().view(np.uint32), new.base)
    assert np.array_equal(o[1].cpu().numpy()[:nu + 1].view(np.uint64), xoffs)
    assert np.array_equal(o[0].cpu().numpy()[:len(xpacked)], xpacked)
    if d1:
        assert np.array_equal(o[4].cpu().numpy()[:nu].view(np.uint32), new.table)


@pytest.mark.parametrize("d1", [True, False])
def test_scale_index(scale, d1):
    old, new = scale["old"], scale["new"]
    packed, offs = old.stream(d1)
    xpacked, xoffs = new.stream(d1)
    tile = tpf.LISTS_APPEND_TILE
    assert old.nlists > 64 * 4096 and len(scale["qlist"]) > 100000          # a second launch of the run scans over the lists
    starts = xoffs[new.base.astype(np.int64)].astype(np.int64)
    assert np.diff(starts).max() > (tile // 4 if d1 else tile)               # the plain stream: a list longer than a stitch tile
    assert ((starts[:-1] // tile != (starts[1:] - 1) // tile) & (np.diff(starts) > 2000)).sum() > 10  # lists in more than one stitch tile
    assert np.diff(np.searchsorted(xoffs[new.base.astype(np.int64)], np.arange(0, len(xpacked), tile))).max() > 1000  # many lists per tile
    assert len(xpacked) > 16 * tile and new.nunits < old.nunits and 0 < scale["staged"] < len(old.vals)
    o, err = _call(old, packed, offs, d1, scale["qlist"], scale["pos"], scale["pptr"], scale["staged"])
    assert err == CLEAN
    _same(o, new, xpacked, xoffs, d1)


# ---- the workspace contract -----------------------------------------------------------------------
class Small:
    def __init__(self, d1=True):
        rng = np.random.default_rng(17)
        lens = [300, 0, 612, 256, 90, 0, 256 * 17, 7]
        s0 = rng.integers(0, 1 << 31, size=len(lens), dtype=np.uint64).astype(np.uint32)
        self.lists = [rr.values(n, d1, s0[j], rng) for j, n in enumerate(lens)]
        self.s0 = s0
        # two sets of removals of the same sizes and the same first units (0, 1, 9, 0)
        rems = ({0: [3, 50, 299], 2: [256, 300, 611], 6: [256 * 9, 256 * 9 + 5, 256 * 17 - 1], 7: [0, 6]},
                {0: [0, 51, 250], 2: [300, 301, 400], 6: [256 * 9 + 100, 256 * 12, 256 * 16], 7: [1, 2]})
        self.cases = [rr.Case(self.lists, {j: np.asarray(p) for j, p in rem.items()}, d1, s0) for rem in rems]
        c = self.cases[0]
        assert [len(x.pos) for x in self.cases] == [len(c.pos)] * 2 and c.staged == self.cases[1].staged  # one graph serves both
        self.stage = c.targeted
        self.size = int(tpf.lib().tpf_lists_remove_workspace_size(c.nunits, c.nlists, c.nq, len(c.pos), self.stage))
        self.cap = int(tpf.lib().tpf_lists_remove_bound(len(c.packed), c.nq, self.stage))
        self.d_in, self.d_off = li.dev8(torch, c.packed), li.dev64(torch, c.offs)
        self.d_ptr, self.d_base = li.dev64(torch, c.ptr), li.dev32(torch, c.base)
        self.d_st, self.d_tab = li.dev32(torch, s0), li.dev32(torch, c.table)
        self.d_pos, self.d_pptr, self.d_ql = li.dev32(torch, c.pos), li.dev64(torch, c.pptr), li.dev32(torch, c.qlist)
        self.out = torch.empty(self.cap, dtype=torch.uint8, device=DEV)
        self.off_out = torch.empty(c.nunits + 1, dtype=torch.int64, device=DEV)
        self.lptr_out = torch.empty(c.nlists + 1, dtype=torch.int64, device=DEV)
        self.lunit_out = torch.empty(c.nlists + 1, dtype=torch.int32, device=DEV)
        self.ulast_out = torch.empty(c.nunits, dtype=torch.int32, device=DEV)
        self.err = torch.zeros(1, dtype=torch.int64, device=DEV)

    def load(self, which):
        """the removals `which`, sentinels in every output"""
        c = self.cases[which]
        self.d_pos.copy_(li.dev32(torch, c.pos))
        self.d_pptr.copy_(li.dev64(torch, c.pptr))
        self.out.fill_(0xA5)
        for t in (self.off_out, self.lptr_out):
            t.fill_(SENT64)
        for t in (self.lunit_out, self.ulast_out):
            t.fill_(SENT - (1 << 32))
        self.err.zero_()

    def call(self, ws, ws_bytes):
        c = self.cases[0]
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return tpf.lib().tpf_lists_remove(p(self.d_in), len(c.packed), p(self.d_off), c.nunits, p(self.d_ptr), p(self.d_base), c.nlists, 1,
                                          p(self.d_st), p(self.d_tab), p(self.d_pos), len(c.pos), p(self.d_pptr), p(self.d_ql), c.nq,
                                          self.stage, p(self.out), self.cap, p(self.off_out), c.nunits, p(self.lptr_out),
                                          p(self.lunit_out), p(self.ulast_out), p(ws), ws_bytes, p(self.err),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, which):
        c = self.cases[which]
        n, u = len(c.xpacked), c.xunits
        assert int(self.err.item()) == CLEAN
        out = self.out.cpu().numpy()
        assert np.array_equal(out[:n], c.xpacked) and (out[n:] == 0xA5).all()
        off = self.off_out.cpu().numpy()
        assert np.array_equal(off[:u + 1].view(np.uint64), c.xoffs) and (off[u + 1:] == SENT64).all()
        assert np.array_equal(self.lptr_out.cpu().numpy().view(np.uint64), c.xptr)
        assert np.array_equal(self.lunit_out.cpu().numpy().view(np.uint32), c.xbase)
        ul = self.ulast_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(ul[:u], c.xtable) and (ul[u:] == SENT).all()

    def untouched(self):
        assert (self.out.cpu().numpy() == 0xA5).all() and (self.off_out.cpu().numpy() == SENT64).all()
        assert (self.lptr_out.cpu().numpy() == SENT64).all() and (self.lunit_out.cpu().numpy().view(np.uint32) == SENT).all()


@pytest.fixture(scope="module")
def small():
    return Small()


def test_known_contents_exact_size_and_guards(small):
    """Exactly tpf_lists_remove_workspace_size bytes between guards, pre-filled with 0x00, 0xFF and the bytes an append
    left, and once more at base 8 (mod 16): the same outputs each time."""
    S = small
    c = S.cases[0]
    assert S.size > 0 and S.size % 8 == 0
    add = li.dev32(torch, np.arange(40, dtype=np.uint32))
    donor = torch.zeros(int(tpf.lib().tpf_lists_append_workspace_size(c.nunits, c.nlists, 40)), dtype=torch.uint8, device=DEV)
    tpf.lists_append(S.d_in[:len(c.packed)], S.d_off, S.d_ptr, S.d_base, add, li.dev64(torch, np.arange(c.nlists + 1) * 5), d1=True,
                     start0=S.d_st, unit_last=S.d_tab, ws=donor)
    torch.cuda.synchronize()
    assert bool((donor != 0).any())
    for mis, fills in ((0, (0x00, 0xFF, donor)), (8, (donor, 0xFF))):  # 8: the least alignment the header promises
        ws = Workspace(S.size, mis)
        for fill in fills:
            ws.fill(fill)
            S.load(0)
            assert S.call(ws.view, S.size) == 0, tpf.lib().tpf_last_error()
            torch.cuda.synchronize()
            S.check(0)
            assert ws.intact(), (mis, fill if isinstance(fill, int) else "donor")


def test_workspace_one_byte_short_is_refused(small):
    S = small
    ws = Workspace(S.size - 1)
    S.load(0)
    L = tpf.lib()
    assert S.call(ws.view, S.size - 1) == -1
    assert b"tpf_lists_remove" in L.tpf_last_error() and b"workspace" in L.tpf_last_error()
    torch.cuda.synchronize()
    S.untouched()
    assert ws.intact() and int(S.err.item()) == 0


def test_captured_and_replayed_on_a_dirty_workspace(small):
    """One call on a stream of its own, captured: one linear sequence, no parallel branches.  The launches depend on the
    sizes alone, so the graph serves other removals of the same sizes, on a workspace overwritten with 0xFF."""
    S = small
    ws = torch.empty(S.size, dtype=torch.uint8, device=DEV)
    S.load(0)
    ws.fill_(0x00)
    assert S.call(ws, S.size) == 0  # warm-up outside the capture (library load, first-launch setup)
    torch.cuda.synchronize()
    S.check(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert S.call(ws, S.size) == 0
    for which in (1, 0):
        S.load(which)
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        S.check(which)
