"""tpf_lists_unit_offsets on the device (include/turbopfor_gpu.h): the unit
offsets of a lists stream from the lists' byte spans and the units' headers.

The streams are those of tests/lists_scan.py, whose offsets the oracle wrote;
the host scan tpf_lists_scan_offsets (tests/test_lists_scan_cpu.py holds it to
the oracle) is the definition the device is compared with wherever the stream
is not clean.  Every call writes into exactly sized, sentinel-guarded outputs,
runs on a workspace of the exact size filled with 0xFF, reads the stream at an
odd byte address behind a junk prefix, and takes list pointers that do not
start at 0.

The caps the scale test crosses: the plan and the short pass (k_scan_plan,
k_scan_short) are grid-stride kernels of at most turbopfor_amd.lists_flat_cap()
threads, one per list; the walk (k_scan_walk) gives a wave LISTS_SCAN_RUN
lists, holds LISTS_SCAN_WINDOW bytes of the stream in LDS and stores the
offsets of 64 units at a time."""
import ctypes

import numpy as np
import pytest

import lists_index as li
import lists_scale as sc
import lists_scan as ls
from lists_index import DEV, SENT, SENT64

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu

PTR0 = 1000  # the list pointers start here: only their differences count


class Run:
    """One call on `s` (lists_scan.Stream) with the anchors `lbyte`: the stream
    `shift` bytes past a 16-byte boundary, `tail` bytes after in_bytes."""

    def __init__(self, s, lbyte, shift=5, in_bytes=None, tail=None, nunits=None):
        self.s = s
        self.nunits = len(s.offs) - 1 if nunits is None else nunits
        self.nlists = len(s.ptr) - 1
        self.in_bytes = len(s.packed) if in_bytes is None else in_bytes
        self.d_in = li.dev8(torch, s.packed, shift=shift)
        if tail is not None:
            self.d_in[self.in_bytes:] = torch.from_numpy(np.resize(tail, self.d_in.numel() - self.in_bytes)).to(DEV)
        self.d_ptr = li.dev64(torch, np.asarray(s.ptr, dtype=np.uint64) + np.uint64(PTR0))
        self.d_lb = li.dev64(torch, lbyte)
        self.off = li.Guarded64(torch, self.nunits + 1)
        self.lu = li.Guarded32(torch, self.nlists + 1)
        self.err = torch.full((1,), 0x77, dtype=torch.int64, device=DEV)
        self.ws = torch.empty(max(int(tpf.lib().tpf_lists_unit_offsets_workspace_size(self.nunits, self.nlists)), 1), dtype=torch.uint8,
                              device=DEV)

    def call(self):
        self.ws.fill_(0xFF)
        tpf.lists_unit_offsets(self.d_in[:self.in_bytes], self.d_ptr, self.d_lb, nunits=self.nunits, out=self.off.view,
                               list_unit=self.lu.view, err=self.err, ws=self.ws)
        return self

    def read(self):
        """-> (offsets, unit directory, code); the guards are held here"""
        off, ok1 = self.off.read()
        lu, ok2 = self.lu.read()
        assert ok1 and ok2, "a write outside d_off[0 .. nunits] or d_list_unit[0 .. nlists]"
        return off.view(np.uint64), lu, int(self.err.item())

    def clean(self):
        off, lu, code = self.read()
        assert code == ls.CLEAN, (self.s.name, code)
        assert np.array_equal(off, np.asarray(self.s.offs, dtype=np.uint64)), self.s.name
        assert np.array_equal(lu, ls.unit_base(self.s.ptr).astype(np.uint32)), self.s.name


def host(packed, s, lbyte, nunits=None, in_bytes=None):
    nunits = len(s.offs) - 1 if nunits is None else nunits
    buf = np.ascontiguousarray(packed[:len(packed) if in_bytes is None else in_bytes])
    return tpf.lists_scan_offsets_host(buf, s.ptr, lbyte, nunits)


# ---- clean streams ----------------------------------------------------------------
@pytest.mark.parametrize("group", ["small", "families"])
def test_clean_streams(group):
    s, lbyte = ls.joined(ls.small_streams() if group == "small" else ls.family_streams(), prefix=13)
    assert int(lbyte[0]) == 13
    for shift in (5, 0):
        Run(s, lbyte, shift=shift).call().clean()
    # without the optional directory, and without d_err
    r = Run(s, lbyte)
    tpf.lists_unit_offsets(r.d_in[:r.in_bytes], r.d_ptr, r.d_lb, out=r.off.view, ws=r.ws)
    off, ok = r.off.read()
    assert ok and np.array_equal(off.view(np.uint64), s.offs)


def test_every_small_stream_alone():
    for s in ls.small_streams():
        Run(s, ls.list_byte(s), shift=3).call().clean()
    # no lists at all: d_off[0] = 0 and a clean d_err
    e = ls.Stream("none", np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    off, _, code = Run(e, np.full(1, 9, np.uint64)).call().read()
    assert code == ls.CLEAN and int(off[0]) == 0


# ---- the device against the host export on corrupted streams ---------------------------
@pytest.fixture(scope="module")
def index():
    pick = ("matrix_d1", "matrix_plain", "vbyte_blocks", "const_gaps", "empty_runs", "wide_d1")
    return ls.joined([x for x in ls.all_streams() if x.name in pick], prefix=7)


def test_single_byte_corruptions_match_the_host(index):
    """The bounds checks absorb every one of these: the device reports the
    host's code and writes the host's offsets, inside the guards."""
    s, lbyte = index
    r = Run(s, lbyte)
    r.call().clean()
    codes = set()
    for pos, new in ls.corruptions(s, 204):
        bad = s.packed.copy()
        bad[pos] = new
        want, wcode = host(bad, s, lbyte)
        r.d_in[pos] = new
        r.off.big.fill_(SENT64)
        off, lu, code = r.call().read()
        r.d_in[pos] = int(s.packed[pos])
        assert code == wcode, (pos, new, code, wcode)
        assert np.array_equal(off, want.astype(np.uint64)), (pos, new)
        assert np.array_equal(lu, ls.unit_base(s.ptr).astype(np.uint32))
        codes.add(wcode)
    assert len(codes) > 30 and ls.CLEAN in codes, sorted(codes)[:10]  # many were refused, and some change nothing the scan reads
    r.call().clean()


def test_structure_refusals_write_nothing(index):
    s, lbyte = index
    nunits, nlists = len(s.offs) - 1, len(s.ptr) - 1
    j = next(j for j in range(2, nlists) if lbyte[j] > lbyte[j - 1] > lbyte[j - 2])
    dec = lbyte.copy()
    dec[j] = lbyte[j - 1] - np.uint64(1)
    big = lbyte.copy()
    big[nlists] += np.uint64(1)
    e = next(j for j in range(nlists - 1) if s.ptr[j + 1] == s.ptr[j] and s.ptr[j + 2] > s.ptr[j + 1])
    own = lbyte.copy()
    own[e + 1] += np.uint64(1)
    pdec = s.ptr.copy()
    pdec[j] = pdec[j - 1] - np.uint64(1)
    cases = [(s, dec, nunits, nunits + j - 1), (s, big, nunits, nunits + nlists - 1), (s, own, nunits, nunits + e),
             (s._replace(ptr=pdec), lbyte, nunits, nunits + j - 1), (s, lbyte, nunits + 1, nunits + 1 + nlists),
             (s, lbyte, nunits - 1, nunits - 1 + nlists)]
    for st, lb, nu, want in cases:
        assert host(s.packed, st, lb, nu)[1] == want
        r = Run(st, lb, nunits=nu).call()
        assert int(r.err.item()) == want
        assert (r.off.big == SENT64).all() and (r.lu.big.cpu().numpy().view(np.uint32) == SENT).all()


# ---- bytes at and past in_bytes -----------------------------------------------------------
def test_bytes_past_in_bytes_change_nothing(index):
    s, lbyte = index
    for tail in (np.array([0xFF], np.uint8), np.array([0x00], np.uint8), np.random.default_rng(3).integers(0, 256, 64, dtype=np.uint8)):
        Run(s, lbyte, tail=tail).call().clean()
    # a stream cut one byte short, whatever follows: the last non-empty list's span ends past in_bytes
    last = max(j for j in range(len(s.ptr) - 1) if s.ptr[j + 1] > s.ptr[j])
    for tail in (s.packed[-1:], np.array([0xFF], np.uint8)):
        r = Run(s, lbyte, in_bytes=len(s.packed) - 1, tail=tail).call()
        assert int(r.err.item()) == len(s.offs) - 1 + last and (r.off.big == SENT64).all()
    # the last list's anchor moved in with it: its last unit is refused, every byte after in_bytes being the one it lacks
    cut = lbyte.copy()
    cut[last + 1:] -= np.uint64(1)
    want, wcode = host(s.packed, s, cut, in_bytes=len(s.packed) - 1)
    for tail in (s.packed[-1:], np.array([0x00], np.uint8)):
        off, _, code = Run(s, cut, in_bytes=len(s.packed) - 1, tail=tail).call().read()
        assert code == wcode == int(ls.unit_base(s.ptr)[last + 1]) - 1 and np.array_equal(off, want.astype(np.uint64))


# ---- past the launch caps -------------------------------------------------------------------
def test_many_lists_and_a_long_list():
    rng = np.random.default_rng(8200)
    kinds = sc.Kinds(rng)
    nlists = tpf.lists_flat_cap(DEV) + 4321  # a second trip of k_scan_plan and k_scan_short
    ix = sc.ScaleIndex(kinds, kinds.choose(rng, nlists))
    packed, offs = ix.stream(True)
    long_list = next(x for x in ls.small_streams() if x.name == "matrix_d1")
    s, lbyte = ls.joined([ls.Stream("scale", packed, offs, ix.ptr), long_list], prefix=3)
    units = np.diff(ls.unit_base(s.ptr))
    assert len(units) > tpf.lists_flat_cap(DEV) and units.max() > 2 * 64 and (units >= 2).sum() > 500
    spans = np.diff(lbyte.astype(np.int64))
    assert spans.max() > 8 * tpf.LISTS_SCAN_WINDOW  # the long list's walk reloads its window many times
    # a wave's LISTS_SCAN_RUN lists hold several lists to walk, and lists of one unit between them
    run = units[:len(units) // tpf.LISTS_SCAN_RUN * tpf.LISTS_SCAN_RUN].reshape(-1, tpf.LISTS_SCAN_RUN)
    assert ((run >= 2).sum(axis=1) >= 2).any() and (((run >= 2).sum(axis=1) >= 1) & ((run == 1).sum(axis=1) >= 1)).any()
    Run(s, lbyte).call().clean()


# ---- a stream of its own, and a graph ---------------------------------------------------------
def test_own_stream_and_graph_replay(index):
    s, lbyte = index
    r = Run(s, lbyte)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r.call()
    stream.synchronize()
    r.clean()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tpf.lists_unit_offsets(r.d_in[:r.in_bytes], r.d_ptr, r.d_lb, nunits=r.nunits, out=r.off.view, list_unit=r.lu.view, err=r.err, ws=r.ws)
    for fill in (0x00, 0xA7):
        r.ws.fill_(fill)
        r.off.big.fill_(SENT64)
        r.lu.big.fill_(SENT - (1 << 32))
        r.err.fill_(0x77)
        graph.replay()
        torch.cuda.synchronize()
        r.clean()
    # the same graph on a corrupted stream: the replay reports what a fresh call reports
    pos, new = ls.corruptions(s, 1, seed=9)[0]
    bad = s.packed.copy()
    bad[pos] = new
    want, wcode = host(bad, s, lbyte)
    r.d_in[pos] = new
    r.ws.fill_(0x5C)
    graph.replay()
    torch.cuda.synchronize()
    off, _, code = r.read()
    assert code == wcode and np.array_equal(off, want.astype(np.uint64))


# ---- end to end: open, build the skip table, decode ------------------------------------------------
def test_open_an_index_without_offsets_and_decode_it():
    rng = np.random.default_rng(8300)
    ix = li.Index([0, 1, 255, 256, 257, 700, 0, 256 * 17 + 3, 256 * 70 + 9, 5, 512], rng)  # (the decode writes at out[ptr[j]]: these pointers start at 0)
    lbyte = ix.offs[ix.base]  # what a saver keeps: lists_list_byte(offsets, list_unit)
    d_in = li.dev8(torch, ix.packed, shift=1)[:len(ix.packed)]
    d_ptr, d_lb, d_s0 = li.dev64(torch, ix.ptr), li.dev64(torch, lbyte), li.dev32(torch, ix.start0)
    assert np.array_equal(tpf.lists_list_byte(li.dev64(torch, ix.offs), li.dev32(torch, ix.base)).cpu().numpy().view(np.uint64), lbyte)
    err = torch.full((3,), 0x77, dtype=torch.int64, device=DEV)
    lu = torch.empty(ix.nlists + 1, dtype=torch.int32, device=DEV)
    off = tpf.lists_unit_offsets(d_in, d_ptr, d_lb, nunits=ix.nunits, list_unit=lu, err=err[0:1])
    table = tpf.lists_unit_last(d_in, off, d_ptr, start0=d_s0, err=err[1:2])
    out = torch.empty(len(ix.vals), dtype=torch.int32, device=DEV)
    tpf.decn256v32_lists(d_in, off, d_ptr, d1=True, start0=d_s0, out=out, err=err[2:3])
    assert err.cpu().tolist() == [ls.CLEAN] * 3
    assert np.array_equal(off.cpu().numpy().view(np.uint64), ix.offs) and np.array_equal(lu.cpu().numpy().view(np.uint32), ix.base)
    assert np.array_equal(table.cpu().numpy().view(np.uint32), ix.table)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ix.vals)
