"""GPU checks of the buffer contract of the codec entry points
(include/turbopfor_gpu.h): a call needs `*_workspace_size(...)` bytes of
workspace and nothing more, at an 8-byte-aligned base, whatever the bytes
hold; it writes its outputs and nothing around them; it reads no input byte
past in_bytes; and it is enqueued on the caller's stream with no
synchronisation of its own.

a. Every pointer argument of a call is a view of exactly its contract size
   inside a larger buffer (tests/guarded.py), 4 KiB of a fill byte on either
   side: the workspace (the size export), an encoder's d_out (the `*_bound`
   export, passed as out_cap), a decoder's values, the offsets (count + 1),
   d_err and d_total (one element).  The workspace is pre-filled with 0x00,
   with 0xFF and with the bytes another entry point left behind, and once
   more with its base at 8 (mod 16).  Outputs and d_err equal the expected
   result every time and every guard stays intact.  Every encoder route
   leaves the bytes of d_out between the stream's end and out_cap untouched,
   which is asserted too.
b. Bytes after in_bytes cannot change a decoder's result.
c. chain_decode only reads the workspace chain_sums wrote.
d. A workspace one byte too small is rejected before anything is enqueued.
e. A chain of calls on a stream of its own, sharing one workspace with no
   synchronisation in between, and the same chain captured into one graph
   and replayed on a workspace overwritten with 0xFF.

Why the unit counts: every array of a workspace is padded to 256 bytes and
every codec workspace ends in a run scan's 256 spare bytes, so an overrun of
an array by a few elements stays inside padding -- the library's own, where
it does no harm and the fill is never looked at -- unless the array's raw
size is a multiple of 256.  The counts below are the smallest at which a
layout or a run boundary changes; the arrays they leave unpadded:
   32 units   ChainWs<u64>::sums, the 64-bit chain's unit sums (32 x 8 B)
   64 units   ChainWs<u32>::sums (64 x 4 B), PlanWs<u32>::plan of the
              generic encoder and of the 256v32 encoder's plan words
              (64 x 4 B), PlanWs<u64>::plan of the enc128v64 route (512 B);
              64 is also one lane run of phase A
   1024 units RunScanWs::tot and pre over the 64 runs of 16 units: 256 B
              where they are u32 (tot and pre of the 32-bit chain, tot of
              every encoder), 512 B where they are u64 (the 64-bit chain,
              pre of the encoders' byte offsets)
   1, 16, 17, 65, 1025: one run, a full run, and one unit more than a full
              run, a lane run and a 256-byte step of `pre`
   33, 49     (64-bit chain) phase A publishes one total per 16 units of
              its 64-unit wave run
   65,537     more than kScanTile = 4096 totals of 16-unit runs, so `tile`
              has two entries
   262,145    (32-bit chain) phase A's own scan over 64-block runs crosses
              a tile.
The workspace of the n-variant entry points is a 256-byte head (and, for the
encoder, the tail's image) in front of one of the above.

Expected results are never produced by the code under test: encoded bytes
and offsets come from the oracle (tests/oracle_lib.py), decoded values are
the original numpy values, totals are numpy sums mod 2^32 or 2^64.  The
decoders are fed the oracle's stream, never an encoder's output."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as orc
from guarded import DEV, GUARD, Guarded

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
SENT8 = 0xA5
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
CLEAN = M64
WIDE = ("64", "128v64", "256v64")
START0 = {False: 0xFFFFF000, True: M64 - 12344}  # by wide: both lists wrap in their first unit
MAXU = 1025
COUNTS = [1, 16, 17, 64, 65, 1024, 1025]
COUNTS64 = [1, 16, 17, 32, 33, 49, 64, 65, 1024, 1025]
TORCH_OF = {np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64}
TPF_EINVAL = -1


def _dt(fmt):
    return np.uint64 if fmt in WIDE else np.uint32


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8:
        a = a.view(np.int64 if a.dtype == np.uint64 else np.int32)
    return torch.from_numpy(a).to(DEV)


class Stream:
    """nu units of n values of `fmt` -- plain, or (d1) one chained delta-1 list from START0 -- with the oracle's encoding.
    Gap widths 0..20 (0..40 for 64 bits) per unit, 6% exceptions, every ninth unit constant."""

    def __init__(self, fmt, n, d1, nu, seed):
        self.fmt, self.n, self.d1, self.nu = fmt, n, d1, nu
        self.dt, self.wide = _dt(fmt), fmt in WIDE
        self.width = tpf.unit_values(fmt, n)
        self.start0 = START0[self.wide]
        rng = np.random.default_rng(seed)
        bits = rng.integers(0, (40 if self.wide else 20) + 1, size=(nu, 1)).astype(np.uint64)
        g = rng.integers(0, 1 << 62, size=(nu, n), dtype=np.uint64) & ((np.uint64(1) << bits) - np.uint64(1))
        exc = rng.random((nu, n)) < 0.06
        g = np.where(exc, rng.integers(0, 1 << 62, size=(nu, n), dtype=np.uint64) >> np.uint64(12 if self.wide else 32), g)
        g[::9] = np.uint64(5)
        if d1:
            flat = np.cumsum(g.reshape(-1) + np.uint64(1), dtype=np.uint64) + np.uint64(self.start0)  # wraps mod 2^64
            self.vals = flat.astype(self.dt).reshape(nu, n)
            self.starts = np.concatenate([np.array([self.start0], dtype=self.dt), self.vals[:-1, -1]])
        else:
            self.vals, self.starts = g.astype(self.dt), None
        self.packed, self.offs = self._encode()
        assert len(self.offs) == nu + 1 and int(self.offs[-1]) == len(self.packed)

    def _encode(self):
        f, v, st = self.fmt, self.vals, self.starts
        if f == "256v32" and self.n == 256:
            return orc.enc256v32_batch(v, starts=st)
        if f == "256v64":
            return orc.enc256v64_batch(v, starts=st)
        if f == "32":
            return orc.enc32_batch(v, starts=st)
        if f == "64":
            return orc.enc64_batch(v, starts=st)
        encs = [orc.encode(f, v[i], d1=self.d1, start=int(st[i]) if self.d1 else 0) for i in range(self.nu)]
        offs = np.concatenate([[0], np.cumsum([len(e) for e in encs])]).astype(np.uint64)
        return np.frombuffer(b"".join(encs), dtype=np.uint8).copy(), offs

    def cut(self, k):
        """the first k units: a stream of its own"""
        c = object.__new__(Stream)
        c.__dict__.update(self.__dict__)
        c.nu, c.vals, c.offs, c.packed = k, self.vals[:k], self.offs[: k + 1], self.packed[: int(self.offs[k])]
        c.starts = None if self.starts is None else self.starts[:k]
        return c

    def padded(self):
        """the values as the batch entry points take them: every unit at the layout's full width, zeros after its n values"""
        v = np.zeros((self.nu, self.width), dtype=self.dt)
        v[:, : self.n] = self.vals
        return v

    def total(self):
        """sum of the list's deltas v[i] - v[i-1] (the first from start0), mod 2^32 or 2^64: what phase A totals"""
        flat = self.vals.reshape(-1)
        d = flat - np.concatenate([np.array([self.start0], dtype=self.dt), flat[:-1]])
        return np.array([d.sum(dtype=np.uint64)]).astype(self.dt)

    def shifted(self, base):
        """the list decoded from `base` instead of start0"""
        return self.vals + np.array((base - self.start0) & M64).astype(self.dt)


@functools.lru_cache(maxsize=None)
def stream(fmt, n, d1):
    return Stream(fmt, n, d1, MAXU, seed=sum(map(ord, fmt)) * 1000 + 2 * n + d1)


class Call:
    """The output buffers of one call: each a Guarded view of exactly its contract size, sentinel-filled."""

    def __init__(self):
        self.bufs = {}

    def out(self, name, count, dt):
        g = Guarded(count * np.dtype(dt).itemsize, init=SENT8)
        self.bufs[name] = (g, dt)
        return g.as_(TORCH_OF[dt])

    def results(self):
        r = {}
        for name, (g, dt) in self.bufs.items():
            got, ok = g.read(dt)
            assert ok, f"written outside {name}"
            r[name] = got
        return r


def _sent(count, dt):
    return np.full(count * np.dtype(dt).itemsize, SENT8, np.uint8).view(dt)


def _pad8(packed, cap):
    """an encoder's d_out of `cap` bytes afterwards: the stream, then the untouched sentinel"""
    return np.concatenate([packed, np.full(cap - len(packed), SENT8, np.uint8)])


def _size(name, *args):
    return int(getattr(tpf.lib(), name)(*args))


def _clean():
    return np.array([CLEAN], dtype=np.uint64)


# ---- the cases: each is (workspace size or None, call(ws) -> outputs, expected outputs) ---------------------
def case_chain32(S, two_phase):
    """tpf_p4d1dec256v32_chained, or chain_sums + chain_decode with d_total"""
    k = S.nu
    packed, offs = _dev(S.packed), _dev(S.offs)

    def call(ws):
        c = Call()
        out = c.out("out", k * 256, np.uint32)
        if two_phase:
            ch = tpf.D1Chain(packed, offs, k, ws=ws, total=c.out("total", 1, np.uint32))
            ch.sums(err=c.out("err_a", 1, np.uint64))
            ch.decode(S.start0, out=out, err=c.out("err", 1, np.uint64))
        else:
            tpf.dec256v32_chained(packed, offs, k, start0=S.start0, out=out, err=c.out("err", 1, np.uint64), ws=ws)
        return c.results()

    want = dict(out=S.vals.reshape(-1), err=_clean())
    if two_phase:
        want.update(total=S.total(), err_a=_clean())
    return _size("tpf_p4d1dec256v32_chain_workspace_size", k), call, want


def case_chain64(S, how):
    """how: "chained" (tpf_d1dec64_chained), "named" (tpf_p4d1dec{256,128}v64_chained) or "two_phase" (chain_sums + chain_decode)"""
    k = S.nu
    packed, offs = _dev(S.packed), _dev(S.offs)

    def call(ws):
        c = Call()
        out = c.out("out", k * S.width, np.uint64)
        if how == "two_phase":
            ch = tpf.D1Chain64(S.fmt, packed, offs, k, ws=ws, total=c.out("total", 1, np.uint64))
            ch.sums(err=c.out("err_a", 1, np.uint64))
            ch.decode(S.start0, out=out, err=c.out("err", 1, np.uint64))
        else:
            tpf.dec64_chained(S.fmt, packed, offs, k, start0=S.start0, out=out, err=c.out("err", 1, np.uint64), ws=ws, named=how == "named")
        return c.results()

    want = dict(out=S.vals.reshape(-1), err=_clean())
    if how == "two_phase":
        want.update(total=S.total(), err_a=_clean())
    return _size("tpf_d1dec64_chain_workspace_size", k), call, want


def case_enc256v32(S, how):
    """how: "plain" (tpf_p4enc256v32_batch), "starts" or "chained" (tpf_p4d1enc256v32_batch with d_starts / with d_starts == NULL)"""
    k = S.nu
    vals = _dev(S.vals.reshape(-1))
    starts = _dev(S.starts) if how == "starts" else None
    cap = _size("tpf_p4enc256v32_bound", k)

    def call(ws):
        c = Call()
        tpf.enc256v32(vals, d1=how != "plain", starts=starts, start0=S.start0, out=c.out("out", cap, np.uint8),
                      offs=c.out("offs", k + 1, np.uint64), ws=ws)
        return c.results()

    return _size("tpf_p4enc256v32_workspace_size", k), call, dict(out=_pad8(S.packed, cap), offs=S.offs)


def case_enc_batch(S, chained=False):
    """tpf_enc_batch; delta-1 with d_starts, or (chained) with d_starts == NULL from start0"""
    k, f = S.nu, tpf.FMT[S.fmt]
    vals = _dev(S.padded().reshape(-1))
    starts = _dev(S.starts) if S.d1 and not chained else None
    cap = _size("tpf_enc_bound", f, k, S.n)

    def call(ws):
        c = Call()
        tpf.enc_batch(S.fmt, vals, k, S.n, d1=S.d1, starts=starts, start0=S.start0, out=c.out("out", cap, np.uint8),
                      offs=c.out("offs", k + 1, np.uint64), ws=ws)
        return c.results()

    return _size("tpf_enc_workspace_size", f, k, S.n), call, dict(out=_pad8(S.packed, cap), offs=S.offs)


def case_dec_batch(S):
    """tpf_dec_batch takes no workspace: exact outputs and guards only.  A unit of an interleaved format with n below the
    layout's width occupies the full width of d_vals; its first n values are compared."""
    k = S.nu
    packed, offs = _dev(S.packed), _dev(S.offs)
    starts = _dev(S.starts) if S.d1 else None

    def call(ws):
        c = Call()
        tpf.dec_batch(S.fmt, packed, offs, k, S.n, starts=starts, err=c.out("err", 1, np.uint64), out=c.out("out", k * S.width, S.dt))
        r = c.results()
        r["out"] = r["out"].reshape(k, S.width)[:, : S.n]
        return r

    return None, call, dict(out=S.vals, err=_clean())


def _nvalues(n, d1):
    return stream("256v32", 256, d1).vals.reshape(-1)[:n]


def case_nenc(n, d1):
    v, start0 = _nvalues(n, d1), START0[False]
    packed, offs = orc.encn256v32(v, d1=d1, start0=start0)
    vals = _dev(v)
    cap = _size("tpf_p4nenc256v32_bound", n)

    def call(ws):
        c = Call()
        tpf.encn256v32(vals, d1=d1, start0=start0, out=c.out("out", cap, np.uint8), offs=c.out("offs", tpf.n_units(n) + 1, np.uint64), ws=ws)
        return c.results()

    return _size("tpf_p4nenc256v32_workspace_size", n), call, dict(out=_pad8(packed, cap), offs=offs)


def case_ndec(n, d1, with_err):
    v, start0 = _nvalues(n, d1), START0[False]
    packed, offs = orc.encn256v32(v, d1=d1, start0=start0)
    d_packed, d_offs = _dev(packed), _dev(offs)

    def call(ws):
        c = Call()
        tpf.decn256v32(d_packed, d_offs, n, d1=d1, start0=start0, out=c.out("out", n, np.uint32),
                       err=c.out("err", 1, np.uint64) if with_err else None, ws=ws)
        return c.results()

    want = dict(out=v)
    if with_err:
        want["err"] = _clean()
    return _size("tpf_p4ndec256v32_workspace_size", n), call, want


@functools.lru_cache(maxsize=None)
def _donor(chain):
    """The bytes a call of another entry point leaves in its workspace: the 256v32 encoder's, or for the 256v32 encoder and
    the n-variant encoder built on it (`chain`) the chained 256v32 decode's."""
    S = stream("256v32", 256, True)
    size, call, _ = case_chain32(S, True) if chain else case_enc256v32(S, "chained")
    ws = torch.zeros(size, dtype=torch.uint8, device=DEV)
    call(ws)
    assert bool((ws != 0).any())
    return ws


def _compare(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def _run(case, chain_donor=False, donor_only=False):
    size, call, want = case
    if size is None:
        _compare(call(None), want, "no workspace")
        return
    assert size > 0 and size % 256 == 0
    donor = _donor(chain_donor)
    plan = ((0, (donor,)),) if donor_only else ((0, (0x00, 0xFF, donor)), (8, (donor,)))  # 8: the least alignment the header promises
    for mis, fills in plan:
        ws = Guarded(size, mis)
        for fill in fills:
            ws.fill(fill)
            what = (mis, fill if isinstance(fill, int) else "donor")
            _compare(call(ws.view), want, what)
            assert ws.intact(), what


# ---- a. known contents, exact size, guards ------------------------------------------------------------------
CHAIN32 = [("tpf_p4d1dec256v32_chained", False), ("tpf_p4d1dec256v32_chain_sums+chain_decode", True)]


@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("name,two_phase", CHAIN32, ids=[c[0] for c in CHAIN32])
def test_chained_256v32(name, two_phase, k):
    _run(case_chain32(stream("256v32", 256, True).cut(k), two_phase))


CHAIN64 = [("tpf_d1dec64_chained", "chained"), ("tpf_d1dec64_chain_sums+chain_decode", "two_phase")]


@pytest.mark.parametrize("k", COUNTS64)
@pytest.mark.parametrize("fmt", ["256v64", "128v64"])
@pytest.mark.parametrize("name,how", CHAIN64, ids=[c[0] for c in CHAIN64])
def test_chained_64(name, how, fmt, k):
    _run(case_chain64(stream(fmt, tpf.unit_values(fmt, 0), True).cut(k), how))


@pytest.mark.parametrize("name,fmt", [("tpf_p4d1dec256v64_chained", "256v64"), ("tpf_p4d1dec128v64_chained", "128v64")])
def test_chained_64_named_forms(name, fmt):
    assert hasattr(tpf.lib(), name)
    _run(case_chain64(stream(fmt, tpf.unit_values(fmt, 0), True).cut(65), "named"))


ENC256 = [("tpf_p4enc256v32_batch", "plain"), ("tpf_p4d1enc256v32_batch-d_starts", "starts"), ("tpf_p4d1enc256v32_batch-chained", "chained")]


@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("name,how", ENC256, ids=[c[0] for c in ENC256])
def test_encode_256v32(name, how, k):
    _run(case_enc256v32(stream("256v32", 256, how != "plain").cut(k), how), chain_donor=True)


# one case per route of tpf_enc_workspace_size and of the dispatch in capi.cpp
ROUTES = [("hot", "256v32", 256), ("enc128v64", "128v64", 128), ("enc128v64", "256v64", 256), ("generic", "32", 127),
          ("generic", "128v32", 128), ("generic", "128v32", 100), ("generic", "256v32", 200), ("generic", "64", 127),
          ("generic", "128v64", 100)]
ROUTE_IDS = [f"{r}-{f}-n{n}" for r, f, n in ROUTES]


@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("d1", [False, True], ids=["plain", "d1"])
@pytest.mark.parametrize("route,fmt,n", ROUTES, ids=ROUTE_IDS)
def test_tpf_enc_batch(route, fmt, n, d1, k):
    _run(case_enc_batch(stream(fmt, n, d1).cut(k)), chain_donor=route == "hot")


@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("d1", [False, True], ids=["plain", "d1"])
@pytest.mark.parametrize("route,fmt,n", ROUTES, ids=ROUTE_IDS)
def test_tpf_dec_batch(route, fmt, n, d1, k):
    _run(case_dec_batch(stream(fmt, n, d1).cut(k)))


NSIZES = [200, 768, 256 * 70 + 77]  # tail only, no tail, both


@pytest.mark.parametrize("n", NSIZES)
@pytest.mark.parametrize("d1", [False, True], ids=["plain", "d1"])
def test_tpf_p4nenc256v32(d1, n):
    _run(case_nenc(n, d1), chain_donor=True)


@pytest.mark.parametrize("n", NSIZES)
@pytest.mark.parametrize("with_err", [True, False], ids=["d_err", "d_err-NULL"])
@pytest.mark.parametrize("d1", [False, True], ids=["plain", "d1"])
def test_tpf_p4ndec256v32(d1, with_err, n):
    """The head words in front of the chained decode's workspace -- the tail's start at ws, the tail's error word at
    ws + 8 -- are the part of a workspace most exposed to the 0xFF fill."""
    _run(case_ndec(n, d1, with_err))


@pytest.mark.parametrize("n", [200, 256 * 70 + 77])
@pytest.mark.parametrize("d1", [False, True], ids=["plain", "d1"])
def test_tpf_p4ndec256v32_tail_error_through_a_dirty_head(d1, n):
    """A tail whose offsets disagree with its bytes travels through the error word at ws + 8 and is merged into d_err as
    block n // 256, whatever that word held before; the full blocks before it still decode exactly."""
    v, start0 = _nvalues(n, d1), START0[False]
    packed, offs = orc.encn256v32(v, d1=d1, start0=start0)
    bad = offs.copy()
    bad[-1] += 1
    d_packed, d_offs = _dev(np.concatenate([packed, np.zeros(64, np.uint8)])), _dev(bad)
    for mis, fill in ((0, 0x00), (0, 0xFF), (8, 0xFF)):
        ws = Guarded(_size("tpf_p4ndec256v32_workspace_size", n), mis)
        ws.fill(fill)
        c = Call()
        tpf.decn256v32(d_packed, d_offs, n, d1=d1, start0=start0, out=c.out("out", n, np.uint32), err=c.out("err", 1, np.uint64), ws=ws.view)
        r = c.results()
        assert int(r["err"][0]) == n // 256 and np.array_equal(r["out"][: n // 256 * 256], v[: n // 256 * 256]), (mis, fill)
        assert ws.intact(), (mis, fill)


# ---- a, once per workspace family: past one tile of the run scan ---------------------------------------------
BIG = 65537      # 4097 runs of 16 units: two tiles of kScanTile = 4096 run totals
BIG_A = 262145   # 4097 runs of 64 blocks: phase A's own scan crosses a tile


@pytest.fixture(scope="module")
def big32():
    """One chained delta-1 list of BIG_A 256v32 blocks (a pattern of 4096 blocks repeated), built once.  Its first BIG
    blocks are a list of their own."""
    base = stream("256v32", 256, True)
    g = base.vals.reshape(-1) - np.concatenate([np.array([base.start0], np.uint32), base.vals.reshape(-1)[:-1]])
    g = np.tile(g[: 1024 * 256], BIG_A // 1024 + 1)[: BIG_A * 256]
    S = object.__new__(Stream)
    S.__dict__.update(base.__dict__)
    S.nu = BIG_A
    S.vals = (np.cumsum(g, dtype=np.uint32) + np.uint32(base.start0)).reshape(BIG_A, 256)
    S.starts = np.concatenate([np.array([base.start0], np.uint32), S.vals[:-1, -1]])
    S.packed, S.offs = orc.enc256v32_batch(S.vals, starts=S.starts)
    return S


@pytest.fixture(scope="module")
def big64():
    """One chained delta-1 list of BIG 128v64 units, the oracle called unit by unit through preallocated buffers."""
    base = stream("128v64", 128, True)
    flat = base.vals.reshape(-1)
    g = flat - np.concatenate([np.array([base.start0], np.uint64), flat[:-1]])
    g = np.tile(g[: 1024 * 128], BIG // 1024 + 1)[: BIG * 128]
    S = object.__new__(Stream)
    S.__dict__.update(base.__dict__)
    S.nu = BIG
    S.vals = (np.cumsum(g, dtype=np.uint64) + np.uint64(base.start0)).reshape(BIG, 128)
    S.starts = np.concatenate([np.array([base.start0], np.uint64), S.vals[:-1, -1]])
    L = orc.lib()
    src = np.concatenate([S.vals.reshape(-1), np.zeros(256, np.uint64)])
    out = np.zeros(BIG * 128 * 9 + 8192, dtype=np.uint8)
    offs = np.zeros(BIG + 1, dtype=np.uint64)
    p0, o0, at = src.ctypes.data, out.ctypes.data, out.ctypes.data
    for i, st in enumerate(S.starts.tolist()):
        at = L.orc_p4d1enc128v64(ctypes.cast(p0 + 1024 * i, orc.u64p), 128, ctypes.cast(at, orc.u8p), st)
        offs[i + 1] = at - o0
    assert int(offs[-1]) <= len(out) - 4096
    S.packed, S.offs = out[: int(offs[-1])].copy(), offs
    return S


def test_chained_256v32_past_one_scan_tile(big32):
    _run(case_chain32(big32.cut(BIG), True), donor_only=True)


def test_chained_256v32_past_one_tile_of_phase_a(big32):
    _run(case_chain32(big32, True), donor_only=True)


def test_encode_256v32_past_one_scan_tile(big32):
    _run(case_enc256v32(big32.cut(BIG), "chained"), chain_donor=True, donor_only=True)


def test_chained_64_past_one_scan_tile(big64):
    _run(case_chain64(big64, "two_phase"), donor_only=True)


def test_enc128v64_route_past_one_scan_tile(big64):
    _run(case_enc_batch(big64, chained=True), donor_only=True)


def test_generic_route_past_one_scan_tile():
    base = stream("32", 127, False)
    S = base.cut(MAXU)
    S.nu, S.vals = BIG, np.tile(base.vals[:1024], (BIG // 1024 + 1, 1))[:BIG]
    S.packed, S.offs = orc.enc32_batch(S.vals)
    _run(case_enc_batch(S), donor_only=True)


# ---- b. bytes after in_bytes cannot change a result ------------------------------------------------------------
def _with_slack(packed, tail, shift=0):
    """The stream `shift` bytes past a 16-byte boundary in a buffer at least GUARD bytes longer, `tail` after it (a byte, or
    None for seeded random bytes) -> the view of exactly the stream"""
    n = len(packed)
    buf = torch.empty(16 + n + GUARD + 16, dtype=torch.uint8, device=DEV)
    s = (shift - buf.data_ptr()) % 16
    if tail is None:
        buf.copy_(torch.from_numpy(np.random.default_rng(41).integers(0, 256, size=buf.numel(), dtype=np.uint8)))
    else:
        buf.fill_(tail)
    buf[s: s + n] = torch.from_numpy(packed)
    assert buf.numel() - (s + n) >= GUARD and buf[s:].data_ptr() % 16 == shift
    return buf[s: s + n]


def _slack_cases():
    k = 200
    c32, n = stream("256v32", 256, True).cut(k), 256 * 70 + 77
    plain = stream("256v32", 256, False).cut(k)
    yield "tpf_p4dec256v32_batch", plain, lambda p, o, c: tpf.dec256v32(p, o, k, out=c.out("out", k * 256, np.uint32), err=c.out("err", 1, np.uint64)), (0,)
    yield "tpf_p4d1dec256v32_chained", c32, lambda p, o, c: tpf.dec256v32_chained(
        p, o, k, start0=c32.start0, out=c.out("out", k * 256, np.uint32), err=c.out("err", 1, np.uint64)), (0, 1)
    for fmt in ("256v64", "128v64"):
        S = stream(fmt, tpf.unit_values(fmt, 0), True).cut(k)
        yield f"tpf_d1dec64_chained-{fmt}", S, lambda p, o, c, S=S: tpf.dec64_chained(
            S.fmt, p, o, k, start0=S.start0, out=c.out("out", k * S.width, np.uint64), err=c.out("err", 1, np.uint64)), (0, 1)
    for fmt in ("32", "64"):
        S = stream(fmt, 127, False).cut(k)
        yield f"tpf_dec_batch-{fmt}-n127", S, lambda p, o, c, S=S: tpf.dec_batch(
            S.fmt, p, o, k, 127, err=c.out("err", 1, np.uint64), out=c.out("out", k * 127, S.dt)), (0,)
    N = object.__new__(Stream)
    N.vals = _nvalues(n, True)
    N.packed, N.offs = orc.encn256v32(N.vals, d1=True, start0=START0[False])
    yield "tpf_p4ndec256v32", N, lambda p, o, c: tpf.decn256v32(
        p, o, n, d1=True, start0=START0[False], out=c.out("out", n, np.uint32), err=c.out("err", 1, np.uint64)), (0,)


SLACK = ["tpf_p4dec256v32_batch", "tpf_p4d1dec256v32_chained", "tpf_d1dec64_chained-256v64", "tpf_d1dec64_chained-128v64",
         "tpf_dec_batch-32-n127", "tpf_dec_batch-64-n127", "tpf_p4ndec256v32"]


@pytest.mark.parametrize("name", SLACK)
def test_bytes_after_in_bytes_do_not_matter(name):
    """The chained decodes run once more with d_in at an odd byte address."""
    cases = {c[0]: c[1:] for c in _slack_cases()}
    assert sorted(cases) == sorted(SLACK)
    S, call, shifts = cases[name]
    offs = _dev(S.offs)
    want = dict(out=S.vals.reshape(-1), err=_clean())
    for shift in shifts:
        for tail in (0x00, 0xFF, None):
            packed = _with_slack(S.packed, tail, shift)
            assert packed.numel() == len(S.packed) and packed.data_ptr() % 2 == shift
            c = Call()
            call(packed, offs, c)
            _compare(c.results(), want, (shift, tail))


# ---- c. phase B reads the workspace, never writes it -------------------------------------------------------------
@pytest.mark.parametrize("k", [65, 1025])
@pytest.mark.parametrize("fmt", ["256v32", "256v64", "128v64"])
def test_chain_decode_only_reads_the_workspace(fmt, k):
    """Shards call chain_decode after an exchange, each with the base the exchange gave it: two bases against one phase A."""
    S = stream(fmt, tpf.unit_values(fmt, 0), True).cut(k)
    packed, offs = _dev(S.packed), _dev(S.offs)
    wide = fmt in WIDE
    ws = Guarded(_size("tpf_d1dec64_chain_workspace_size" if wide else "tpf_p4d1dec256v32_chain_workspace_size", k))
    ws.fill(0xFF)
    ch = tpf.D1Chain64(fmt, packed, offs, k, ws=ws.view) if wide else tpf.D1Chain(packed, offs, k, ws=ws.view)
    assert np.array_equal(ch.sums().cpu().numpy().view(S.dt), S.total())
    snap, ok = ws.read()
    assert ok
    for base in (S.start0, 0x0123456789ABCDEF & (M64 if wide else M32)):
        c = Call()
        ch.decode(base, out=c.out("out", k * S.width, S.dt), err=c.out("err", 1, np.uint64))
        _compare(c.results(), dict(out=S.shifted(base).reshape(-1), err=_clean()), base)
        after, ok = ws.read()
        assert ok and np.array_equal(after, snap), base


# ---- d. a workspace one byte too small is rejected before anything is enqueued -----------------------------------
def _too_small_cases():
    """name -> (size export, call(L, ws pointer, ws_bytes, c, stream) -> return code); every output comes from `c`"""
    k, n = 65, 256 * 70 + 77
    c32, c64 = stream("256v32", 256, True).cut(k), stream("256v64", 256, True).cut(k)
    p32, o32, p64, o64 = _dev(c32.packed), _dev(c32.offs), _dev(c64.packed), _dev(c64.offs)
    v32 = _dev(c32.vals.reshape(-1))
    f64 = tpf.FMT["256v64"]
    ptr = lambda t: t.data_ptr()
    out32 = lambda c: ptr(c.out("out", k * 256, np.uint32))
    out64 = lambda c: ptr(c.out("out", k * 256, np.uint64))
    err = lambda c: ptr(c.out("err", 1, np.uint64))
    cap = _size("tpf_p4enc256v32_bound", k)
    size32, size64 = _size("tpf_p4d1dec256v32_chain_workspace_size", k), _size("tpf_d1dec64_chain_workspace_size", k)
    yield "tpf_p4d1dec256v32_chain_sums", size32, lambda L, w, b, c, s: L.tpf_p4d1dec256v32_chain_sums(
        ptr(p32), p32.numel(), ptr(o32), k, w, b, ptr(c.out("total", 1, np.uint32)), err(c), s)
    yield "tpf_p4d1dec256v32_chained", size32, lambda L, w, b, c, s: L.tpf_p4d1dec256v32_chained(
        ptr(p32), p32.numel(), ptr(o32), k, out32(c), c32.start0, w, b, err(c), s)
    yield "tpf_d1dec64_chain_sums", size64, lambda L, w, b, c, s: L.tpf_d1dec64_chain_sums(
        f64, ptr(p64), p64.numel(), ptr(o64), k, w, b, ptr(c.out("total", 1, np.uint64)), err(c), s)
    yield "tpf_d1dec64_chained", size64, lambda L, w, b, c, s: L.tpf_d1dec64_chained(
        f64, ptr(p64), p64.numel(), ptr(o64), k, out64(c), c64.start0, w, b, err(c), s)
    yield "tpf_p4enc256v32_batch", _size("tpf_p4enc256v32_workspace_size", k), lambda L, w, b, c, s: L.tpf_p4enc256v32_batch(
        ptr(v32), k, ptr(c.out("out", cap, np.uint8)), cap, ptr(c.out("offs", k + 1, np.uint64)), w, b, s)
    yield "tpf_p4d1enc256v32_batch", _size("tpf_p4enc256v32_workspace_size", k), lambda L, w, b, c, s: L.tpf_p4d1enc256v32_batch(
        ptr(v32), k, None, c32.start0, ptr(c.out("out", cap, np.uint8)), cap, ptr(c.out("offs", k + 1, np.uint64)), w, b, s)
    for route, fmt, nn in (ROUTES[0], ROUTES[2], ROUTES[3]):
        S = stream(fmt, nn, False).cut(k)
        f, vals, bound = tpf.FMT[fmt], _dev(S.padded().reshape(-1)), _size("tpf_enc_bound", tpf.FMT[fmt], k, nn)
        yield f"tpf_enc_batch-{route}", _size("tpf_enc_workspace_size", f, k, nn), lambda L, w, b, c, s, f=f, vals=vals, bound=bound, nn=nn: \
            L.tpf_enc_batch(f, ptr(vals), k, nn, 0, None, 0, ptr(c.out("out", bound, np.uint8)), bound, ptr(c.out("offs", k + 1, np.uint64)), w, b, s)
    nv = _dev(_nvalues(n, True))
    ncap = _size("tpf_p4nenc256v32_bound", n)
    yield "tpf_p4nenc256v32", _size("tpf_p4nenc256v32_workspace_size", n), lambda L, w, b, c, s: L.tpf_p4nenc256v32(
        ptr(nv), n, 1, START0[False], ptr(c.out("out", ncap, np.uint8)), ncap, ptr(c.out("offs", tpf.n_units(n) + 1, np.uint64)), w, b, s)
    npk, nof = orc.encn256v32(_nvalues(n, True), d1=True, start0=START0[False])
    dpk, dof = _dev(npk), _dev(nof)
    yield "tpf_p4ndec256v32", _size("tpf_p4ndec256v32_workspace_size", n), lambda L, w, b, c, s: L.tpf_p4ndec256v32(
        ptr(dpk), dpk.numel(), ptr(dof), n, 1, START0[False], ptr(c.out("out", n, np.uint32)), w, b, err(c), s)


TOO_SMALL = ["tpf_p4d1dec256v32_chain_sums", "tpf_p4d1dec256v32_chained", "tpf_d1dec64_chain_sums", "tpf_d1dec64_chained",
             "tpf_p4enc256v32_batch", "tpf_p4d1enc256v32_batch", "tpf_enc_batch-hot", "tpf_enc_batch-enc128v64", "tpf_enc_batch-generic",
             "tpf_p4nenc256v32", "tpf_p4ndec256v32"]


@pytest.mark.parametrize("name", TOO_SMALL)
def test_workspace_one_byte_too_small_is_rejected(name):
    cases = {c[0]: c[1:] for c in _too_small_cases()}
    assert sorted(cases) == sorted(TOO_SMALL)
    size, call = cases[name]
    L = tpf.lib()
    ws = Guarded(size, init=0x5C)
    c = Call()
    rc = call(L, ws.view.data_ptr(), size - 1, c, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == TPF_EINVAL and b"workspace" in L.tpf_last_error(), (rc, L.tpf_last_error())
    torch.cuda.synchronize()
    for key, got in c.results().items():  # nothing was enqueued: not even the initialisation of d_err
        assert (got.view(np.uint8) == SENT8).all(), key
    got, ok = ws.read()
    assert ok and (got == 0x5C).all()


# ---- e. a stream of its own and a captured graph, one workspace, no synchronisation between the calls -------------
class Pipeline:
    """tpf_p4d1enc256v32_batch (chained) -> tpf_p4d1dec256v32_chained -> tpf_p4nenc256v32 (D1) -> tpf_p4ndec256v32 (D1), each
    on an input of its own that a device op produces just before the call (the xor of two halves), all four sharing one
    workspace of the largest size needed."""
    NB, N, ROUNDS = 70, 256 * 70 + 77, 4

    def __init__(self):
        nb, n, L = self.NB, self.N, tpf.lib()
        self.start0 = START0[False]
        self.sets = [self._inputs(r) for r in range(self.ROUNDS)]
        self.lenb = max(len(s["b"].packed) for s in self.sets)
        self.lend = max(len(s["d"][0]) for s in self.sets)
        u8 = lambda m: torch.zeros(m, dtype=torch.uint8, device=DEV)
        i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=DEV)
        i64 = lambda m: torch.zeros(m, dtype=torch.int64, device=DEV)
        # the two halves of each input and the buffer their xor lands in; the decoders also take their offsets
        self.half = dict(a=(i32(nb * 256), i32(nb * 256)), b=(u8(self.lenb), u8(self.lenb)), c=(i32(n), i32(n)), d=(u8(self.lend), u8(self.lend)))
        self.inp = dict(a=i32(nb * 256), b=u8(self.lenb), c=i32(n), d=u8(self.lend))
        self.off_b, self.off_d = i64(nb + 1), i64(tpf.n_units(n) + 1)
        self.cap_a, self.cap_c = _size("tpf_p4enc256v32_bound", nb), _size("tpf_p4nenc256v32_bound", n)
        self.out = dict(a=u8(self.cap_a), offs_a=i64(nb + 1), b=i32(nb * 256), c=u8(self.cap_c), offs_c=i64(tpf.n_units(n) + 1), d=i32(n))
        self.err = i64(2)
        self.ws = u8(max(int(L.tpf_p4enc256v32_workspace_size(nb)), int(L.tpf_p4d1dec256v32_chain_workspace_size(nb)),
                         int(L.tpf_p4nenc256v32_workspace_size(n)), int(L.tpf_p4ndec256v32_workspace_size(n))))

    def _inputs(self, r):
        a, b = Stream("256v32", 256, True, self.NB, seed=900 + r), Stream("256v32", 256, True, self.NB, seed=910 + r)
        c = Stream("256v32", 256, True, self.NB + 1, seed=920 + r).vals.reshape(-1)[: self.N]
        dv = Stream("256v32", 256, True, self.NB + 1, seed=930 + r).vals.reshape(-1)[: self.N]
        return dict(a=a, b=b, c=(c,) + orc.encn256v32(c, d1=True, start0=self.start0),
                    d=orc.encn256v32(dv, d1=True, start0=self.start0) + (dv,))

    def load(self, r, ws_fill):
        """round r's inputs as xor halves, sentinel outputs, the workspace overwritten"""
        s, rng = self.sets[r], np.random.default_rng(50 + r)
        raw = dict(a=s["a"].vals.reshape(-1).view(np.uint8), b=s["b"].packed, c=s["c"][0].view(np.uint8), d=s["d"][0])
        for key, (h0, h1) in self.half.items():
            full = np.zeros(h0.numel() * h0.element_size(), dtype=np.uint8)
            full[: len(raw[key])] = raw[key]
            mask = rng.integers(0, 256, size=len(full), dtype=np.uint8)
            h0.view(torch.uint8).copy_(torch.from_numpy(full ^ mask))
            h1.view(torch.uint8).copy_(torch.from_numpy(mask))
        self.off_b.copy_(_dev(s["b"].offs))
        self.off_d.copy_(_dev(s["d"][1]))
        for t in self.out.values():
            t.view(torch.uint8).fill_(SENT8)
        self.err.zero_()
        self.ws.fill_(ws_fill)

    def seq(self):
        """the four calls on the current stream, nothing in between but the device op that produces the next input"""
        nb, n, o = self.NB, self.N, self.out
        for key in "abcd":
            if key == "a":
                torch.bitwise_xor(*self.half["a"], out=self.inp["a"])
                tpf.enc256v32(self.inp["a"], d1=True, start0=self.start0, out=o["a"], offs=o["offs_a"], ws=self.ws)
            elif key == "b":
                torch.bitwise_xor(*self.half["b"], out=self.inp["b"])
                tpf.dec256v32_chained(self.inp["b"], self.off_b, nb, start0=self.start0, out=o["b"], err=self.err[0:1], ws=self.ws)
            elif key == "c":
                torch.bitwise_xor(*self.half["c"], out=self.inp["c"])
                tpf.encn256v32(self.inp["c"], d1=True, start0=self.start0, out=o["c"], offs=o["offs_c"], ws=self.ws)
            else:
                torch.bitwise_xor(*self.half["d"], out=self.inp["d"])
                tpf.decn256v32(self.inp["d"], self.off_d, n, d1=True, start0=self.start0, out=o["d"], err=self.err[1:2], ws=self.ws)

    def check(self, r):
        s = self.sets[r]
        got = {k: t.cpu().numpy() for k, t in self.out.items()}
        assert self.err.cpu().numpy().tolist() == [-1, -1], r
        assert np.array_equal(got["offs_a"].view(np.uint64), s["a"].offs) and np.array_equal(got["a"], _pad8(s["a"].packed, self.cap_a)), r
        assert np.array_equal(got["b"].view(np.uint32), s["b"].vals.reshape(-1)), r
        assert np.array_equal(got["offs_c"].view(np.uint64), s["c"][2]) and np.array_equal(got["c"], _pad8(s["c"][1], self.cap_c)), r
        assert np.array_equal(got["d"].view(np.uint32), s["d"][2]), r


@pytest.fixture(scope="module")
def pipeline():
    return Pipeline()


def test_chain_on_a_stream_of_its_own(pipeline):
    p = pipeline
    p.load(0, 0x00)
    torch.cuda.synchronize()
    stream_ = torch.cuda.Stream()
    with torch.cuda.stream(stream_):
        p.seq()
    stream_.synchronize()  # once, at the end
    p.check(0)


def test_chain_captured_and_replayed_on_a_dirty_workspace(pipeline):
    """One linear sequence on a single stream, no parallel branches, as tests/test_gpu_edges.py captures the plain calls."""
    p = pipeline
    p.load(0, 0x00)
    p.seq()  # warm-up outside the capture (library load, first-launch setup)
    torch.cuda.synchronize()
    p.check(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p.seq()
    for r in (1, 2, 3):
        p.load(r, 0xFF)
        graph.replay()
        torch.cuda.synchronize()
        p.check(r)
