"""The host-memory streams (tpf_host_enc, tpf_host_dec and their _multi forms,
csrc/host_stream.cpp) against the oracle at every format, mode and chunk cut
of tests/host_inputs.py: the chunk loop, the three slots, the pinned staging
of pageable memory, the chained delta-1 start carried across chunk and shard
cuts, the rebased offsets, the global number of a corrupt block and out_cap.

Every expected byte and value comes from the oracle (host_inputs composes
each unit with its true start; tests/test_host_streams_cpu.py shows that a
wrong start, a stride of n or a dropped padding slot changes the bytes).
Every array a call may write lies inside a larger buffer of 0xA5 with 4096
bytes or more either side, pageable numpy or pinned torch memory; the margins,
and an encoder's bytes from h_off[nblocks] to out_cap, are 0xA5 afterwards
(but for tpf_host_enc_multi at a capacity of every shard's bound or more,
which turbopfor_capi.h lets use h_out up to out_cap as scratch).
The largest input is 36 units of 256 values."""
import ctypes
import re

import numpy as np
import pytest

import host_inputs as hi

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")
pytestmark = pytest.mark.gpu

FILL = 0xA5
MARGIN = 4096
CASES = [(f, n, m) for f, n in hi.PAIRS for m in hi.MODES]
IDS = [f"{hi.FMT_NAME[f]}-n{n}-{m}" for f, n, m in CASES]
MULTI_CASES = [(f, n, m) for f, n in hi.MULTI_PAIRS for m in hi.MODES]
MULTI_IDS = [f"{hi.FMT_NAME[f]}-n{n}-{m}" for f, n, m in MULTI_CASES]
PINNED_NBLOCKS = (6, 16, 36)
vp, u64 = ctypes.c_void_p, ctypes.c_uint64


@pytest.fixture(scope="module")
def L():
    lib = tpf.lib()
    lib.tpf_host_dec.argtypes = [ctypes.c_int, vp, u64, vp, u64, ctypes.c_uint, vp, vp]
    lib.tpf_host_enc.argtypes = [ctypes.c_int, vp, u64, ctypes.c_uint, ctypes.c_int, vp, u64, vp, u64, vp]
    lib.tpf_host_dec_multi.argtypes = [vp, ctypes.c_int] + lib.tpf_host_dec.argtypes
    lib.tpf_host_enc_multi.argtypes = [vp, ctypes.c_int] + lib.tpf_host_enc.argtypes
    for f in (lib.tpf_host_dec, lib.tpf_host_enc, lib.tpf_host_dec_multi, lib.tpf_host_enc_multi):
        f.restype = ctypes.c_int
    lib.tpf_enc_bound.argtypes = [ctypes.c_int, u64, ctypes.c_uint]
    lib.tpf_enc_bound.restype = u64
    lib.tpf_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture
def chunked(monkeypatch):
    """chunked(c): five units of the case's value bytes per chunk (the
    library reads the variable on every call); chunked(c, 1): one unit;
    down: TPF_HOST_DOWN."""
    def set_(c, nbytes=None, down=None):
        monkeypatch.setenv("TPF_HOST_CHUNK_BYTES", str(c.chunk_bytes if nbytes is None else nbytes))
        if down is None:
            monkeypatch.delenv("TPF_HOST_DOWN", raising=False)
        else:
            monkeypatch.setenv("TPF_HOST_DOWN", down)
    return set_


class Guard:
    """nbytes at byte `phase` past a 64-byte boundary inside a larger pageable
    (numpy) or pinned (torch) buffer filled with 0xA5, MARGIN bytes or more
    either side."""

    def __init__(self, nbytes, pinned=False, phase=0, data=None):
        total = 2 * MARGIN + 64 + nbytes
        if pinned:
            self.keep = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            self.big = self.keep.numpy()
        else:
            self.big = np.empty(total, dtype=np.uint8)
        self.big[:] = FILL
        self.s = MARGIN + (phase - (self.big.ctypes.data + MARGIN)) % 64
        self.nbytes = nbytes
        self.view = self.big[self.s: self.s + nbytes]
        self.ptr = self.big.ctypes.data + self.s
        assert self.ptr % 64 == phase
        self.data = None
        if data is not None:
            self.data = np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()
            assert len(self.data) == nbytes
            self.view[:] = self.data

    def as_(self, dtype):
        return self.view.view(dtype)

    def check(self, used=None, what=""):
        """The margins hold the fill; so does the view from byte `used` on;
        an input (data given) is unchanged."""
        assert (self.big[: self.s] == FILL).all(), f"{what}: bytes before the array were written"
        assert (self.big[self.s + self.nbytes:] == FILL).all(), f"{what}: bytes past the array were written"
        if used is not None:
            assert (self.view[used:] == FILL).all(), f"{what}: bytes past {used} were written"
        if self.data is not None:
            assert np.array_equal(self.view, self.data), f"{what}: the input array was changed"


def _starts(c, nb, first, pinned, decode):
    st = None
    if c.d1 and (decode or c.h_starts is not None):
        st = np.ascontiguousarray(c.true_starts[first: first + nb])
    return None if st is None else Guard(st.nbytes, pinned, data=st)


def enc(L, c, nb, pinned=False, cap=None, phase=0, first=0, devs=None):
    """One tpf_host_enc (devs: tpf_host_enc_multi) call on units first ..
    first + nb of the case -> (rc, h_out guard, h_off guard, checker of the
    untouched arrays)."""
    units = c.units[first: first + nb]
    gv = Guard(units.nbytes, pinned, data=units)
    if cap is None:
        cap = int(L.tpf_enc_bound(c.fmt, nb, c.n))
    go = Guard(cap, pinned, phase)
    gf = Guard((nb + 1) * 8, pinned)
    gs = _starts(c, nb, first, pinned, decode=False)
    args = (c.fmt, gv.ptr, nb, c.n, c.d1, gs.ptr if gs else None, c.start0_arg(first), go.ptr, cap, gf.ptr)
    if devs is None:
        rc = L.tpf_host_enc(*args)
    else:
        d = np.asarray(devs, dtype=np.int32)
        rc = L.tpf_host_enc_multi(d.ctypes.data, len(d), *args)

    def others(what):
        gv.check(what=what + " h_vals")
        if gs:
            gs.check(what=what + " h_starts")
    return rc, go, gf, others


def check_enc(L, c, nb, res, what, first=0, scratch=False):
    """scratch: the call may use h_out up to out_cap as scratch (tpf_host_enc_multi
    at a capacity that holds every shard's bound, turbopfor_capi.h); the margins
    past out_cap are held to the fill all the same."""
    rc, go, gf, others = res
    assert rc == 0, (what, L.tpf_last_error())
    exp_p, exp_o = c.stream(nb, first)
    np.testing.assert_array_equal(gf.as_(np.uint64), exp_o, err_msg=what + " offsets")
    total = int(exp_o[-1])
    bad = np.nonzero(go.view[:total] != exp_p)[0]
    assert not len(bad), (what, "first differing byte", int(bad[0]), "unit", int(np.searchsorted(exp_o, bad[0], "right")) - 1)
    go.check(used=None if scratch else total, what=what + " h_out")
    gf.check(what=what + " h_off")
    others(what)


def dec(L, c, nb, pinned=False, with_off=True, first=0, whole=False, devs=None, off=None, slack=0):
    """One tpf_host_dec (devs: tpf_host_dec_multi) call on the expected stream
    of units first .. first + nb at an odd byte address (whole: the case's
    whole stream as h_in and h_off + first; off: offsets to pass instead;
    slack: bytes of in_bytes past the stream) -> (rc, h_vals guard, checker)."""
    if whole:
        p, o = c.packed, c.off[first: first + nb + 1]
    else:
        p, o = c.stream(nb, first)
    if slack:
        p = np.concatenate([p, np.full(slack, 0x5A, dtype=np.uint8)])
    if off is not None:
        o = off
    gi = Guard(len(p), pinned, phase=1, data=p)
    o = np.ascontiguousarray(o, dtype=np.uint64)
    gs = _starts(c, nb, first, pinned, decode=True)
    gv = Guard(nb * c.stride * c.es, pinned)
    args = (c.fmt, gi.ptr, len(p), o.ctypes.data if with_off else None, nb, c.n, gv.ptr, gs.ptr if gs else None)
    if devs is None:
        rc = L.tpf_host_dec(*args)
    else:
        d = np.asarray(devs, dtype=np.int32)
        rc = L.tpf_host_dec_multi(d.ctypes.data, len(d), *args)

    def others(what):
        gi.check(what=what + " h_in")
        gv.check(what=what + " h_vals")
        if gs:
            gs.check(what=what + " h_starts")
    return rc, gv, others


def check_dec(L, c, nb, res, what, first=0):
    rc, gv, others = res
    assert rc == 0, (what, L.tpf_last_error())
    got = gv.as_(c.dtype).reshape(nb, c.stride)[:, : c.n]
    exp = c.units[first: first + nb, : c.n]
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert not len(bad), (what, "first differing unit", int(bad[0]))
    others(what)


@pytest.mark.parametrize("fmt,n,mode", CASES, ids=IDS)
def test_host_enc_vs_oracle(L, chunked, fmt, n, mode):
    """4.1: offsets and bytes of tpf_host_enc equal the oracle's at one, two,
    three, four and seven chunks of five units, a ragged one-unit tail and
    one-unit chunks, on pageable buffers; on pinned ones with h_out at byte
    phase 3, by SDMA and with TPF_HOST_DOWN=kernel."""
    c = hi.case(fmt, n, mode)
    chunked(c)
    for nb in hi.NBLOCKS:
        check_enc(L, c, nb, enc(L, c, nb), f"{c.id} nb={nb} pageable")
    chunked(c, 1)
    check_enc(L, c, hi.ONE_UNIT_NB, enc(L, c, hi.ONE_UNIT_NB), f"{c.id} one-unit chunks pageable")
    for down in (None, "kernel"):
        chunked(c, down=down)
        for nb in PINNED_NBLOCKS:
            check_enc(L, c, nb, enc(L, c, nb, pinned=True, phase=3), f"{c.id} nb={nb} pinned down={down}")
    chunked(c, 1, down="kernel")
    check_enc(L, c, hi.ONE_UNIT_NB, enc(L, c, hi.ONE_UNIT_NB, pinned=True, phase=3), f"{c.id} one-unit chunks pinned kernel")


@pytest.mark.parametrize("fmt,n,mode", CASES, ids=IDS)
def test_host_dec_vs_oracle(L, chunked, fmt, n, mode):
    """4.2: tpf_host_dec reads the oracle's stream at an odd byte address,
    with the expected offsets and with h_off = NULL (scanned), and returns the
    first n values of every unit; nothing outside nblocks * stride values is
    written.  A delta-1 stream is decoded with its true starts.  Pageable, and
    pinned by SDMA and with TPF_HOST_DOWN=kernel (the kernel stores through the
    mapped host pointer, at c0 * stride * es: 4-byte aligned only for p4Dec32
    at n = 127); and a sub-stream: h_in whole, h_off + 5, 11 units."""
    c = hi.case(fmt, n, mode)
    for with_off in (True, False):
        chunked(c)
        for nb in hi.NBLOCKS:
            check_dec(L, c, nb, dec(L, c, nb, with_off=with_off), f"{c.id} nb={nb} pageable off={with_off}")
        chunked(c, 1)
        check_dec(L, c, hi.ONE_UNIT_NB, dec(L, c, hi.ONE_UNIT_NB, with_off=with_off), f"{c.id} one-unit chunks off={with_off}")
        for down in (None, "kernel"):
            chunked(c, down=down)
            for nb in PINNED_NBLOCKS:
                check_dec(L, c, nb, dec(L, c, nb, pinned=True, with_off=with_off), f"{c.id} nb={nb} pinned down={down} off={with_off}")
    for pinned, down in ((False, None), (True, None), (True, "kernel")):
        chunked(c, down=down)
        check_dec(L, c, 11, dec(L, c, 11, pinned=pinned, first=5, whole=True), f"{c.id} sub-stream pinned={pinned} down={down}", first=5)


def _devs(k):
    return [i % torch.cuda.device_count() for i in range(k)]


@pytest.mark.parametrize("fmt,n,mode", MULTI_CASES, ids=MULTI_IDS)
def test_host_multi_vs_oracle(L, chunked, fmt, n, mode):
    """4.3: two and three shards (devices i % device_count), each of several
    five-unit chunks: the encoder at a roomy capacity, at exactly the summed
    bounds of the shards (both written in place: the later shards land at
    provisional offsets inside h_out and are moved down, so h_out is the
    call's scratch up to out_cap and only the bytes below h_off[nblocks] and
    the margins past out_cap are held), at exactly the stream's length and a
    little above it (through scratch: every byte from h_off[nblocks] on keeps
    the fill); the decoder with and without offsets."""
    c = hi.case(fmt, n, mode)
    chunked(c)
    for k in hi.MULTI_K:
        for nb in hi.MULTI_NBLOCKS:
            bounds = sum(int(L.tpf_enc_bound(fmt, nb * (d + 1) // k - nb * d // k, n)) for d in range(k))
            length = int(c.off[nb])
            assert length + 77 < bounds
            for pinned, cap in ((False, 2 * bounds + 999), (False, bounds), (False, length), (False, length + 77),
                                (True, bounds), (True, length)):
                what = f"{c.id} k={k} nb={nb} cap={cap} pinned={pinned}"
                check_enc(L, c, nb, enc(L, c, nb, pinned=pinned, cap=cap, phase=3 if pinned else 0, devs=_devs(k)), what,
                          scratch=cap >= bounds)
            for pinned, with_off in ((False, True), (False, False), (True, True)):
                what = f"{c.id} k={k} nb={nb} decode off={with_off} pinned={pinned}"
                check_dec(L, c, nb, dec(L, c, nb, pinned=pinned, with_off=with_off, devs=_devs(k)), what)


@pytest.mark.parametrize("fmt,n", hi.CORRUPT_PAIRS, ids=lambda v: str(v))
def test_corrupt_block_is_named_by_its_global_number(L, chunked, fmt, n):
    """4.4: 36 units in chunks of five; off[b] + 1 makes block b - 1 one byte
    too long: tpf_host_dec answers TPF_ECORRUPT and names block b - 1, in
    chunk 0, chunk 1, a reused slot and next to the ragged tail; of two bad
    blocks the lower; with every offset equal, block 0.  These are refusals of
    bad input: offsets are checked, never followed."""
    c = hi.corrupt_case(fmt, n)
    nb = hi.MAX_NB
    chunked(c)

    def run(off, what, pinned=False, devs=None, slack=0):
        rc, gv, others = dec(L, c, nb, pinned=pinned, off=off, devs=devs, slack=slack)
        msg = L.tpf_last_error().decode()
        assert rc == -4, (what, rc, msg)
        others(what)
        return msg

    for b in hi.CORRUPT_AT:
        off = c.off.copy()
        off[b] += 1
        for pinned in (False, True):
            assert f"block {b - 1} parses" in run(off, f"{c.id} b={b}", pinned), (b, pinned)
        msg = run(off, f"{c.id} b={b} multi", devs=_devs(2))
        m = re.search(r"blocks (\d+)\.\.(\d+), block numbers below are shard-relative.*block (\d+) parses", msg)
        assert m, msg
        assert int(m.group(1)) + int(m.group(3)) == b - 1 and int(m.group(1)) <= b - 1 < int(m.group(2)), msg
    off = c.off.copy()
    off[8] += 1
    off[18] += 1
    assert "block 7 parses" in run(off, f"{c.id} two bumps")
    # the last block itself, alone in the ragged tail chunk: chunk 7, block 0 of it
    off = c.off.copy()
    off[nb] += 1
    assert f"block {nb - 1} parses" in run(off, f"{c.id} last block", slack=8)
    off = np.full(nb + 1, c.off[0], dtype=np.uint64)
    assert "block 0 parses" in run(off, f"{c.id} all offsets equal")
    # the library is usable afterwards
    check_dec(L, c, nb, dec(L, c, nb), f"{c.id} after the refusals")


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("fmt,n,mode", [(2, 256, "plain"), (4, 100, "chain")], ids=["256v32-n256", "128v64-n100"])
def test_host_enc_out_cap(L, chunked, fmt, n, mode, pinned):
    """4.5: 16 units in chunks of five.  out_cap = the stream's length
    succeeds; one byte less fails at the last chunk, the first chunk's length
    + 1 at chunk 1 with later chunks queued: TPF_EINVAL "out_cap too small",
    no byte at or past h_out + out_cap written, and the next encode and a
    decode in the same process are bit-exact.  tpf_host_enc_multi at two
    shards refuses length - 1 as well."""
    c = hi.case(fmt, n, mode)
    nb = 16
    length, first_chunk = int(c.off[nb]), int(c.off[hi.CHUNK_UNITS])
    assert first_chunk + 1 < int(c.off[2 * hi.CHUNK_UNITS]) and first_chunk + 1 < length - 1
    for down in ((None, "kernel") if pinned else (None,)):
        chunked(c, down=down)
        ph = 3 if pinned else 0
        check_enc(L, c, nb, enc(L, c, nb, pinned=pinned, cap=length, phase=ph), f"{c.id} cap=length down={down}")
        for cap, devs in ((length - 1, None), (first_chunk + 1, None), (length - 1, _devs(2))):
            what = f"{c.id} cap={cap} devs={devs} down={down}"
            rc, go, gf, others = enc(L, c, nb, pinned=pinned, cap=cap, phase=ph, devs=devs)
            assert rc == -1, (what, rc, L.tpf_last_error())
            assert b"out_cap too small" in L.tpf_last_error(), (what, L.tpf_last_error())
            go.check(what=what + " h_out")
            gf.check(what=what + " h_off")
            others(what)
            check_enc(L, c, nb, enc(L, c, nb, pinned=pinned, phase=ph), what + ": the next encode")
            check_dec(L, c, nb, dec(L, c, nb, pinned=pinned), what + ": the next decode")
        check_enc(L, c, nb, enc(L, c, nb, pinned=pinned, cap=length, phase=ph, devs=_devs(2)), f"{c.id} multi cap=length down={down}")


def test_host_enc_refuses_bad_arguments_with_a_device(L):
    """The same answers as tests/test_capi_cpu.py gives without a GPU: a
    (fmt, n) the batch encoder refuses (n = 0 used to divide by zero) and null
    pointers are TPF_EINVAL, and the next call works."""
    c = hi.case(2, 256, "plain")
    vals = np.ascontiguousarray(c.units[:4])
    out = np.zeros(65536, dtype=np.uint8)
    off = np.zeros(5, dtype=np.uint64)
    devs = np.zeros(2, dtype=np.int32)
    for fmt, n in [(0, 0), (3, 0), (99, 0), (2, 0), (2, 257), (1, 129), (4, 129), (5, 100), (99, 5)]:
        assert L.tpf_host_enc(fmt, vals.ctypes.data, 4, n, 0, None, 0, out.ctypes.data, len(out), off.ctypes.data) == -1
        assert b"unsupported" in L.tpf_last_error(), (fmt, n, L.tpf_last_error())
        assert L.tpf_host_enc_multi(devs.ctypes.data, 2, fmt, vals.ctypes.data, 4, n, 0, None, 0, out.ctypes.data, len(out),
                                    off.ctypes.data) == -1
        assert b"unsupported" in L.tpf_last_error(), (fmt, n, L.tpf_last_error())
    assert L.tpf_host_enc(2, None, 4, 256, 0, None, 0, out.ctypes.data, len(out), off.ctypes.data) == -1
    assert L.tpf_host_enc(2, vals.ctypes.data, 4, 256, 0, None, 0, None, len(out), off.ctypes.data) == -1
    assert L.tpf_host_enc(2, vals.ctypes.data, 4, 256, 0, None, 0, out.ctypes.data, len(out), None) == -1
    for nd in (0, 65):
        assert L.tpf_host_enc_multi(devs.ctypes.data, nd, 2, vals.ctypes.data, 4, 256, 0, None, 0, out.ctypes.data, len(out),
                                    off.ctypes.data) == -1
    check_enc(L, c, 4, enc(L, c, 4), "after the refusals")
