"""The census conditions of tests/test_gpu_formats64.py, established on the
oracle's bytes alone: which modes, on which base layout, the seeded inputs of
v64_inputs reach at every n, so that the GPU tests cannot pass by never
reaching a path; the padding law the device is held to; and the host-side
framing (tpf_block_size) on every block of every case.  No device."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import p4_modes
import v64_inputs
from h64_inputs import ONE, U64, _below

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
FMT = {"128v64": 4, "256v64": 5}


def _decodes(case, packed, off):
    for i in range(case.nu):
        st = int(case.starts[i]) if case.d1 else 0
        got, used = oracle_lib.decode(case.fmt, packed[int(off[i]): int(off[i + 1])].tobytes(), case.n, d1=case.d1, start=st)
        assert used == int(off[i + 1]) - int(off[i]), i
        np.testing.assert_array_equal(got, case.vals[i], err_msg=f"unit {i}")


@pytest.mark.parametrize("fmt,n", v64_inputs.V64_CASES)
@pytest.mark.parametrize("d1", [False, True])
def test_v64_census(fmt, n, d1):
    """1029 units of v64_values reach every class the encoder can produce at
    n (v64_inputs.required_modes, by base layout) in at least 10 units, bitmap
    blocks with bx <= 32 and with bx > 32 in at least 10 each, at least 10
    plain blocks on each layout for the decode-only bx = 0 rewrite, and from
    n = 63 every vbEnc64 marker length; every parse ends at the next offset;
    the oracle decodes its own stream and the rewritten one to the inputs."""
    c = v64_inputs.v64_case(fmt, n, d1)
    assert c.nu == 1029
    v64_inputs.check_census(c)
    need = v64_inputs.required_modes(n)
    if n >= 63:
        assert all(c.lens[k] >= 1 for k in range(1, 10)), sorted(c.lens.items())
    _decodes(c, c.packed, c.off)
    bp, bo, kv, kh = v64_inputs.as_bx0(fmt, c.packed, c.off, n)
    if "plain_v" in need:
        assert kv >= 10 and kh >= 10, (kv, kh)
        assert v64_inputs.census(fmt, bp, bo, n)[0]["bx0"] == kv + kh
        _decodes(c, bp, bo)
    if d1:
        flat = c.vals.ravel()
        assert (flat[1:] < flat[:-1]).any()  # the chained list wraps 2^64


def test_p4bits64_reads_only_the_widths():
    """What the enumeration below rests on: the oracle's p4Bits64 returns the
    same (b, bx) for any two non-constant blocks with the same widths."""
    L = oracle_lib.lib()
    rng = np.random.default_rng(5)
    bx = ctypes.c_uint()
    for _ in range(300):
        n = int(rng.integers(2, 129))
        w = rng.integers(0, 65, size=n)
        outs = set()
        for _ in range(3):
            v = np.array([int(v64_inputs._of_width(rng, int(x))) if x else 0 for x in w], dtype=np.uint64)
            if len(set(v.tolist())) == 1:
                break
            b = L.orc_p4bits64(oracle_lib.ptr(v, oracle_lib.u64p), n, ctypes.byref(bx))
            outs.add((b, bx.value))
        assert len(outs) <= 1, (w, outs)


def test_smallest_n_with_vbyte():
    """Over every multiset of n widths 0..64 at n = 2, 3 and 4 (2,145, 47,905
    and 814,385 of them) no block is vbyte (bx = 65 from p4Bits64).  The
    directed search -- one to three exceptions of one width, of every excess
    over bases on both layouts, and the two-tier blocks of VB_MIN_N64's
    argument (one value 8..19 bits over the base, one 62..64 bits wide) --
    finds raw vbyte first at n = VB_MIN_N64 over a vertical base and at n =
    VB_H_MIN_N64 over a horizontal one, and no compressed vbyte."""
    f = oracle_lib.lib().orc_p4bits64
    bx = ctypes.c_uint()
    pbx = ctypes.byref(bx)
    v = (ctypes.c_uint64 * 4)()
    top = [0] + [1 << (w - 1) for w in range(1, 65)]  # one value of each width
    for n, count in ((2, 2145), (3, 47905), (4, 814385)):
        seen = 0
        for ws in itertools.combinations_with_replacement(range(65), n):
            v[:n] = [top[w] for w in ws]
            if ws[0] == ws[-1] and ws[0] > 1:
                v[0] ^= 1  # same width, not constant
            f(v, n, pbx)
            assert bx.value != 65, ws
            seen += 1
        assert seen == count
    rng = np.random.default_rng(9)
    first = {}

    def note(x, n):
        blk = p4_modes.parse64(oracle_lib.encode("128v64", x), 0, n, 128)
        assert blk.mode != "vb_comp"
        if blk.mode == "vb_raw":
            first.setdefault(blk.split, n)

    for n in range(2, v64_inputs.VB_H_MIN_N64 + 1):
        for b, k, ow in itertools.product((0, 3, 20, 33, 40), (1, 2, 3), range(2, 64)):
            if b + ow > 64 or k >= n:
                continue
            x = v64_inputs._base(rng, n, b)
            for q in rng.choice(n, size=k, replace=False):
                x[q] = v64_inputs._of_width(rng, b + ow)
            note(x, n)
        for b, d, top in itertools.product((0, 1, 3, 5, 33, 36, 40), range(8, 20), (62, 63, 64)):
            if n < 3:
                continue
            x = v64_inputs._base(rng, n, b)
            q, r = rng.choice(n, size=2, replace=False)
            x[q] = v64_inputs._of_width(rng, b + d)
            x[r] = v64_inputs._of_width(rng, top)
            note(x, n)
    assert first == {"vb_raw_v": v64_inputs.VB_MIN_N64, "vb_raw_h": v64_inputs.VB_H_MIN_N64}, first


def test_smallest_n_with_compressed_vbyte():
    """A directed search: a base of width b on either layout, xn >= 4
    exceptions whose excess has exactly d bits (one-byte markers) and one
    outlier ow bits over the base.  Compressed vbyte first appears at n =
    VB_COMP_MIN_N64, on both layouts."""
    rng = np.random.default_rng(10)
    first = {}
    for n in range(5, v64_inputs.VB_COMP_MIN_N64 + 1):
        for xn, d, b, ow in itertools.product(range(4, min(n, 14)), (3, 4, 5, 6, 7), (0, 3, 33, 40), range(5, 30)):
            if xn + 1 > n:
                continue
            v = _below(rng, (n,), b)
            pos = rng.choice(n, size=xn + 1, replace=False)
            v[pos[:xn]] |= rng.integers(1 << (d - 1), min(1 << d, 150), size=xn, dtype=np.uint64) << U64(b)
            v[pos[xn]] = v64_inputs._of_width(rng, b + max(ow, d + 1))
            blk = p4_modes.parse64(oracle_lib.encode("128v64", v), 0, n, 128)
            assert n >= v64_inputs.VB_H_MIN_N64 or blk.split not in ("vb_raw_h", "vb_comp_h"), (n, xn, d, b, ow)
            if blk.mode == "vb_comp":
                first.setdefault(blk.split, n)
    assert first == {"vb_comp_v": v64_inputs.VB_COMP_MIN_N64, "vb_comp_h": v64_inputs.VB_COMP_MIN_N64}, first


def test_mixed_width_draws_find_no_earlier_vbyte():
    """The seeded mixed-width search behind VB_H_MIN_N64 and VB_COMP_MIN_N64,
    at 5,000 draws per n (v64_inputs.py quotes a longer run of the same
    draw): a base of width 0..40 and one to n - 1 exceptions whose excess has
    1..8, 9..29 or 30 and more bits.  At n = 5..8 it finds no vbyte but raw over
    a vertical base, at n = 9 raw vbyte over both layouts, and no compressed vbyte
    below n = VB_COMP_MIN_N64."""
    rng = np.random.default_rng(64)
    for n in range(v64_inputs.VB_MIN_N64, v64_inputs.VB_COMP_MIN_N64):
        found = set()
        for _ in range(5000):
            b0 = int(rng.integers(0, 41))
            ws = [b0] * n
            for q in range(int(rng.integers(1, n))):
                r = rng.random()
                d = int(rng.integers(1, 9)) if r < 0.6 else int(rng.integers(9, 30)) if r < 0.75 else int(rng.integers(30, 65))
                ws[q] = min(64, b0 + d)
            v = np.array([int(v64_inputs._of_width(rng, w)) if w else 0 for w in ws], dtype=np.uint64)
            blk = p4_modes.parse64(oracle_lib.encode("128v64", v), 0, n, 128)
            if blk.mode in ("vb_raw", "vb_comp"):
                found.add(blk.split)
        if n < v64_inputs.VB_H_MIN_N64:
            assert found <= {"vb_raw_v"}, (n, found)  # (rare there: test_smallest_n_with_vbyte finds it by direction)
        else:
            assert found == {"vb_raw_v", "vb_raw_h"}, (n, found)


@pytest.mark.parametrize("fmt,n", [c for c in v64_inputs.BLOCK_SIZE_CASES if c[1] < v64_inputs.WIDTH[c[0]]])
def test_padding_law_of_the_oracle(fmt, n):
    """What test_v64_padding_contract holds the device to.  Without delta-1
    every plain-mode block of fewer than 128 values (either layout, width 63 /
    64 included) changes with the caller's slots past n, no block of another
    mode does, and no length changes; with delta-1 nothing changes."""
    c = v64_inputs.v64_case(fmt, n, False)
    dirty = v64_inputs.padded(c.vals, fmt, fill=0xDEADBEEFDEADBEEF)
    pk, off = v64_inputs.oracle_stream(fmt, dirty, n)
    np.testing.assert_array_equal(off, c.off)
    changed = {"plain_v": 0, "plain_h": 0, "plain63": 0}
    pos = 0
    for _, bn, blk in v64_inputs.blocks_of(fmt, pk, off, n):
        same = np.array_equal(c.packed[pos: blk.end], pk[pos: blk.end])
        carries = bn < 128 and blk.mode in ("plain", "plain63")
        assert same != carries, (fmt, n, bn, blk.split, pos)
        if carries:
            changed[blk.split] += 1
            lo, hi = blk.base  # only the base payload differs
            assert np.array_equal(c.packed[pos: lo], pk[pos: lo]) and hi == blk.end
        pos = blk.end
    if min(v64_inputs.block_ns(fmt, n)) > 1:
        assert min(changed.values()) >= 10, changed
    d = v64_inputs.v64_case(fmt, n, True)
    pk1, off1 = v64_inputs.oracle_stream(fmt, v64_inputs.padded(d.vals, fmt, fill=0xDEADBEEFDEADBEEF), n, d.starts)
    np.testing.assert_array_equal(off1, d.off)
    np.testing.assert_array_equal(pk1, d.packed)


@pytest.fixture(scope="module")
def capi():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    L = ctypes.CDLL(LIB)
    L.tpf_block_size.restype = ctypes.c_uint64
    L.tpf_block_size.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint, ctypes.POINTER(ctypes.c_int)]
    return L


@pytest.mark.parametrize("fmt,n", v64_inputs.BLOCK_SIZE_CASES)
@pytest.mark.parametrize("d1", [False, True])
def test_block_size_on_every_mode(capi, fmt, n, d1):
    """tpf_block_size (framing.cpp) returns the oracle's length for every unit
    of every case -- and for every 128v64 block of the 256v64 units -- and 0
    for the unit cut by one byte; the same on the bx = 0 rewrite."""
    c = v64_inputs.v64_case(fmt, n, d1)
    streams = [(c.packed, c.off)]
    if n > 1:
        streams.append(v64_inputs.as_bx0(fmt, c.packed, c.off, n)[:2])
    for packed, off in streams:
        raw = packed.tobytes()
        for i in range(c.nu):
            enc = raw[int(off[i]): int(off[i + 1])]
            assert capi.tpf_block_size(FMT[fmt], enc, len(enc), n, None) == len(enc), (fmt, n, i)
            assert capi.tpf_block_size(FMT[fmt], enc, len(enc) - 1, n, None) == 0, (fmt, n, i)
        if fmt == "256v64":
            pos = 0
            for _, bn, blk in v64_inputs.blocks_of(fmt, packed, off, n):
                enc = raw[pos: blk.end]
                assert capi.tpf_block_size(FMT["128v64"], enc, len(enc), bn, None) == len(enc), (n, bn, pos)
                assert capi.tpf_block_size(FMT["128v64"], enc, len(enc) - 1, bn, None) == 0, (n, bn, pos)
                pos = blk.end
