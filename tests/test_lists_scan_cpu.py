"""CPU-only checks of the way in for a lists stream without offsets
(include/turbopfor_capi.h tpf_lists_scan_offsets, include/turbopfor_gpu.h
tpf_lists_unit_offsets): the exports and the binding exist, the device call
judges its arguments before any device call (TPF_EINVAL) and reports
TPF_ENODEV instead of falling back to the host scan, the host scan -- the
sequential definition the device call is held to -- reproduces the oracle's
offsets on every stream of tests/lists_scan.py with and without per-list
anchors, reports every code of its contract, and runs clean under
-fsanitize=address,undefined (tests/cpp/sanitize_lists_framing.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lists_scan as ls
import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
EINVAL, ENODEV = -1, -3
P = 0x1000  # a non-null pointer that is never followed: every call that takes it is refused on the host


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    return turbopfor_amd.declare(ctypes.CDLL(LIB))


def _no_device():
    return subprocess.run([sys.executable, "-c", "import torch,sys;sys.exit(0 if torch.cuda.is_available() else 1)"]).returncode != 0


def scan(lib, packed, ptr, lbyte, nunits, in_bytes=None):
    """-> (offsets written over a sentinel fill, the code or -1)"""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
    lb = None if lbyte is None else np.ascontiguousarray(lbyte, dtype=np.uint64)
    off = np.full(nunits + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    r = lib.tpf_lists_scan_offsets(packed.ctypes.data, len(packed) if in_bytes is None else in_bytes, ptr.ctypes.data, len(ptr) - 1,
                                   None if lb is None else lb.ctypes.data, off.ctypes.data, nunits)
    assert r < 0 or r == int(off[nunits])
    return off, (ls.CLEAN if r >= 0 else -r - 1)


# ---- exports and arguments ------------------------------------------------------
def test_exports_and_binding(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_lists_scan_offsets", "tpf_lists_unit_offsets", "tpf_lists_unit_offsets_workspace_size"} <= exported
    protos = turbopfor_amd.prototypes()
    assert len(protos["tpf_lists_unit_offsets"][1]) == 12 and len(protos["tpf_lists_scan_offsets"][1]) == 7
    assert protos["tpf_lists_scan_offsets"][0] is ctypes.c_int64
    for name in ("lists_unit_offsets", "lists_scan_offsets_host", "lists_list_byte"):
        assert callable(getattr(turbopfor_amd, name))
    # the binding's restatement of the walker's shape is the source's
    with open(os.path.join(ROOT, "turbopfor-cpp_amd", "csrc", "p4_lists_scan.hip")) as f:
        src = f.read()
    assert int(re.search(r"kScanRun = (\d+);", src).group(1)) == turbopfor_amd.LISTS_SCAN_RUN
    assert int(re.search(r"kScanWin = (\d+);", src).group(1)) == turbopfor_amd.LISTS_SCAN_WINDOW


STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, 0x3FFFFFFF]


def test_workspace_size_is_monotone_and_a_multiple_of_256(lib):
    f = lib.tpf_lists_unit_offsets_workspace_size
    for fixed in (0, 1, 1000, 10 ** 6):
        for a, b in zip(STEPS, STEPS[1:]):
            assert 0 < f(a, fixed) <= f(b, fixed) and 0 < f(fixed, a) <= f(fixed, b)
            assert f(a, fixed) % 256 == 0 and f(fixed, a) % 256 == 0
    assert f(10 ** 6, 10 ** 6) < 32 * 10 ** 6  # a few words per list, nothing per unit or value
    assert f(10, 1000) == f(10 ** 6, 1000)


def _call(lib, d_in=P, in_bytes=100, ptr=P, lbyte=P, nlists=5, off=P, nunits=10, lu=None, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_lists_unit_offsets_workspace_size(min(nunits, 1 << 20), min(nlists, 1 << 20))
    return lib.tpf_lists_unit_offsets(d_in, in_bytes, ptr, lbyte, nlists, off, nunits, lu, ws, ws_bytes, None, None)


@pytest.mark.parametrize("arg", ["d_in", "ptr", "lbyte", "off", "ws"])
def test_null_pointer_is_einval(lib, arg):
    assert _call(lib, **{arg: None}) == EINVAL
    assert b"tpf_lists_unit_offsets" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


def test_small_workspace_and_limits_are_einval(lib):
    need = lib.tpf_lists_unit_offsets_workspace_size(10, 5)
    assert _call(lib, ws_bytes=need - 1) == EINVAL and b"workspace" in lib.tpf_last_error()
    for kw in (dict(nunits=0x80000000), dict(nlists=0x80000000)):
        assert _call(lib, ws_bytes=2 ** 62, **kw) == EINVAL and b"0x7FFFFFFF" in lib.tpf_last_error()
    # a null d_in is refused whenever there are units, and d_off is always written
    assert _call(lib, d_in=None, nlists=0) == EINVAL and _call(lib, off=None, nlists=0, nunits=0) == EINVAL


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        pytest.skip("a HIP device is visible")
    for call in (lambda: _call(lib), lambda: _call(lib, lu=P), lambda: _call(lib, d_in=None, nunits=0),
                 lambda: _call(lib, nlists=0, nunits=0, ptr=None, lbyte=None, ws=None, ws_bytes=0, d_in=None)):
        assert call() == ENODEV
        assert b"no CPU fallback" in lib.tpf_last_error()


# ---- the host scan against the oracle ------------------------------------------------
@pytest.mark.parametrize("group", ["small", "families"])
def test_host_scan_reproduces_the_oracle(lib, group):
    streams = ls.small_streams() if group == "small" else ls.family_streams()
    units = 0
    for s in streams:
        nunits = len(s.offs) - 1
        want = np.asarray(s.offs, dtype=np.uint64)
        assert int(want[-1]) == len(s.packed)
        for lbyte in (None, ls.list_byte(s)):
            off, code = scan(lib, s.packed, s.ptr, lbyte, nunits)
            assert code == ls.CLEAN, (s.name, code)
            assert (off == want).all(), s.name
        units += nunits
    print(f"{group}: {len(streams)} streams, {units} units")
    # several streams as one index behind a junk prefix: list_byte[0] != 0 and ptr[0] != 0
    s, lbyte = ls.joined(streams, prefix=13)
    s = s._replace(ptr=s.ptr + np.uint64(1000))
    off, code = scan(lib, s.packed, s.ptr, lbyte, len(s.offs) - 1)
    assert code == ls.CLEAN and (off == s.offs).all() and int(lbyte[0]) == 13
    got, c2 = turbopfor_amd.lists_scan_offsets_host(s.packed, s.ptr, lbyte)
    assert c2 == ls.CLEAN and (got.astype(np.uint64) == s.offs).all()


def test_census_of_the_full_blocks():
    """What the fixture's full blocks hold: every mode of a full block the scan
    sizes, compressed vbyte with every marker length."""
    modes, lens = ls.full_block_census(ls.all_streams())
    print(dict(modes), dict(lens))
    missing = [m for m in ("plain", "plain32", "zero", "const", "const32", "bitmap", "bx0", "vb_raw", "vb_comp") if modes[m] < 1]
    missing += [f"marker length {k}" for k in range(1, 6) if lens[k] < 1]
    assert not missing, f"the fixture's full blocks do not reach: {missing}"


# ---- every code --------------------------------------------------------------------
@pytest.fixture(scope="module")
def index():
    s, lbyte = ls.joined([x for x in ls.small_streams() if x.name in ("matrix_d1", "vbyte_blocks", "empty_runs")], prefix=5)
    return s, lbyte, ls.unit_base(s.ptr), len(s.offs) - 1, len(s.ptr) - 1


def test_truncation(lib, index):
    s, lbyte, base, nunits, nlists = index
    last = max(j for j in range(nlists) if s.ptr[j + 1] > s.ptr[j])
    # without anchors the last unit no longer fits; with them the last non-empty list's span ends past in_bytes
    off, code = scan(lib, s.packed[5:], s.ptr, None, nunits, in_bytes=len(s.packed) - 5 - 1)
    assert code == nunits - 1 and (off[:nunits] == s.offs[:nunits] - np.uint64(5)).all()
    off, code = scan(lib, s.packed, s.ptr, lbyte, nunits, in_bytes=len(s.packed) - 1)
    assert code == nunits + last and (off == 0x5A5A5A5A5A5A5A5A).all()


def test_bad_header_and_a_moved_anchor(lib, index):
    s, lbyte, base, nunits, nlists = index
    j = next(j for j in range(1, nlists - 1) if base[j + 1] - base[j] >= 3 and base[j] > base[j - 1])
    u = int(base[j]) + 1
    bad = s.packed.copy()
    bad[int(s.offs[u])] = 0x3F  # a plain header with b = 63
    off, code = scan(lib, bad, s.ptr, lbyte, nunits)
    assert code == u and (off == ls.want_with_bad(s, lbyte, [u])).all()
    assert int(off[u + 1]) == int(lbyte[j + 1]) and (np.diff(off.astype(np.int64)) >= 0).all()
    # list_byte[j] one byte late: list j - 1's last unit does not end its span, and list j starts inside a unit
    moved = lbyte.copy()
    moved[j] += np.uint64(1)
    off, code = scan(lib, s.packed, s.ptr, moved, nunits)
    assert code == int(base[j]) - 1
    others = np.ones(nunits + 1, bool)
    others[int(base[j]): int(base[j + 1])] = False
    assert (off[others] == s.offs[others]).all() and int(off[base[j]]) == int(lbyte[j]) + 1


def test_structure_codes(lib, index):
    s, lbyte, base, nunits, nlists = index
    untouched = lambda off: (off == 0x5A5A5A5A5A5A5A5A).all()
    j = next(j for j in range(2, nlists) if lbyte[j] > lbyte[j - 1] > lbyte[j - 2])
    dec = lbyte.copy()
    dec[j] = lbyte[j - 1] - np.uint64(1)
    off, code = scan(lib, s.packed, s.ptr, dec, nunits)
    assert code == nunits + j - 1 and untouched(off)
    big = lbyte.copy()
    big[nlists] += np.uint64(1)
    off, code = scan(lib, s.packed, s.ptr, big, nunits)
    assert code == nunits + nlists - 1 and untouched(off)
    pdec = s.ptr.copy()
    pdec[j] = pdec[j - 1] - np.uint64(1)
    off, code = scan(lib, s.packed, pdec, lbyte, nunits)
    assert code == nunits + j - 1 and untouched(off)
    for k in (nunits + 1, nunits - 1):  # the unit counts do not add up
        off, code = scan(lib, s.packed, s.ptr, lbyte, k)
        assert code == k + nlists and untouched(off)
        assert scan(lib, s.packed, s.ptr, None, k)[1] == k + nlists
    # an empty list that owns a byte
    e = next(j for j in range(nlists - 1) if s.ptr[j + 1] == s.ptr[j] and s.ptr[j + 2] > s.ptr[j + 1])
    own = lbyte.copy()
    own[e + 1] += np.uint64(1)
    off, code = scan(lib, s.packed, s.ptr, own, nunits)
    assert code == nunits + e and untouched(off)
    # no lists: off[0] = 0
    off, code = scan(lib, s.packed, s.ptr[:1], lbyte[:1], 0)
    assert code == ls.CLEAN and int(off[0]) == 0


# ---- the sanitizer run -----------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("gcc") is None, reason="no host compiler")
def test_lists_framing_under_asan_ubsan(tmp_path):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    orc = tmp_path / "orc.o"
    exe = tmp_path / "san"
    subprocess.check_call(["gcc", *flags, "-std=c11", "-c", os.path.join(ROOT, "oracle", "tpf_oracle.c"), "-o", str(orc)])
    subprocess.check_call(["g++", *flags, "-std=c++20", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sanitize_lists_framing.cpp"),
                           os.path.join(ROOT, "turbopfor-cpp_amd", "csrc", "framing.cpp"), str(orc), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "40"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout
