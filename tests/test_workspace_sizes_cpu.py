"""Workspace sizes are part of the C ABI's contract with callers that size a
buffer once and reuse it: the *_workspace_size exports are pure functions of
their counts, and the values below were recorded from the library before the
launchers' workspace layouts were rewritten on one shared carver (tpf_ws.h).
CPU-only: the exports load and run without a device."""
import ctypes
import os
import subprocess

import pytest

import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("TPF_LIB") or os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
FMT = {"32": 0, "128v32": 1, "256v32": 2, "64": 3, "128v64": 4, "256v64": 5}
COUNTS = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 2**31 - 1]

# name -> the value at every count of COUNTS
ONE_COUNT = {'tpf_p4d1dec256v32_chain_workspace_size': [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 18944, 18944, 19712, 9663807744],
 'tpf_d1dec64_chain_workspace_size': [256, 1280, 1280, 1280, 1280, 1536, 1536, 1792, 37376, 37376, 38144, 19327615232],
 'tpf_p4enc256v32_workspace_size': [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 'tpf_p4nenc256v32_workspace_size': [3840, 3840, 3840, 3840, 3840, 3840, 3840, 3840, 3840, 3840, 3840, 39849728],
 'tpf_p4ndec256v32_workspace_size': [512, 512, 512, 512, 512, 512, 512, 512, 1536, 1536, 1536, 37749760]}

# tpf_enc_workspace_size(fmt, count, n) for every (fmt, n) of n in {1, 127, 128,
# 256} that the batch entry points accept
ENC = {('32', 1): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('32', 127): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('32', 128): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('32', 256): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('128v32', 1): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('128v32', 127): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('128v32', 128): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('256v32', 1): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('256v32', 127): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('256v32', 128): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('256v32', 256): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('64', 1): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('64', 127): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('64', 128): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('64', 256): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('128v64', 1): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('128v64', 127): [256, 1280, 1280, 1280, 1280, 1280, 1280, 1536, 19968, 19968, 20736, 10200809728],
 ('128v64', 128): [256, 1280, 1280, 1280, 1280, 1536, 1536, 1792, 36352, 36352, 37120, 18790744320],
 ('256v64', 256): [256, 1280, 1280, 1280, 1280, 1536, 1536, 1792, 36352, 36352, 37120, 18790744320]}

# tpf_p4ndec256v32_lists_workspace_size(nunits, nlists): row = nunits, column = nlists
LISTS = [[1280, 2048, 2048, 2048, 2048, 2304, 2816, 3328, 82944, 83456, 83968, 42953868032],
 [2560, 3328, 3328, 3328, 3328, 3584, 4096, 4608, 84224, 84736, 85248, 42953869312],
 [2560, 3328, 3328, 3328, 3328, 3584, 4096, 4608, 84224, 84736, 85248, 42953869312],
 [2560, 3328, 3328, 3328, 3328, 3584, 4096, 4608, 84224, 84736, 85248, 42953869312],
 [2560, 3328, 3328, 3328, 3328, 3584, 4096, 4608, 84224, 84736, 85248, 42953869312],
 [2560, 3328, 3328, 3328, 3328, 3584, 4096, 4608, 84224, 84736, 85248, 42953869312],
 [2560, 3328, 3328, 3328, 3328, 3584, 4096, 4608, 84224, 84736, 85248, 42953869312],
 [3072, 3840, 3840, 3840, 3840, 4096, 4608, 5120, 84736, 85248, 85760, 42953869824],
 [36352, 37120, 37120, 37120, 37120, 37376, 37888, 38400, 118016, 118528, 119040, 42953903104],
 [36352, 37120, 37120, 37120, 37120, 37376, 37888, 38400, 118016, 118528, 119040, 42953903104],
 [37376, 38144, 38144, 38144, 38144, 38400, 38912, 39424, 119040, 119552, 120064, 42953904128],
 [18253743360, 18253744128, 18253744128, 18253744128, 18253744128, 18253744384, 18253744896, 18253745408, 18253825024, 18253825536,
  18253826048, 61207610112]]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    return turbopfor_amd.declare(ctypes.CDLL(LIB))


@pytest.mark.parametrize("name", sorted(ONE_COUNT))
def test_workspace_size_of_one_count(lib, name):
    assert [int(getattr(lib, name)(c)) for c in COUNTS] == ONE_COUNT[name]


@pytest.mark.parametrize("fmt,n", sorted(ENC))
def test_enc_workspace_size(lib, fmt, n):
    assert [int(lib.tpf_enc_workspace_size(FMT[fmt], c, n)) for c in COUNTS] == ENC[(fmt, n)]


SWEEP = 70_000  # past 65,537 units: the scan over 16-unit runs has crossed one tile of 4096 run totals


def _swept(f):
    """A caller sizes one buffer for its largest batch and reuses it for every smaller one, at a 256-byte granule."""
    v = [int(f(c)) for c in range(SWEEP + 1)]
    assert all(x % 256 == 0 for x in v)
    assert all(a <= b for a, b in zip(v, v[1:]))


@pytest.mark.parametrize("name", sorted(ONE_COUNT))
def test_workspace_size_of_one_count_is_monotonic_in_256_byte_steps(lib, name):
    _swept(getattr(lib, name))


@pytest.mark.parametrize("fmt,n", sorted(ENC))
def test_enc_workspace_size_is_monotonic_in_256_byte_steps(lib, fmt, n):
    _swept(lambda c: lib.tpf_enc_workspace_size(FMT[fmt], c, n))


def test_lists_decode_workspace_size(lib):
    got = [[int(lib.tpf_p4ndec256v32_lists_workspace_size(u, l)) for l in COUNTS] for u in COUNTS]
    assert got == LISTS
