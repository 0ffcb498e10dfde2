"""CPU-only checks of the host surface of the union with a resident index
(include/turbopfor_gpu.h tpf_lists_union): the symbols are exported, the
workspace-size function is a pure host function, the arguments are judged
before any device call (TPF_EINVAL), the entry point reports TPF_ENODEV instead
of falling back to a CPU codec -- and the numpy restatement of the definition
the GPU tests compare against (tests/lists_union_ref.py) is the sorted set
union."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from lists_index import Index
import lists_ref as ref
import lists_union_ref as ur
import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
EINVAL, ENODEV = -1, -3
P = 0x1000  # a non-null pointer that is never followed: every call below is refused on the host
STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, 0x3FFFFFFF]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    L = turbopfor_amd.declare(ctypes.CDLL(LIB))
    assert hasattr(L, "tpf_lists_union"), "the library does not export tpf_lists_union"
    return L


def _no_device():
    return subprocess.run([sys.executable, "-c", "import torch,sys;sys.exit(0 if torch.cuda.is_available() else 1)"]).returncode != 0


def test_symbols_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_lists_union", "tpf_lists_union_workspace_size"} <= exported
    with open(os.path.join(ROOT, "turbopfor-cpp_amd", "python", "turbopfor_amd.py")) as f:
        assert "def lists_union(" in f.read()
    with open(os.path.join(ROOT, "include", "turbopfor_gpu.h")) as f:
        assert "#define TPF_LISTS_NONE 0xFFFFFFFFu" in f.read()


def test_workspace_size_is_a_pure_host_function(lib):
    f = lib.tpf_lists_union_workspace_size
    for fixed in (0, 1, 1000, 10 ** 6):
        for a, b in zip(STEPS, STEPS[1:]):
            assert 0 < f(a, fixed, fixed) <= f(b, fixed, fixed), ("nq", a, b, fixed)
            assert 0 < f(fixed, a, fixed) <= f(fixed, b, fixed), ("probe_values", a, b, fixed)
            assert 0 < f(fixed, fixed, a) <= f(fixed, fixed, b), ("out_values", a, b, fixed)
    assert f(1000, 10 ** 6, 10 ** 7) == f(1000, 10 ** 6, 10 ** 7)  # no state


def test_workspace_is_linear(lib):
    """O(nq + probe_values + out_values / 256) words: nothing sized by the index or by the values of the lists."""
    f = lib.tpf_lists_union_workspace_size
    for nq, pv, ov in [(10 ** 6, 10 ** 6, 10 ** 9), (1, 0, 0), (10, 10 ** 7, 10 ** 6), (3 * 10 ** 6, 5, 10 ** 10), (1, 1, 2 ** 38)]:
        assert f(nq, pv, ov) < 64 * (nq + pv + ov // 256) + 65536, (nq, pv, ov)
    assert f(10, 10 ** 6, 1000) < f(10, 10 ** 7, 1000)
    assert f(10, 1000, 10 ** 8) < f(10, 1000, 10 ** 9)


def _call(lib, d_in=P, d_off=P, nunits=10, ptr=P, lu=P, nlists=5, ul=P, probe=P, probe_values=100, probe_ptr=P, qlist=P, nq=3, out=P,
          out_values=1000, out_ptr=P, pidx=None, tpos=None, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_lists_union_workspace_size(min(nq, 1 << 20), min(probe_values, 1 << 20), min(out_values, 1 << 30))
    return lib.tpf_lists_union(d_in, 100, d_off, nunits, ptr, lu, nlists, None, ul, probe, probe_values, probe_ptr, qlist, nq, out,
                               out_values, out_ptr, pidx, tpos, ws, ws_bytes, None, None)


@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "lu", "ul", "probe_ptr", "qlist", "out_ptr", "ws", "probe", "out"])
def test_null_pointer_is_einval(lib, arg):
    assert _call(lib, **{arg: None}) == EINVAL
    assert b"tpf_lists_union" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


def test_null_probe_and_out_are_allowed_when_empty(lib):
    # with nothing to read or write the two pointers may be null: the call gets past them to the workspace check
    assert _call(lib, probe=None, probe_values=0, out=None, out_values=0, ws_bytes=0) == EINVAL
    assert b"tpf_lists_union" in lib.tpf_last_error() and b"workspace" in lib.tpf_last_error()


def test_small_workspace_is_einval(lib):
    need = lib.tpf_lists_union_workspace_size(3, 100, 1000)
    assert _call(lib, ws_bytes=need - 1) == EINVAL
    assert b"tpf_lists_union" in lib.tpf_last_error() and b"workspace" in lib.tpf_last_error()


@pytest.mark.parametrize("kw", [dict(nlists=0x80000000), dict(nunits=0x80000000), dict(nq=0x80000000), dict(probe_values=0x80000000),
                                dict(out_values=256 * 0x7FFFFFFD), dict(out_values=256 * 0x7FFFFFFF, nq=1)])
def test_limits_are_einval(lib, kw):
    assert _call(lib, ws_bytes=2 ** 62, **kw) == EINVAL  # out_values / 256 + nq: 0x7FFFFFFD + 3 and 0x7FFFFFFF + 1
    assert b"tpf_lists_union" in lib.tpf_last_error() and b"0x7FFFFFFF" in lib.tpf_last_error()


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        pytest.skip("a HIP device is visible")
    for call in (lambda: _call(lib), lambda: _call(lib, pidx=P, tpos=P),
                 lambda: _call(lib, nq=0, qlist=None, probe_ptr=None, probe=None, probe_values=0, out=None, out_values=0, ws=None,
                               ws_bytes=0)):
        assert call() == ENODEV
        assert b"no CPU fallback" in lib.tpf_last_error()


# ---- the reference of the GPU tests is the set union ---------------------------------------
@pytest.fixture(scope="module")
def matrix():
    rng = np.random.default_rng(17)
    lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
    ix = Index(lens, rng, ptr0=37, start_bits=31)
    assert ix.ascends()
    return ix


def _hold(ix, queries, ptr0):
    vals, out_ptr, pidx, tpos = ur.want_union(ix, queries, ptr0)
    assert out_ptr[0] == 0 and len(vals) == out_ptr[-1] == len(pidx) == len(tpos)
    assert (((pidx != ur.NONE) | (tpos != ur.NONE))).all()  # every value comes from the probe, the list or both
    probe = np.concatenate([np.zeros(ptr0, np.uint32)] + [np.asarray(pv, np.uint32) for _, pv in queries])
    at = ptr0
    for k, (j, pv) in enumerate(queries):
        pv = np.asarray(pv, np.uint32)
        a, b = int(out_ptr[k]), int(out_ptr[k + 1])
        lst = ix.lists[j]
        assert np.array_equal(vals[a:b], np.union1d(lst, pv)), (k, j)
        both = (pidx[a:b] != ur.NONE) & (tpos[a:b] != ur.NONE)
        assert np.array_equal(vals[a:b][both], pv[np.isin(pv, lst)])  # both set exactly at the common values
        fp, fl = pidx[a:b] != ur.NONE, tpos[a:b] != ur.NONE
        assert np.array_equal(probe[pidx[a:b][fp]], vals[a:b][fp]) and np.array_equal(pidx[a:b][fp], at + np.arange(len(pv)))
        assert np.array_equal(lst[tpos[a:b][fl]], vals[a:b][fl]) and np.array_equal(tpos[a:b][fl], np.arange(len(lst)))
        at += len(pv)


def test_reference_is_the_set_union_at_the_edges(matrix):
    ix = matrix
    queries = [(j, ur.edge_probe(ix, j)) for j in range(ix.nlists)]
    for j, pv in queries:
        assert (np.diff(pv.astype(np.int64)) > 0).all() and pv[0] == 0 and pv[-1] == 0xFFFFFFFF and ix.start0[j] in pv
        v = ix.lists[j]
        if len(v):
            assert min(int(v[-1]) + 1, 0xFFFFFFFF) in pv
        for i in range(1, ix.units(j)):
            assert {int(v[256 * i - 1]), int(v[256 * i]) - 1, int(v[256 * i]), min(int(v[256 * i]) + 1, 0xFFFFFFFF)} <= set(pv.tolist())
    _hold(ix, queries, 5)


def test_reference_is_the_set_union_on_random_probes(matrix):
    ix = matrix
    rng = np.random.default_rng(5)
    queries = []
    for j in range(ix.nlists):
        v = ix.lists[j]
        for m in (0, 1, 70, 3000):
            hi = int(v[-1]) + 30000 if len(v) else 1 << 31
            cand = rng.integers(max(int(ix.start0[j]) - 30000, 0), hi, size=m, dtype=np.uint64).astype(np.uint32)
            take = v[rng.permutation(len(v))[:m // 2]] if len(v) else np.zeros(0, np.uint32)
            queries.append((j, np.unique(np.concatenate([cand, take]))))
    _hold(ix, queries, 0)


def test_whole_request_reference_equals_the_per_query_one(matrix):
    ix = matrix
    rng = np.random.default_rng(9)
    queries = [(j, ur.edge_probe(ix, j)[:: int(rng.integers(1, 4))]) for j in rng.permutation(ix.nlists)]
    queries += [(ix.of_len(0), np.zeros(0, np.uint32)), (ix.of_len(257), np.zeros(0, np.uint32)), (ix.of_len(0), np.array([3, 9], np.uint32))]
    ptr0 = 4
    probe = np.concatenate([np.full(ptr0, 77, np.uint32)] + [pv for _, pv in queries] + [np.full(6, 78, np.uint32)])
    pp = ptr0 + np.concatenate([[0], np.cumsum([len(pv) for _, pv in queries])]).astype(np.int64)
    a = ur.want_union(ix, queries, ptr0)
    b = ur.want_union_keys(ix, [j for j, _ in queries], pp, probe)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
