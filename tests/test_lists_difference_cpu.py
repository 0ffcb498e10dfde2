"""CPU-only checks of the host surface of the difference with a resident index
(include/turbopfor_gpu.h tpf_lists_difference): the symbols are exported, the
workspace-size function is a pure host function of probe_values alone, the
arguments are judged before any device call (TPF_EINVAL), the entry point
reports TPF_ENODEV instead of falling back to a CPU codec -- and the numpy
restatement of the definition the GPU tests compare against
(tests/lists_difference_ref.py) is the set difference, and the miss side of the
union's reference (tests/lists_union_ref.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lists_difference_ref as dr
from lists_index import Index
import lists_ref as ref
import lists_union_ref as ur
import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
EINVAL, ENODEV = -1, -3
P = 0x1000  # a non-null pointer that is never followed: every call below is refused on the host
STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 262144, 262145, 10 ** 6, 0x3FFFFFFF]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    L = turbopfor_amd.declare(ctypes.CDLL(LIB))
    assert hasattr(L, "tpf_lists_difference"), "the library does not export tpf_lists_difference"
    return L


def _no_device():
    return subprocess.run([sys.executable, "-c", "import torch,sys;sys.exit(0 if torch.cuda.is_available() else 1)"]).returncode != 0


def test_symbols_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_lists_difference", "tpf_lists_difference_workspace_size"} <= exported
    with open(os.path.join(ROOT, "turbopfor-cpp_amd", "python", "turbopfor_amd.py")) as f:
        assert "def lists_difference(" in f.read()
    with open(os.path.join(ROOT, "include", "turbopfor_gpu.h")) as f:
        hdr = f.read()
    assert "int tpf_lists_difference(" in hdr and "size_t tpf_lists_difference_workspace_size(uint64_t nq, uint64_t probe_values);" in hdr


def test_workspace_size_is_a_pure_host_function(lib):
    f = lib.tpf_lists_difference_workspace_size
    for nq in (0, 1, 1000, 10 ** 6):
        for a, b in zip(STEPS, STEPS[1:]):
            assert 0 < f(nq, a) <= f(nq, b), ("probe_values", a, b, nq)
    for pv in STEPS:
        assert f(1, pv) % 8 == 0
        for nq in STEPS:
            assert f(nq, pv) == f(1, pv), ("nq sizes nothing", nq, pv)  # independent of nq
    assert f(10, 10 ** 6) < f(10, 10 ** 7)
    assert f(1000, 10 ** 6) == f(1000, 10 ** 6)  # no state


def test_workspace_is_a_few_words_per_probe_value(lib):
    f = lib.tpf_lists_difference_workspace_size
    for pv in (0, 1, 5, 10 ** 4, 10 ** 7, 0x7FFFFFFF):
        assert f(7, pv) < 32 * pv + 65536, pv


def _call(lib, d_in=P, d_off=P, nunits=10, ptr=P, lu=P, nlists=5, ul=P, probe=P, probe_values=100, probe_ptr=P, qlist=P, nq=3, out=P,
          out_values=1000, out_ptr=P, pidx=None, tpos=None, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.tpf_lists_difference_workspace_size(min(nq, 1 << 20), min(probe_values, 1 << 20))
    return lib.tpf_lists_difference(d_in, 100, d_off, nunits, ptr, lu, nlists, None, ul, probe, probe_values, probe_ptr, qlist, nq, out,
                                    out_values, out_ptr, pidx, tpos, ws, ws_bytes, None, None)


@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "lu", "ul", "probe_ptr", "qlist", "out_ptr", "ws", "probe", "out"])
def test_null_pointer_is_einval(lib, arg):
    assert _call(lib, **{arg: None}) == EINVAL
    assert b"tpf_lists_difference" in lib.tpf_last_error() and b"null" in lib.tpf_last_error()


def test_null_probe_and_out_are_allowed_when_empty(lib):
    # with nothing to read or write the two pointers may be null: the call gets past them to the workspace check
    assert _call(lib, probe=None, probe_values=0, out=None, out_values=0, ws_bytes=0) == EINVAL
    assert b"tpf_lists_difference" in lib.tpf_last_error() and b"workspace" in lib.tpf_last_error()


def test_small_workspace_is_einval(lib):
    need = lib.tpf_lists_difference_workspace_size(3, 100)
    assert _call(lib, ws_bytes=need - 1) == EINVAL
    assert b"tpf_lists_difference" in lib.tpf_last_error() and b"workspace" in lib.tpf_last_error()


@pytest.mark.parametrize("kw", [dict(nlists=0x80000000), dict(nunits=0x80000000), dict(nq=0x80000000), dict(probe_values=0x80000000)])
def test_limits_are_einval(lib, kw):
    assert _call(lib, ws_bytes=2 ** 62, **kw) == EINVAL
    assert b"tpf_lists_difference" in lib.tpf_last_error() and b"0x7FFFFFFF" in lib.tpf_last_error()


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        return  # a HIP device is visible: the GPU tests call the entry point
    for call in (lambda: _call(lib), lambda: _call(lib, pidx=P, tpos=P),
                 lambda: _call(lib, nq=0, qlist=None, probe_ptr=None, probe=None, probe_values=0, out=None, out_values=0, ws=None,
                               ws_bytes=0)):
        assert call() == ENODEV
        assert b"no CPU fallback" in lib.tpf_last_error()


# ---- the reference of the GPU tests is the set difference, and the union's misses ----------
@pytest.fixture(scope="module")
def matrix():
    rng = np.random.default_rng(17)
    lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
    ix = Index(lens, rng, ptr0=37, start_bits=31)
    assert ix.ascends()
    return ix


def _hold(ix, queries, ptr0):
    """ascending probes: against np.setdiff1d and against union_one"""
    vals, out_ptr, pidx, tpos = dr.want_difference(ix, queries, ptr0)
    assert out_ptr[0] == 0 and len(vals) == out_ptr[-1] == len(pidx) == len(tpos)
    probe = np.concatenate([np.zeros(ptr0, np.uint32)] + [np.asarray(pv, np.uint32) for _, pv in queries])
    at = ptr0
    for k, (j, pv) in enumerate(queries):
        pv = np.asarray(pv, np.uint32)
        assert (np.diff(pv.astype(np.int64)) > 0).all()
        a, b = int(out_ptr[k]), int(out_ptr[k + 1])
        lst = ix.lists[j]
        assert np.array_equal(vals[a:b], np.setdiff1d(pv, lst)), (k, j)
        assert np.array_equal(probe[pidx[a:b]], vals[a:b]) and ((pidx[a:b] >= at) & (pidx[a:b] < at + len(pv))).all()
        # tpos: the list values below v, so the value there (if any) is the first above v
        t = tpos[a:b].astype(np.int64)
        assert (t <= len(lst)).all()
        assert (lst[t[t < len(lst)]] > vals[a:b][t < len(lst)]).all() and (lst[t[t > 0] - 1] < vals[a:b][t > 0]).all()
        # the union's reference: a difference's values, pidx and tpos are exactly the union's slots with tpos == NONE,
        # each tpos being that slot minus M(i), the misses before it
        uv, upi, utp = ur.union_one(lst, pv, at)
        slots = np.nonzero(utp == ur.NONE)[0]
        assert np.array_equal(uv[slots], vals[a:b]) and np.array_equal(upi[slots], pidx[a:b])
        assert np.array_equal(slots - np.arange(len(slots)), t)
        at += len(pv)
    return len(vals)


def test_reference_is_the_set_difference_at_the_edges(matrix):
    ix = matrix
    queries = [(j, dr.edge_probe(ix, j)) for j in range(ix.nlists)]
    assert _hold(ix, queries, 5) > 2 * ix.nlists
    # an empty list: everything is a miss and tpos is 0
    e = ix.of_len(0)
    v, _, pi, tp = dr.want_difference(ix, [(e, queries[e][1])], 0)
    assert np.array_equal(v, queries[e][1]) and (tp == 0).all() and np.array_equal(pi, np.arange(len(v)))


def test_reference_is_the_set_difference_on_random_probes(matrix):
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


def test_reference_reports_every_occurrence_in_probe_order(matrix):
    ix = matrix
    j = ix.of_len(257)
    v = ix.lists[j]
    pv = np.array([int(v[5]) + 1, int(v[5]), int(v[-1]) + 9, int(v[5]) + 1, 0, int(v[0]), 0], np.uint32)
    assert not np.isin(pv[[0, 2, 4]], v).any()
    vals, out_ptr, pidx, tpos = dr.want_difference(ix, [(j, pv)], 3)
    assert vals.tolist() == pv[[0, 2, 3, 4, 6]].tolist() and pidx.tolist() == [3, 5, 6, 7, 9] and out_ptr.tolist() == [0, 5]
    assert tpos.tolist() == [6, 257, 6, 0, 0]


def test_whole_request_reference_equals_the_per_query_one(matrix):
    ix = matrix
    rng = np.random.default_rng(9)
    queries = [(j, dr.edge_probe(ix, j)[:: int(rng.integers(1, 4))]) for j in rng.permutation(ix.nlists)]
    queries += [(ix.of_len(0), np.zeros(0, np.uint32)), (ix.of_len(257), np.zeros(0, np.uint32)), (ix.of_len(0), np.array([3, 9], np.uint32))]
    queries.append((ix.of_len(513), ix.lists[ix.of_len(513)][::-2]))  # descending members: no miss
    ptr0 = 4
    probe = np.concatenate([np.full(ptr0, 77, np.uint32)] + [pv for _, pv in queries] + [np.full(6, 78, np.uint32)])
    pp = ptr0 + np.concatenate([[0], np.cumsum([len(pv) for _, pv in queries])]).astype(np.int64)
    a = dr.want_difference(ix, queries, ptr0)
    b = dr.want_difference_keys(ix, [j for j, _ in queries], pp, probe)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
