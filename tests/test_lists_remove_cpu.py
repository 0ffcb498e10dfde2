"""CPU-only checks of the host surface of the delete from a resident index
(include/turbopfor_gpu.h tpf_lists_remove): the symbols are exported, the
arguments are judged before any device call (TPF_EINVAL, with the cause in the
message), the bound and the workspace size never decrease, the bound covers
every case of the GPU matrix (tests/test_gpu_lists_remove.py), the numpy
restatement (tests/lists_remove_ref.py) agrees with a hand-written example, and
-- on the oracle's bytes alone -- the principle the call rests on: the units of
a list before the one that holds its first removed position keep their bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lists_ref as ref
import lists_remove_ref as rr
import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
u64 = ctypes.c_uint64
vp = ctypes.c_void_p
EINVAL, ENODEV = -1, -3
P = 0x1000  # a non-null pointer that is never followed: every call below is refused on the host
STEPS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10 ** 6, 0x3FFFFFFF]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    return turbopfor_amd.declare(ctypes.CDLL(LIB))


@pytest.fixture(scope="module")
def matrix():
    return {k: rr.matrix_case(*k) for k in ((True, True), (True, False), (False, False))}


def _no_device():
    return subprocess.run([sys.executable, "-c", "import torch,sys;sys.exit(0 if torch.cuda.is_available() else 1)"]).returncode != 0


def test_symbols_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_lists_remove", "tpf_lists_remove_bound", "tpf_lists_remove_workspace_size"} <= exported
    with open(os.path.join(ROOT, "turbopfor-cpp_amd", "python", "turbopfor_amd.py")) as f:
        src = f.read()
    assert "def lists_remove(" in src and "def lists_remove_bound(" in src
    assert turbopfor_amd.prototypes()["tpf_lists_remove"] == (
        ctypes.c_int, [vp, u64, vp, u64, vp, vp, u64, ctypes.c_int, vp, vp, vp, u64, vp, vp, u64, u64, vp, u64, vp, u64, vp, vp, vp, vp,
                       ctypes.c_size_t, vp, vp])


def _call(lib, d_in=P, d_off=P, nunits=10, ptr=P, lu=P, nlists=5, d1=1, st=None, ul=P, pos=P, pos_values=100, pptr=P, ql=P, nq=3,
          stage=500, out=P, out_cap=1000, off_out=P, units_cap=20, lptr_out=P, lunit_out=P, ul_out=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        sm = lambda x: min(x, 1 << 20)
        ws_bytes = lib.tpf_lists_remove_workspace_size(sm(nunits), sm(nlists), sm(nq), sm(pos_values), sm(stage))
    return lib.tpf_lists_remove(d_in, 100, d_off, nunits, ptr, lu, nlists, d1, st, ul, pos, pos_values, pptr, ql, nq, stage, out, out_cap,
                                off_out, units_cap, lptr_out, lunit_out, ul_out, ws, ws_bytes, None, None)


def _msg(lib, *words):
    m = lib.tpf_last_error()
    assert b"tpf_lists_remove" in m
    for w in words:
        assert w in m, (w, m)


@pytest.mark.parametrize("d1", [0, 1])
@pytest.mark.parametrize("arg", ["d_in", "d_off", "ptr", "lu", "pptr", "ql", "pos", "out", "off_out", "lptr_out", "lunit_out", "ws"])
def test_null_pointer_is_einval(lib, arg, d1):
    assert _call(lib, d1=d1, **{arg: None}) == EINVAL
    _msg(lib, b"null")


def test_null_tables_are_refused_only_with_d1(lib):
    for kw in (dict(ul=None), dict(ul_out=None)):
        assert _call(lib, d1=1, **kw) == EINVAL
        _msg(lib, b"d_unit_last")
        # the plain form ignores both tables: the call gets past them to the workspace check
        assert _call(lib, d1=0, ws_bytes=0, **kw) == EINVAL
        _msg(lib, b"workspace")
    # d_start0 is optional with d1 too
    assert _call(lib, d1=1, st=None, ws_bytes=0) == EINVAL
    _msg(lib, b"workspace")


def test_null_pointers_are_allowed_where_the_sizes_do_not_need_them(lib):
    # no units: nothing of the stream, its offsets or its table is read; no queries: none of the removals; no positions: no d_pos
    for kw in (dict(nunits=0, d_in=None, d_off=None, ul=None), dict(nq=0, pos=None, pptr=None, ql=None), dict(pos_values=0, pos=None),
               dict(out_cap=0, out=None)):
        assert _call(lib, ws_bytes=0, **kw) == EINVAL
        _msg(lib, b"workspace")


def test_small_workspace_is_einval(lib):
    need = lib.tpf_lists_remove_workspace_size(10, 5, 3, 100, 500)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == EINVAL
    _msg(lib, b"workspace")


@pytest.mark.parametrize("kw", [dict(nunits=0x80000000), dict(nlists=0x80000000), dict(nq=0x80000000), dict(pos_values=0x80000000),
                                dict(stage=0x80000000), dict(units_cap=0x80000000), dict(stage=0x7FFFFFFF, nq=0x7FFFFFFF)])
def test_limits_are_einval(lib, kw):
    assert _call(lib, ws_bytes=2 ** 62, **kw) == EINVAL
    _msg(lib, b"0x7FFFFFFF")


def test_no_cpu_fallback_without_device(lib):
    if not _no_device():
        pytest.skip("a HIP device is visible")
    for call in (lambda: _call(lib), lambda: _call(lib, d1=0, ul=None, ul_out=None), lambda: _call(lib, nq=0, pos=None, pptr=None, ql=None),
                 lambda: _call(lib, nlists=0, ptr=None, lu=None, ws=None, ws_bytes=0)):
        assert call() == ENODEV
        assert b"no CPU fallback" in lib.tpf_last_error()


def test_bound_and_workspace_never_decrease(lib):
    f = lib.tpf_lists_remove_bound
    for x, y in ((0, 0), (1, 1), (1000, 10), (10, 1000), (10 ** 6, 10 ** 6)):
        for a, b in zip(STEPS, STEPS[1:]):
            assert f(a, x, y) <= f(b, x, y) and f(x, a, y) <= f(x, b, y) and f(x, y, a) <= f(x, y, b), (a, b, x, y)
    g = lib.tpf_lists_remove_workspace_size
    for base in ((1, 1, 1, 1, 1), (1000, 10, 3, 50, 5000), (10, 1000, 700, 10 ** 5, 10 ** 6)):
        for i in range(5):
            for a, b in zip(STEPS, STEPS[1:]):
                lo, hi = list(base), list(base)
                lo[i], hi[i] = a, b
                if lo[1] == 0:
                    continue  # nlists == 0 is a no-op that needs nothing
                assert g(*lo) <= g(*hi), (i, a, b, base)
    assert f(123, 0, 0) >= 123
    assert g(10, 0, 3, 100, 500) == 0  # nlists == 0 is a no-op


def test_bound_covers_the_matrix(lib, matrix):
    """Every targeted list alone with its exact staging, and each matrix as one index with its exact staging and with the
    staging that always suffices: the bound is at least the byte length of the oracle's composition of the shortened lists."""
    for (d1, st), c in matrix.items():
        assert lib.tpf_lists_remove_bound(len(c.packed), c.nq, c.staged) >= len(c.xpacked)
        assert lib.tpf_lists_remove_bound(len(c.packed), c.nq, c.targeted) >= len(c.xpacked)
        assert c.staged <= c.targeted
        for j in c.removals:
            s = len(c.lists[j]) - 256 * c.u0[j] if j in c.u0 else 0
            assert lib.tpf_lists_remove_bound(len(c.list_bytes(j)), 1, s) >= len(c.list_bytes(j, new=True)), (j, c.plan[j])


def test_reference_on_a_hand_written_example():
    a = np.arange(10, 10 + 300, dtype=np.uint32)
    b = np.array([7, 9, 11], dtype=np.uint32)
    c = np.array([5], dtype=np.uint32)
    got = rr.remove([a, b, c], {0: [0, 256, 299], 2: [0]})
    assert got[0].tolist() == list(range(11, 266)) + list(range(267, 309))
    assert got[1] is b and got[2].tolist() == []
    k = rr.Case([a, b, c], {0: np.array([0, 256, 299]), 1: np.zeros(0), 2: np.array([0])}, True, np.array([3, 0, 1], np.uint32), ptr0=0,
                pos0=2)
    assert k.qlist.tolist() == [0, 1, 2] and k.pptr.tolist() == [2, 5, 5, 6]
    assert k.pos[2:6].tolist() == [0, 256, 299, 0] and k.pos[0] == rr.JUNK and k.pos[6] == rr.JUNK
    assert k.u0 == {0: 0, 2: 0} and k.staged == 301 and k.targeted == 304
    assert k.xptr.tolist() == [0, 297, 300, 300] and k.xbase.tolist() == [0, 2, 3, 3]
    assert k.xtable.tolist() == [266 + 1, 308, 11]
    assert k.table.tolist() == [265, 309, 11, 5]
    # ... and the composition is the oracle's of the shortened lists, list by list
    p0, o0, _, _ = ref.compose([got[0]], True, [3])
    assert np.array_equal(k.list_bytes(0, new=True), p0)


def test_matrix_holds_the_cases(matrix):
    c = matrix[(True, True)]
    got = {(n, p) for n, p in c.plan if p is not None}
    want = {(n, p) for n in rr.LENS for p in rr.PATTERNS if rr.positions(p, n, np.random.default_rng(0)) is not None}
    assert got == want and len(want) >= 70
    assert {(0, "none"), (1, "all"), (256, "lastfull"), (257, "tail"), (256 * 17 + 3, "unit"), (513, "p255_256")} <= got
    u0s = set(c.u0.values())
    assert 0 in u0s and max(u0s) >= 8                                                    # u0 == 0 and u0 > 0
    old, new = [len(v) for v in c.lists], [len(v) for v in c.new]
    assert any(o and not n for o, n in zip(old, new))                                     # a list emptied
    assert any(o % 256 == 0 and n % 256 for o, n in zip(old, new) if n)                   # a tail created
    assert any(o % 256 and n % 256 == 0 for o, n in zip(old, new) if n)                   # a tail removed
    touched = [j in c.u0 for j in range(c.nlists)]
    assert any(touched[j - 1] and not touched[j] and old[j] and touched[j + 1] for j in range(1, c.nlists - 1))
    assert int(c.ptr[0]) == rr.PTR0 and int(c.pptr[0]) == rr.POS0
    for cc in matrix.values():
        kinds = ref.block_kinds(cc.xpacked, cc.xoffs, cc.xptr)
        assert kinds["bitmap"] > 0 and kinds["vbyte"] > 0, kinds  # both exception layouts among the expected full blocks


def test_units_before_the_first_removed_position_keep_their_bytes(matrix):
    """The oracle's bytes alone: for every list of every matrix, units [0, u0) of the expected stream are byte-identical
    to the old stream's, and a list that loses nothing keeps all of them."""
    seen = 0
    for c in matrix.values():
        for j in range(c.nlists):
            keep = c.u0.get(j, ref.n_units(len(c.lists[j])))
            a0, b0 = int(c.base[j]), int(c.xbase[j])
            olds = c.offs[a0: a0 + keep + 1].astype(np.int64) - int(c.offs[a0])
            news = c.xoffs[b0: b0 + keep + 1].astype(np.int64) - int(c.xoffs[b0])
            assert np.array_equal(olds, news), (j, c.plan[j])
            n = int(olds[-1])
            assert np.array_equal(c.packed[int(c.offs[a0]): int(c.offs[a0]) + n], c.xpacked[int(c.xoffs[b0]): int(c.xoffs[b0]) + n])
            seen += keep > 0 and j in c.u0
    assert seen >= 30
