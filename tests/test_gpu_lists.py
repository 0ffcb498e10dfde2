"""GPU parity of the many-lists decode (include/turbopfor_gpu.h
tpf_p4ndec256v32_lists): many posting lists laid end to end, each an
n-variant stream, decoded in one call.  The streams are the oracle's
composition (tests/lists_ref.py), the expected decode is the original values,
bit-exact, plain and delta-1."""
import ctypes

import numpy as np
import pytest

import lists_ref as ref

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5A5A5A5
CLEAN = -1  # UINT64_MAX read back as int64


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _dev8(a, shift=0, pad=0):
    """packed bytes on the device, `shift` bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    buf = torch.zeros(len(a) + pad + 32, dtype=torch.uint8, device=DEV)
    s = (shift - buf.data_ptr()) % 16
    view = buf[s: s + len(a) + pad]
    assert view.data_ptr() % 16 == shift % 16
    view[: len(a)] = torch.from_numpy(a).to(DEV)
    return view


def _run(packed, offs, ptr, d1=False, start0=None, cap=None, slack=91, shift=0, pad=0, nunits=None):
    """Decode into a sentinel-filled buffer of `cap` values (default: ptr[-1])
    inside a larger one.  -> (whole buffer as uint32, err as int)"""
    cap = int(ptr[-1]) if cap is None else cap
    big = torch.full((max(cap, int(ptr[-1])) + slack,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    o = _dev64(offs if nunits is None else offs[: nunits + 1])
    tpf.decn256v32_lists(_dev8(packed, shift, pad), o, _dev64(ptr), d1=d1,
                         start0=None if start0 is None else _dev32(start0), out=big[:cap], err=err)
    return big.cpu().numpy().view(np.uint32), int(err.item())


def _check(got, err, ptr, vals):
    lo, hi = int(ptr[0]), int(ptr[-1])
    assert err == CLEAN
    assert np.array_equal(got[lo:hi], vals)
    assert (got[:lo] == SENT).all() and (got[hi:] == SENT).all()


def _lists(lens, d1, rng, start0=None, outliers=False):
    if d1:
        return [ref.d1_values(n, 0 if start0 is None else int(start0[j]), rng, outliers) for j, n in enumerate(lens)]
    return [ref.plain_values(n, rng) for n in lens]


# ---- the shape matrix ------------------------------------------------------
@pytest.fixture(scope="module")
def matrix():
    """(order seed, d1) -> the composed stream, built once."""
    built = {}
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
        for d1 in (False, True):
            start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
            lists = _lists(lens, d1, rng, start0)
            built[(seed, d1)] = (ref.compose(lists, d1, start0, ptr0=37), start0)
    return built


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_shape_matrix(matrix, seed, d1):
    """Lists that start and end on, one before and one after the boundaries of
    the 16-unit decode runs, the 64-unit sum runs and the 64-unit workgroups,
    and that span several of each; ptr[0] = 37, so every output position is
    odd-aligned, and the values around the lists stay untouched."""
    (packed, offs, ptr, vals), start0 = matrix[(seed, d1)]
    got, err = _run(packed, offs, ptr, d1, start0)
    _check(got, err, ptr, vals)


def test_start0_null_is_zero():
    rng = np.random.default_rng(5)
    lens = [0, 300, 256, 77, 0, 256 * 20 + 9, 1]
    lists = _lists(lens, True, rng)
    packed, offs, ptr, vals = ref.compose(lists, True, None, ptr0=3)
    a, ea = _run(packed, offs, ptr, True, None)
    b, eb = _run(packed, offs, ptr, True, np.zeros(len(lens), np.uint32))
    _check(a, ea, ptr, vals)
    assert eb == CLEAN and np.array_equal(a, b)


# ---- many heads per run ----------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_many_heads_per_run(d1):
    """220 consecutive tail-only lists (16 heads in every decode run), 70
    consecutive empty lists in the middle, empty lists first and last."""
    rng = np.random.default_rng(7)
    lens = [0, 0] + list(rng.integers(1, 256, size=110)) + [0] * 70 + list(rng.integers(1, 256, size=110)) + [700, 0, 256, 0]
    start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    lists = _lists(lens, d1, rng, start0)
    packed, offs, ptr, vals = ref.compose(lists, d1, start0, ptr0=1)
    got, err = _run(packed, offs, ptr, d1, start0)
    _check(got, err, ptr, vals)


# ---- degenerate partitions --------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_one_list_equals_the_single_list_call(d1):
    rng = np.random.default_rng(8)
    n = 256 * 150 + 77
    v = ref.d1_values(n, 49, rng) if d1 else ref.plain_values(n, rng)
    packed, offs, ptr, vals = ref.compose([v], d1, [49])
    got, err = _run(packed, offs, ptr, d1, np.array([49], np.uint32), slack=0)
    single = tpf.decn256v32(_dev8(packed), _dev64(offs), n, d1=d1, start0=49)
    assert err == CLEAN
    assert np.array_equal(got, single.cpu().numpy().view(np.uint32))
    assert np.array_equal(got, vals)


def test_one_block_lists_equal_the_per_block_starts_call():
    rng = np.random.default_rng(9)
    nl = 150
    start0 = rng.integers(0, 1 << 32, size=nl, dtype=np.uint64).astype(np.uint32)
    lists = _lists([256] * nl, True, rng, start0)
    packed, offs, ptr, vals = ref.compose(lists, True, start0)
    assert len(offs) == nl + 1
    got, err = _run(packed, offs, ptr, True, start0, slack=0)
    batch = tpf.dec256v32(_dev8(packed), _dev64(offs), nl, starts=_dev32(start0))
    assert err == CLEAN
    assert np.array_equal(got, batch.cpu().numpy().view(np.uint32).reshape(-1))
    assert np.array_equal(got, vals)


# ---- exceptions --------------------------------------------------------------
def test_d1_exception_kinds():
    """Gaps with outliers at 0.5 % to 30 % per block: vbyte and bitmap
    exception blocks both occur (phase A's lane path and its declined blocks)."""
    rng = np.random.default_rng(10)
    lens = [256 * 70 + 130, 5, 256 * 3, 256 * 33 + 1, 0, 200, 256 * 18 + 255]
    start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    lists = _lists(lens, True, rng, start0, outliers=True)
    packed, offs, ptr, vals = ref.compose(lists, True, start0, ptr0=2)
    kinds = ref.block_kinds(packed, offs, ptr - ptr[0])
    assert kinds["vbyte"] >= 5 and kinds["bitmap"] >= 5, kinds
    got, err = _run(packed, offs, ptr, True, start0)
    _check(got, err, ptr, vals)


def test_wrap():
    """start0 within 10^6 of 2^32: every list's chained sums wrap."""
    rng = np.random.default_rng(11)
    lens = [256 * 20 + 5, 100, 256, 256 * 65, 0, 3]
    start0 = ((1 << 32) - rng.integers(1, 10 ** 6, size=len(lens))).astype(np.uint32)
    lists = _lists(lens, True, rng, start0)
    assert all(int(v[-1]) < int(s) for v, s in zip(lists, start0) if len(v) >= 256)  # wrapped
    packed, offs, ptr, vals = ref.compose(lists, True, start0, ptr0=5)
    got, err = _run(packed, offs, ptr, True, start0)
    _check(got, err, ptr, vals)


@pytest.mark.parametrize("shift", [1, 3, 7])
def test_misaligned_input(matrix, shift):
    (packed, offs, ptr, vals), start0 = matrix[(1, True)]
    got, err = _run(packed, offs, ptr, True, start0, shift=shift)
    _check(got, err, ptr, vals)


def test_more_lists_than_a_tile():
    """Crosses this path's own tiles over LISTS: 5,000 lists are more than one
    4,096-entry tile of the run scan over the lists' unit counts (p4_scan.h,
    reused unchanged), more than 64 x 64 lists, so the cooperative search for a
    run's list takes three steps, and many 16-list runs and 64-list workgroups
    of the tails kernel; runs start inside lists of 17 to 32 units."""
    rng = np.random.default_rng(12)
    kind = rng.random(5000)
    lens = np.where(kind < 0.78, rng.integers(0, 256, size=5000),
                    np.where(kind < 0.995, rng.integers(256, 450, size=5000), rng.integers(4097, 8000, size=5000)))
    start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    lists = _lists([int(n) for n in lens], True, rng, start0)
    packed, offs, ptr, vals = ref.compose(lists, True, start0, ptr0=9)
    got, err = _run(packed, offs, ptr, True, start0)
    _check(got, err, ptr, vals)


# ---- error reporting -------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(13)
    lens = [300, 0, 256 * 2 + 100, 256, 90, 0, 256 * 17]
    plain = ref.compose(_lists(lens, False, rng), False, None, ptr0=11)
    start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    d1 = ref.compose(_lists(lens, True, rng, start0), True, start0, ptr0=11)
    return lens, plain, d1, start0


@pytest.mark.parametrize("d1", [False, True])
def test_tail_error_index(small, d1):
    """The tail of list 2 (units 2..4 of the stream: its tail is unit 4) with
    its end offset bumped by one is reported as global unit 4."""
    lens, plain, chained, start0 = small
    packed, offs, ptr, _ = chained if d1 else plain
    _, base = ref.units_loop(ptr)
    u = base[3] - 1
    assert u == 4 and lens[2] % 256
    bad = offs.copy()
    bad[u + 1] += 1
    _, err = _run(packed, bad, ptr, d1, start0, pad=64)
    assert err == u


def _untouched(got):
    assert (got == SENT).all()


def test_decreasing_list_ptr(small):
    lens, (packed, offs, ptr, _), _, _ = small
    j = 3
    bad = ptr.copy()
    bad[j + 1] = bad[j] - 1
    got, err = _run(packed, offs, bad, cap=int(ptr[-1]))
    assert err == (len(offs) - 1) + j
    _untouched(got)


def test_list_ptr_past_the_capacity(small):
    lens, (packed, offs, ptr, _), _, _ = small
    cap = int(ptr[4]) - 1  # list 3 (256 values) is the first to end past it
    j = int(np.argmax(ptr[1:] > cap))
    assert j == 3
    got, err = _run(packed, offs, ptr, cap=cap)
    assert err == (len(offs) - 1) + j
    _untouched(got)


def test_units_do_not_add_up(small):
    lens, (packed, offs, ptr, _), _, _ = small
    nunits = len(offs) - 2  # one unit short of what list_ptr implies
    got, err = _run(packed, offs, ptr, nunits=nunits)
    assert err == nunits + len(lens)
    _untouched(got)


def test_host_refusals(small):
    lens, (packed, offs, ptr, _), _, _ = small
    L = tpf.lib()
    nunits, nlists = len(offs) - 1, len(lens)
    ws_bytes = int(L.tpf_p4ndec256v32_lists_workspace_size(nunits, nlists))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.empty(int(ptr[-1]), dtype=torch.int32, device=DEV)
    p, o, lp = _dev8(packed), _dev64(offs), _dev64(ptr)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.tpf_p4ndec256v32_lists(p.data_ptr(), p.numel(), o.data_ptr(), nunits, lp.data_ptr(), nlists, 0, None, out.data_ptr(),
                                  out.numel(), ws.data_ptr(), ws_bytes - 1, None, s)
    assert rc == -1 and b"tpf_p4ndec256v32_lists" in L.tpf_last_error() and b"workspace" in L.tpf_last_error()
    rc = L.tpf_p4ndec256v32_lists(p.data_ptr(), p.numel(), None, nunits, lp.data_ptr(), nlists, 0, None, out.data_ptr(),
                                  out.numel(), ws.data_ptr(), ws_bytes, None, s)
    assert rc == -1 and b"tpf_p4ndec256v32_lists" in L.tpf_last_error() and b"null" in L.tpf_last_error()
    # nothing to do: a successful no-op that still reports clean
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    rc = L.tpf_p4ndec256v32_lists(p.data_ptr(), p.numel(), o.data_ptr(), nunits, lp.data_ptr(), 0, 0, None, out.data_ptr(),
                                  out.numel(), ws.data_ptr(), ws_bytes, err.data_ptr(), s)
    assert rc == 0 and int(err.item()) == CLEAN
