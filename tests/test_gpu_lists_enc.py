"""GPU parity of the many-lists encode (include/turbopfor_gpu.h
tpf_p4nenc256v32_lists): many posting lists in one dense value array, each
encoded as an n-variant stream, the streams laid end to end, in one call.
Expected bytes, offsets and pointers are the oracle's composition
(tests/lists_ref.py); every check compares packed[:total] and all nunits + 1
offsets for equality, with d_out a window inside a sentinel-filled buffer."""
import ctypes

import numpy as np
import pytest

import lists_enc_inputs as inp
import lists_ref as ref

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5
SENT64 = 0x5A5A5A5A5A5A5A5A
CLEAN = -1  # UINT64_MAX read back as int64
LEAD = 48   # sentinel bytes in front of the output window


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _values(vals, ptr, in_shift=0, place="middle"):
    """The value array on the device.  Values sit at their list_ptr positions
    (positions below ptr[0] are filler that must not matter); the array itself
    starts in_shift bytes past a 16-byte boundary.  place: "middle" leaves
    filler before and after, "start" / "end" put the window at the very start /
    end of its own allocation (ptr[0] == 0 and in_values == ptr[-1])."""
    lo, hi = int(ptr[0]), int(ptr[-1])
    assert len(vals) == hi - lo
    filler = np.random.default_rng(99).integers(0, 1 << 32, size=lo, dtype=np.uint64).astype(np.uint32)
    host = np.concatenate([filler, np.asarray(vals, dtype=np.uint32)])
    if place == "middle":
        buf = torch.empty(len(host) + 8 + 61, dtype=torch.int32, device=DEV)
        buf.fill_(0x3C3C3C3C)
        s = ((in_shift - buf.data_ptr()) % 16) // 4
        view = buf[s: s + len(host)]
        assert view.data_ptr() % 16 == in_shift % 16
    elif place == "start":
        assert lo == 0
        buf = torch.empty(len(host) + 61, dtype=torch.int32, device=DEV)
        buf.fill_(0x3C3C3C3C)
        view = buf[: len(host)]
    else:
        assert lo == 0
        buf = torch.empty(len(host) + 61, dtype=torch.int32, device=DEV)
        buf.fill_(0x3C3C3C3C)
        view = buf[61:]
        assert view.data_ptr() + 4 * view.numel() == buf.data_ptr() + 4 * buf.numel()
    view.copy_(_dev32(host))
    return view


def _run(vals, ptr, nunits, d1=False, start0=None, cap=None, in_shift=0, out_shift=0, place="middle", in_values=None, call_ptr=None):
    """One call through the binding into a window of `cap` bytes inside a larger
    sentinel-filled buffer.  -> (before, window, after as uint8 arrays,
    offsets as uint64 [nunits + 1], err).  in_values: the readable length passed
    (default: all of ptr[-1]); call_ptr: the pointers passed (default: ptr)."""
    values = _values(vals, ptr, in_shift, place)
    if in_values is not None:
        values = values[:in_values]
    cap = tpf.lists_enc_bound(len(vals), len(ptr) - 1) if cap is None else cap
    big = torch.full((LEAD + 16 + cap + 97,), SENT, dtype=torch.uint8, device=DEV)
    s = LEAD + (out_shift - (big.data_ptr() + LEAD)) % 16
    win = big[s: s + cap]
    assert win.data_ptr() % 16 == out_shift % 16
    offs = torch.full((nunits + 1,), SENT64, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    got, got_offs = tpf.encn256v32_lists(values, _dev64(ptr if call_ptr is None else call_ptr), d1=d1, start0=None if start0 is None else _dev32(start0),
                                         nunits=nunits, out=win, offsets=offs, err=err)
    assert got.data_ptr() == win.data_ptr() and got.numel() == cap  # untrimmed: the asynchronous form
    b = big.cpu().numpy()
    return b[:s], b[s: s + cap], b[s + cap:], got_offs.cpu().numpy().view(np.uint64), int(err.item())


def _check(res, packed, offs):
    before, win, after, got_offs, err = res
    total = len(packed)
    assert err == CLEAN
    assert np.array_equal(got_offs, offs)
    assert int(got_offs[-1]) == total
    assert np.array_equal(win[:total], packed)
    assert (before == SENT).all() and (win[total:] == SENT).all() and (after == SENT).all()


_lists, matrix_inputs, kinds_inputs = inp.lists, inp.matrix_inputs, inp.kinds_inputs


# ---- the shape matrix ------------------------------------------------------
@pytest.fixture(scope="module")
def matrix():
    """(order seed, d1) -> the composed stream, built once."""
    return {k: (ref.compose(lists, k[1], start0, ptr0=37), start0) for k, (lists, start0) in matrix_inputs().items()}


@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (4, 1), (8, 3), (12, 7)])
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_shape_matrix(matrix, seed, d1, in_shift, out_shift):
    """Lists that start and end on, one before and one after one unit, the
    16-unit, 32-unit and 64-unit boundaries, and that span several runs;
    ptr[0] = 37, random start0; d_in itself 0 / 4 / 8 / 12 bytes and d_out
    0 / 1 / 3 / 7 bytes past a 16-byte boundary."""
    (packed, offs, ptr, vals), start0 = matrix[(seed, d1)]
    _check(_run(vals, ptr, len(offs) - 1, d1, start0, in_shift=in_shift, out_shift=out_shift), packed, offs)


@pytest.mark.parametrize("in_shift", [0, 4, 8, 12])
@pytest.mark.parametrize("out_shift", [0, 1, 3, 7])
def test_alignment_cross(matrix, in_shift, out_shift):
    (packed, offs, ptr, vals), start0 = matrix[(1, True)]
    _check(_run(vals, ptr, len(offs) - 1, True, start0, in_shift=in_shift, out_shift=out_shift), packed, offs)


# ---- many heads per run ----------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_many_heads_per_run(d1):
    """Tails back to back, a tail between full blocks of one run, full blocks
    of different lists adjacent, 70 empty lists in a row, empty lists first
    and last."""
    rng = np.random.default_rng(7)
    lens = [0, 0] + list(rng.integers(1, 256, size=110)) + [0] * 70 + list(rng.integers(1, 256, size=110)) + [700, 0, 256, 0] \
        + [256, 512, 3, 256, 0, 256 * 2 + 1, 256, 0]
    start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    lists = _lists([int(n) for n in lens], d1, rng, start0)
    packed, offs, ptr, vals = ref.compose(lists, d1, start0, ptr0=1)
    _check(_run(vals, ptr, len(offs) - 1, d1, start0), packed, offs)


# ---- exceptions --------------------------------------------------------------
def test_d1_exception_kinds():
    """Gaps with outliers at 0.5 % to 30 % per block: vbyte and bitmap
    exception blocks both occur, so both emission paths and the run copy's
    long blocks are crossed."""
    lists, start0 = kinds_inputs()
    packed, offs, ptr, vals = ref.compose(lists, True, start0, ptr0=2)
    kinds = ref.block_kinds(packed, offs, ptr - ptr[0])
    assert kinds["vbyte"] >= 5 and kinds["bitmap"] >= 5, kinds
    _check(_run(vals, ptr, len(offs) - 1, True, start0), packed, offs)


def test_wrap():
    """start0 within 10^6 of 2^32: the deltas of every list's first unit wrap."""
    rng = np.random.default_rng(11)
    lens = [256 * 20 + 5, 100, 256, 256 * 65, 0, 3]
    start0 = ((1 << 32) - rng.integers(1, 10 ** 6, size=len(lens))).astype(np.uint32)
    lists = _lists(lens, True, rng, start0)
    packed, offs, ptr, vals = ref.compose(lists, True, start0, ptr0=5)
    _check(_run(vals, ptr, len(offs) - 1, True, start0), packed, offs)


def test_more_lists_than_a_tile():
    """5,000 lists: more than one 4,096-entry tile of the run scan over the
    lists, three steps of the cooperative list search, many 16-list runs of the
    tails kernels; runs start inside lists of 17 to 32 units."""
    rng = np.random.default_rng(12)
    kind = rng.random(5000)
    lens = np.where(kind < 0.78, rng.integers(0, 256, size=5000),
                    np.where(kind < 0.995, rng.integers(256, 450, size=5000), rng.integers(4097, 8000, size=5000)))
    start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    lists = _lists([int(n) for n in lens], True, rng, start0)
    packed, offs, ptr, vals = ref.compose(lists, True, start0, ptr0=9)
    _check(_run(vals, ptr, len(offs) - 1, True, start0), packed, offs)


# ---- degenerate partitions --------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_one_list_equals_the_single_list_call(d1):
    rng = np.random.default_rng(8)
    n = 256 * 150 + 77
    v = ref.d1_values(n, 49, rng) if d1 else ref.plain_values(n, rng)
    packed, offs, ptr, vals = ref.compose([v], d1, [49])
    res = _run(vals, ptr, len(offs) - 1, d1, np.array([49], np.uint32))
    _check(res, packed, offs)
    sp, so = tpf.encn256v32(_dev32(v), d1=d1, start0=49)
    assert np.array_equal(res[1][: len(packed)], sp.cpu().numpy())
    assert np.array_equal(res[3], so.cpu().numpy().view(np.uint64))


def test_one_block_lists_equal_the_per_block_starts_call():
    rng = np.random.default_rng(9)
    nl = 150
    start0 = rng.integers(0, 1 << 32, size=nl, dtype=np.uint64).astype(np.uint32)
    lists = _lists([256] * nl, True, rng, start0)
    packed, offs, ptr, vals = ref.compose(lists, True, start0)
    assert len(offs) == nl + 1
    res = _run(vals, ptr, nl, True, start0)
    _check(res, packed, offs)
    bp, bo = tpf.enc256v32(_dev32(vals), d1=True, starts=_dev32(start0))
    assert np.array_equal(res[1][: len(packed)], bp.cpu().numpy())
    assert np.array_equal(res[3], bo.cpu().numpy().view(np.uint64))


# ---- round trip, NULL start0, defaults ------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_round_trip(matrix, d1):
    """The encoder's own d_out, d_off, d_list_ptr and d_start0 feed the lists
    decode unchanged and return the input."""
    (packed, offs, ptr, vals), start0 = matrix[(1, d1)]
    values = _values(vals, ptr)
    lp, s0 = _dev64(ptr), _dev32(start0)
    got, got_offs = tpf.encn256v32_lists(values, lp, d1=d1, start0=s0)  # the defaults: sized and trimmed by the binding
    assert got.numel() == len(packed) and np.array_equal(got.cpu().numpy(), packed)
    back = tpf.decn256v32_lists(got, got_offs, lp, d1=d1, start0=s0)
    assert np.array_equal(back.cpu().numpy().view(np.uint32)[int(ptr[0]):], vals)


def test_start0_null_is_zero():
    rng = np.random.default_rng(5)
    lens = [0, 300, 256, 77, 0, 256 * 20 + 9, 1]
    lists = _lists(lens, True, rng)
    packed, offs, ptr, vals = ref.compose(lists, True, None, ptr0=3)
    a = _run(vals, ptr, len(offs) - 1, True, None)
    b = _run(vals, ptr, len(offs) - 1, True, np.zeros(len(lens), np.uint32))
    _check(a, packed, offs)
    _check(b, packed, offs)


# ---- no read outside the lists -------------------------------------------------
@pytest.mark.parametrize("place", ["start", "end"])
def test_input_window_at_the_allocation_edge(place):
    """ptr[0] = 0 and in_values = ptr[-1], the values at the very start / end of
    their allocation, delta-1: a stray in[pos - 1] or a load past the last tail
    would show as different bytes.  Lists that begin with a full block, with a
    tail, and end with either."""
    rng = np.random.default_rng(21)
    for lens in ([256 * 3, 77, 0, 256 * 33 + 255], [5, 256 * 2, 256 * 40], [256], [255]):
        start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
        lists = _lists(lens, True, rng, start0)
        packed, offs, ptr, vals = ref.compose(lists, True, start0, ptr0=0)
        _check(_run(vals, ptr, len(offs) - 1, True, start0, place=place), packed, offs)


# ---- error reporting -------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(13)
    lens = [300, 0, 256 * 2 + 100, 256, 90, 0, 256 * 17]
    start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    return lens, ref.compose(_lists(lens, True, rng, start0), True, start0, ptr0=11), start0


def _untouched(res, nunits):
    before, win, after, got_offs, _ = res
    assert (before == SENT).all() and (win == SENT).all() and (after == SENT).all()
    assert len(got_offs) == nunits + 1 and (got_offs == SENT64).all()


def test_decreasing_list_ptr(small):
    lens, (packed, offs, ptr, vals), start0 = small
    j = 3
    bad = ptr.copy()
    bad[j + 1] = bad[j] - 1
    nunits = len(offs) - 1
    res = _run(vals, ptr, nunits, True, start0, cap=len(packed), call_ptr=bad)
    assert res[4] == nunits + j
    _untouched(res, nunits)


def test_list_ptr_past_in_values(small):
    lens, (packed, offs, ptr, vals), start0 = small
    in_values = int(ptr[4]) - 1  # list 3 (256 values) is the first to end past it
    j = int(np.argmax(ptr[1:] > in_values))
    assert j == 3
    nunits = len(offs) - 1
    res = _run(vals, ptr, nunits, True, start0, cap=len(packed), in_values=in_values)
    assert res[4] == nunits + j
    _untouched(res, nunits)


def test_units_do_not_add_up(small):
    lens, (packed, offs, ptr, vals), start0 = small
    nunits = len(offs) - 2  # one unit short of what list_ptr implies
    res = _run(vals, ptr, nunits, True, start0, cap=len(packed))
    assert res[4] == nunits + len(lens)
    _untouched(res, nunits)


def test_capacity_one_byte_short(small):
    """out_cap = total - 1: nothing is written to d_out, d_off is complete."""
    lens, (packed, offs, ptr, vals), start0 = small
    nunits = len(offs) - 1
    before, win, after, got_offs, err = _run(vals, ptr, nunits, True, start0, cap=len(packed) - 1)
    assert err == nunits + len(lens) + 1
    assert (before == SENT).all() and (win == SENT).all() and (after == SENT).all()
    assert np.array_equal(got_offs, offs)


def test_capacity_exact(small):
    lens, (packed, offs, ptr, vals), start0 = small
    _check(_run(vals, ptr, len(offs) - 1, True, start0, cap=len(packed)), packed, offs)


def test_host_refusals(small):
    lens, (packed, offs, ptr, vals), start0 = small
    L = tpf.lib()
    nunits, nlists = len(offs) - 1, len(lens)
    ws_bytes = int(L.tpf_p4nenc256v32_lists_workspace_size(nunits, nlists))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    values = _values(vals, ptr)
    out = torch.empty(len(packed), dtype=torch.uint8, device=DEV)
    o = torch.full((nunits + 1,), SENT64, dtype=torch.int64, device=DEV)
    lp = _dev64(ptr)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = L.tpf_p4nenc256v32_lists
    rc = f(values.data_ptr(), values.numel(), lp.data_ptr(), nlists, 0, None, out.data_ptr(), out.numel(), o.data_ptr(), nunits,
           ws.data_ptr(), ws_bytes - 1, None, s)
    assert rc == -1 and b"tpf_p4nenc256v32_lists" in L.tpf_last_error() and b"workspace" in L.tpf_last_error()
    rc = f(values.data_ptr(), values.numel(), lp.data_ptr(), nlists, 0, None, out.data_ptr(), out.numel(), None, nunits,
           ws.data_ptr(), ws_bytes, None, s)
    assert rc == -1 and b"tpf_p4nenc256v32_lists" in L.tpf_last_error() and b"null" in L.tpf_last_error()
    # nothing to do: a successful no-op that still reports clean and an empty stream
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    rc = f(values.data_ptr(), values.numel(), lp.data_ptr(), 0, 0, None, out.data_ptr(), out.numel(), o.data_ptr(), nunits,
           ws.data_ptr(), ws_bytes, err.data_ptr(), s)
    assert rc == 0 and int(err.item()) == CLEAN and int(o[0].item()) == 0


def test_all_lists_empty():
    """nunits == 0 with every list empty: d_off[0] = 0, clean."""
    ptr = np.full(6, 4, dtype=np.uint64)
    before, win, after, got_offs, err = _run(np.zeros(0, np.uint32), ptr, 0, True, np.zeros(5, np.uint32), cap=16)
    assert err == CLEAN and got_offs.tolist() == [0]
    assert (before == SENT).all() and (win == SENT).all() and (after == SENT).all()
