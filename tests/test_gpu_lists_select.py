"""GPU parity of the read side of a resident index (include/turbopfor_gpu.h
tpf_lists_unit_base, tpf_p4ndec256v32_lists_select): a selection of the lists
of a resident stream, any order, repeats allowed, decoded in one call into a
dense output.  The streams are the oracle's composition (tests/lists_ref.py),
the expected decode is the original values of the selected lists, bit-exact,
plain and delta-1 (random start0 per list of the index)."""
import numpy as np
import pytest

import lists_ref as ref

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5A5A5A5
SENT64 = 0x5A5A5A5A5A5A5A5A
CLEAN = -1  # UINT64_MAX read back as int64
PADV = 64   # sentinel values before d_out


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


class Index:
    """A composed stream with its directory: what a caller keeps resident."""

    def __init__(self, lens, d1, rng, ptr0=0, start0=None):
        self.d1 = d1
        self.start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32) if start0 is None else start0
        if d1:
            self.lists = [ref.d1_values(n, int(self.start0[j]), rng) for j, n in enumerate(lens)]
        else:
            self.lists = [ref.plain_values(n, rng) for n in lens]
        self.packed, self.offs, self.ptr, self.vals = ref.compose(self.lists, d1, self.start0, ptr0=ptr0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.nlists, self.nunits = len(lens), len(self.offs) - 1
        self.lens = list(lens)

    def of_len(self, n):
        return self.lens.index(n)


def _run(ix, sel, cap=None, shift=0, start0="own", packed=None, offs=None, ptr=None, base=None, nunits=None):
    """Decode selection `sel` of `ix` into cap values (default: what it holds)
    of a sentinel-filled buffer, d_out one value past a 16-byte boundary.
    -> (values before d_out, the cap values, values after, out_ptr, err)"""
    sel = np.asarray(sel, dtype=np.uint32)
    total = int(sum(len(ix.lists[j]) for j in sel if j < ix.nlists))
    cap = total if cap is None else cap
    big = torch.full((cap + 2 * PADV + 8,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    s = PADV + ((4 - big.data_ptr() - 4 * PADV) % 16) // 4
    out = big[s: s + cap]
    assert out.data_ptr() % 16 == 4
    out_ptr = torch.full((len(sel) + 1,), SENT64, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = None
    if ix.d1 and start0 is not None:
        st = _dev32(ix.start0 if isinstance(start0, str) else start0)
    o = ix.offs if offs is None else offs
    if nunits is not None:
        o = o[: nunits + 1]
    tpf.decn256v32_lists_select(_dev8(ix.packed if packed is None else packed, shift, 64), _dev64(o),
                                _dev64(ix.ptr if ptr is None else ptr), _dev32(ix.base if base is None else base), _dev32(sel),
                                d1=ix.d1, start0=st, out=out, out_ptr=out_ptr, err=err)
    got = big.cpu().numpy().view(np.uint32)
    return got[:s], got[s: s + cap], got[s + cap:], out_ptr.cpu().numpy(), int(err.item())


def _check(ix, sel, res):
    before, got, after, out_ptr, err = res
    assert err == CLEAN
    want_ptr = np.concatenate([[0], np.cumsum([len(ix.lists[j]) for j in sel])]).astype(np.int64)
    assert np.array_equal(out_ptr, want_ptr)
    for k, j in enumerate(sel):
        assert np.array_equal(got[want_ptr[k]: want_ptr[k + 1]], ix.lists[j]), (k, j)
    assert (before == SENT).all() and (after == SENT).all() and (got[want_ptr[-1]:] == SENT).all()


def _untouched(res, out_ptr_too=True):
    before, got, after, out_ptr, _ = res
    assert (before == SENT).all() and (got == SENT).all() and (after == SENT).all()
    if out_ptr_too:
        assert (out_ptr == SENT64).all()


@pytest.fixture(scope="module")
def matrix():
    """(order seed, d1) -> the shape-matrix index (17 lists, about 92k values), built once."""
    built = {}
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
        for d1 in (False, True):
            built[(seed, d1)] = Index(lens, d1, rng, ptr0=37)
    return built


@pytest.fixture(scope="module")
def small():
    return {d1: Index([300, 0, 256 * 2 + 100, 256, 90, 0, 256 * 17], d1, np.random.default_rng(13), ptr0=11) for d1 in (False, True)}


# ---- 1. the directory --------------------------------------------------------
def _unit_base(ptr):
    n = len(ptr) - 1
    out = torch.full((n + 1,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.lists_unit_base(_dev64(ptr), out=out, err=err)
    return out.cpu().numpy().view(np.uint32), int(err.item())


def test_unit_base(matrix):
    rng = np.random.default_rng(3)
    tails = [0, 0] + list(rng.integers(1, 256, size=110)) + [0] * 70 + list(rng.integers(1, 256, size=110)) + [0]
    for ptr in (matrix[(1, False)].ptr, np.concatenate([[5], 5 + np.cumsum(tails)]).astype(np.uint64), np.array([9], np.uint64)):
        got, err = _unit_base(ptr)
        assert err == CLEAN and got.tolist() == ref.units_loop(ptr)[1]
    bad = matrix[(1, False)].ptr.copy()
    j = 6
    bad[j + 1] = bad[j] - 1
    got, err = _unit_base(bad)
    assert err == j and (got == SENT).all()


# ---- 2. everything, in order -----------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_all_lists_in_order(matrix, seed, d1):
    ix = matrix[(seed, d1)]
    sel = list(range(ix.nlists))
    res = _run(ix, sel)
    _check(ix, sel, res)
    assert np.array_equal(res[1], ix.vals)
    assert np.array_equal(res[3].astype(np.uint64), ix.ptr - ix.ptr[0])
    # the one place where the library's own full decode is the statement: the two calls agree bit for bit
    full = tpf.decn256v32_lists(_dev8(ix.packed), _dev64(ix.offs), _dev64(ix.ptr), d1=d1, start0=_dev32(ix.start0))
    assert np.array_equal(full.cpu().numpy().view(np.uint32)[int(ix.ptr[0]):], res[1])


# ---- 3. scattered, repeated, reversed -------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("kind", ["reversed", "permuted", "twice"])
def test_scattered_selection(matrix, kind, d1):
    ix = matrix[(1, d1)]
    rng = np.random.default_rng(21)
    if kind == "reversed":
        sel = list(range(ix.nlists))[::-1]
    elif kind == "permuted":
        sel = [int(j) for j in rng.permutation(ix.nlists)]
    else:
        z = ix.of_len(0)
        body = [int(j) for j in rng.permutation(np.repeat(np.arange(ix.nlists), 2))]
        sel = [z] * 5 + body[:17] + [z] * 5 + body[17:] + [z] * 5
    _check(ix, sel, _run(ix, sel))


# ---- 4. run boundaries in the virtual sequence --------------------------------------
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("pre", [False, True])
def test_heads_around_run_boundaries(matrix, pre, d1):
    """The list after one of 15, 16, 16+, 63+, 64, 64+ units has its head on,
    one before and one after the first unit of a 16-unit decode run and of a
    64-unit workgroup; a 1-unit list in front moves each by one."""
    ix = matrix[(1, d1)]
    for n in (256 * 15, 256 * 16, 256 * 16 + 1, 256 * 63 + 255, 256 * 64, 256 * 64 + 1):
        sel = ([ix.of_len(256)] if pre else []) + [ix.of_len(n), ix.of_len(513), ix.of_len(n)]
        _check(ix, sel, _run(ix, sel))


@pytest.mark.parametrize("d1", [False, True])
def test_long_list_alone_and_between_tails(matrix, d1):
    ix = matrix[(1, d1)]
    big = ix.of_len(256 * 130 + 77)
    for sel in ([big], [ix.of_len(5), big, ix.of_len(255)]):
        _check(ix, sel, _run(ix, sel))


# ---- 5. many heads per run --------------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_many_heads_per_run(d1):
    """300 tail-only lists (and one empty list, the 301st, to select): 200 of
    them in random order, 70 empty selections in a row in the middle -- every
    decode run of the virtual sequence holds 16 heads."""
    rng = np.random.default_rng(7)
    ix = Index(list(rng.integers(1, 256, size=300)) + [0], d1, rng, ptr0=1)
    pick = [int(j) for j in rng.permutation(300)[:200]]
    sel = pick[:100] + [300] * 70 + pick[100:]
    _check(ix, sel, _run(ix, sel))


# ---- 6. start0 == NULL ----------------------------------------------------------------
def test_start0_null_is_zero():
    rng = np.random.default_rng(5)
    ix = Index([0, 300, 256, 77, 0, 256 * 20 + 9, 1], True, rng, ptr0=3, start0=np.zeros(7, np.uint32))
    sel = [5, 1, 3, 0, 2, 6, 5]
    a = _run(ix, sel, start0=None)
    b = _run(ix, sel, start0=np.zeros(ix.nlists, np.uint32))
    _check(ix, sel, a)
    assert b[4] == CLEAN and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


# ---- 7. only the selection is read ----------------------------------------------------
def _damage(ix, lists, packed, offs):
    for j in lists:
        a, b = int(ix.base[j]), int(ix.base[j + 1])
        if b - a >= 2:
            packed[int(ix.offs[a]): int(ix.offs[b])] = 0xFF
            offs[a + 1: b] = len(ix.packed) + 12345


@pytest.mark.parametrize("d1", [False, True])
def test_only_the_selection_is_read(matrix, d1):
    ix = matrix[(1, d1)]
    rng = np.random.default_rng(31)
    sel = [int(j) for j in rng.permutation(ix.nlists)[: ix.nlists // 3]] + [ix.of_len(256 * 17 + 3)]
    others = [j for j in range(ix.nlists) if j not in sel]
    assert sum(int(ix.base[j + 1] - ix.base[j]) >= 2 for j in others) >= 3
    packed, offs, start0 = ix.packed.copy(), ix.offs.copy(), ix.start0.copy()
    _damage(ix, others, packed, offs)
    start0[others] = rng.integers(0, 1 << 32, size=len(others), dtype=np.uint64).astype(np.uint32)
    _check(ix, sel, _run(ix, sel, packed=packed, offs=offs, start0=start0))
    # the same damage to a selected list is found: its first unit's end offset is checked, never followed
    j = ix.of_len(256 * 17 + 3)
    _damage(ix, [j], packed, offs)
    assert _run(ix, sel, packed=packed, offs=offs, start0=start0)[4] == int(ix.base[j])


# ---- 8. capacity -----------------------------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_capacity(matrix, d1):
    ix = matrix[(2, d1)]
    sel = [ix.of_len(255), ix.of_len(256 * 16 + 1), ix.of_len(0), ix.of_len(1), ix.of_len(256), ix.of_len(255), ix.of_len(511)]
    want_ptr = np.concatenate([[0], np.cumsum([len(ix.lists[j]) for j in sel])]).astype(np.int64)
    res = _run(ix, sel, cap=int(want_ptr[-1]) - 1)
    assert res[4] == ix.nunits + len(sel)
    _untouched(res, out_ptr_too=False)
    assert np.array_equal(res[3], want_ptr)
    _check(ix, sel, _run(ix, sel, cap=int(want_ptr[-1])))


# ---- 9. refused selections ----------------------------------------------------------------
SEL8 = [6, 0, 1, 2, 4, 5, 3, 0]


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("what", ["nlists", "ffffffff", "list_unit"])
def test_refused_selection_first_wins(small, what, d1):
    ix = small[d1]
    sel, base = list(SEL8), ix.base.copy()
    if what == "nlists":
        sel[3], sel[6] = ix.nlists, 0xFFFFFFFF
    elif what == "ffffffff":
        sel[3], sel[6] = 0xFFFFFFFF, ix.nlists
    else:
        base[sel[3] + 1] += 1  # list 2 one unit too long, and list 3 (k = 6) one too short
    res = _run(ix, sel, base=base, cap=int(ix.ptr[-1] - ix.ptr[0]) * 2)
    assert res[4] == ix.nunits + 3
    _untouched(res)


def test_refused_list_unit_past_nunits(small):
    ix = small[False]
    res = _run(ix, SEL8, nunits=ix.nunits - 1, cap=int(ix.ptr[-1]))  # list 6 (k = 0) ends at unit nunits
    assert res[4] == (ix.nunits - 1) + 0
    _untouched(res)


def test_refused_decreasing_list_ptr(small):
    ix = small[False]
    ptr = ix.ptr.copy()
    j = 4  # selected at k = 4; list 5, whose start moves with it, comes later
    ptr[j + 1] = ptr[j] - 1
    res = _run(ix, SEL8, ptr=ptr, cap=int(ix.ptr[-1]))
    assert res[4] == ix.nunits + SEL8.index(j)
    _untouched(res)


@pytest.mark.parametrize("d1", [False, True])
def test_mistakes_at_unselected_lists_are_not_reported(small, d1):
    ix = small[d1]
    sel = [6, 0, 1, 2, 5, 0]  # neither list 3 nor list 4: entry 4 of the directory and of list_ptr is theirs alone
    ptr, base = ix.ptr.copy(), ix.base.copy()
    ptr[4] = ptr[3] - 1
    base[4] += 7
    _check(ix, sel, _run(ix, sel, ptr=ptr, base=base))


# ---- 10. nsel == 0 ----------------------------------------------------------------------
def test_empty_selection(small):
    before, got, after, out_ptr, err = _run(small[False], [], cap=100)
    assert err == CLEAN and out_ptr.tolist() == [0]
    assert (before == SENT).all() and (got == SENT).all() and (after == SENT).all()


# ---- 11. misaligned stream ----------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 5, 15])
def test_misaligned_stream(matrix, shift):
    ix = matrix[(1, True)]
    sel = [int(j) for j in np.random.default_rng(41).permutation(ix.nlists)]
    _check(ix, sel, _run(ix, sel, shift=shift))
