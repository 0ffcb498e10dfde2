"""GPU parity of the block-range reads of a resident index
(include/turbopfor_gpu.h tpf_lists_unit_last, tpf_lists_range_units,
tpf_p4ndec256v32_lists_units): the skip table of a delta-1 stream, the search
from doc-id ranges to unit ranges, and the decode of unit ranges of selected
lists.  The streams are the oracle's composition (tests/lists_ref.py); the
expected values are slices of the original lists, the expected table and the
expected unit ranges numpy restatements of their definitions -- never the
code under test."""
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
SMALL = [300, 0, 256 * 2 + 100, 256, 90, 0, 256 * 17]


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _dev8(a, shift=0, pad=64):
    """packed bytes on the device, `shift` bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    buf = torch.zeros(len(a) + pad + 32, dtype=torch.uint8, device=DEV)
    s = (shift - buf.data_ptr()) % 16
    view = buf[s: s + len(a) + pad]
    assert view.data_ptr() % 16 == shift % 16
    view[: len(a)] = torch.from_numpy(a).to(DEV)
    return view


def _sentinel32(n):
    """n sentinel values, the first 4 bytes past a 16-byte boundary, inside a
    sentinel-filled buffer -> (whole buffer, start index)"""
    big = torch.full((n + 2 * PADV + 8,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    s = PADV + ((4 - big.data_ptr() - 4 * PADV) % 16) // 4
    assert big[s:].data_ptr() % 16 == 4
    return big, s


class Index:
    """A composed stream with its directory and the skip table its values imply."""

    def __init__(self, lens, d1, rng, ptr0=0, start0=None, start_bits=32, outliers=False, lists=None):
        self.d1 = d1
        nl = len(lens) if lists is None else len(lists)
        self.start0 = rng.integers(0, 1 << start_bits, size=nl, dtype=np.uint64).astype(np.uint32) if start0 is None else start0
        if lists is not None:
            self.lists = lists
        elif d1:
            self.lists = [ref.d1_values(n, int(self.start0[j]), rng, outliers=outliers) for j, n in enumerate(lens)]
        else:
            self.lists = [ref.plain_values(n, rng) for n in lens]
        self.packed, self.offs, self.ptr, self.vals = ref.compose(self.lists, d1, self.start0, ptr0=ptr0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.lens = [len(v) for v in self.lists]
        self.nlists, self.nunits = len(self.lens), len(self.offs) - 1
        # the definition: entry u = the last value of unit i of list j, position min(256 (i + 1), n) - 1
        self.table = np.array([v[min(256 * (i + 1), len(v)) - 1] for v in self.lists for i in range(ref.n_units(len(v)))], dtype=np.uint32)
        assert len(self.table) == self.nunits

    def of_len(self, n):
        return self.lens.index(n)

    def units(self, j):
        return ref.n_units(self.lens[j])

    def slice(self, j, uf, uc):
        return self.lists[j][256 * uf: min(256 * (uf + uc), self.lens[j])]


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
    return {d1: Index(SMALL, d1, np.random.default_rng(13), ptr0=11) for d1 in (False, True)}


@pytest.fixture(scope="module")
def ascending():
    """delta-1 indexes whose lists do not wrap: start0 < 2^31, gaps below 2^14, at most 33,357 values"""
    rng = np.random.default_rng(17)
    lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
    ixs = [Index(lens, True, rng, ptr0=37, start_bits=31), Index(SMALL, True, rng, ptr0=11, start_bits=31)]
    for ix in ixs:
        assert all(int(v[-1]) > int(s) for v, s in zip(ix.lists, ix.start0) if len(v))
    return ixs


# ---- 1. the skip table -----------------------------------------------------------
def _table(ix, shift=0, start0="own", offs=None, ptr=None):
    o = ix.offs if offs is None else offs
    big, s = _sentinel32(len(o) - 1)
    out = big[s: s + len(o) - 1]
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = None if start0 is None else _dev32(ix.start0)
    tpf.lists_unit_last(_dev8(ix.packed, shift), _dev64(o), _dev64(ix.ptr if ptr is None else ptr), start0=st, out=out, err=err)
    got = big.cpu().numpy().view(np.uint32)
    assert (got[:s] == SENT).all() and (got[s + len(o) - 1:] == SENT).all()
    return got[s: s + len(o) - 1], int(err.item())


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("seed", [1, 2])
def test_unit_last(matrix, small, seed, shift):
    for ix in (matrix[(seed, True)], small[True]):
        got, err = _table(ix, shift)
        assert err == CLEAN
        assert np.array_equal(got, ix.table)


def test_unit_last_wrapping_lists():
    rng = np.random.default_rng(11)
    lens = [256 * 20 + 5, 100, 256, 256 * 65, 0, 3]
    start0 = ((1 << 32) - rng.integers(1, 10 ** 6, size=len(lens))).astype(np.uint32)
    ix = Index(lens, True, rng, ptr0=5, start0=start0)
    assert all(int(v[-1]) < int(s) for v, s in zip(ix.lists, start0) if len(v) >= 256)  # wrapped
    got, err = _table(ix)
    assert err == CLEAN and np.array_equal(got, ix.table)


def test_unit_last_start0_null_is_zero():
    rng = np.random.default_rng(5)
    ix = Index([0, 300, 256, 77, 0, 256 * 20 + 9, 1], True, rng, ptr0=3, start0=np.zeros(7, np.uint32))
    got, err = _table(ix, start0=None)
    assert err == CLEAN and np.array_equal(got, ix.table)


def test_unit_last_structure_errors_leave_the_table(small):
    ix = small[True]
    ptr = ix.ptr.copy()
    j = 3
    ptr[j + 1] = ptr[j] - 1
    got, err = _table(ix, ptr=ptr)
    assert err == ix.nunits + j and (got == SENT).all()
    got, err = _table(ix, offs=ix.offs[:-1])  # one unit short of what list_ptr implies
    assert err == (ix.nunits - 1) + ix.nlists and (got == SENT).all()


@pytest.mark.parametrize("tail", [False, True])
def test_unit_last_corrupted_block(small, tail):
    ix = small[True]
    j = 6 if not tail else 2
    u = int(ix.base[j]) + (5 if not tail else ix.units(j) - 1)
    offs = ix.offs.copy()
    offs[u + 1] += 1
    assert _table(ix, offs=offs)[1] == u


# ---- 2. the range search -----------------------------------------------------------
def _want_range(ix, j, lo, hi):
    """numpy restatement of the definition in include/turbopfor_gpu.h"""
    ua, ub = int(ix.base[j]), int(ix.base[j + 1])
    t = ix.table[ua:ub].astype(np.int64)
    ge = np.nonzero(t >= lo)[0]
    if lo > hi or ua == ub or len(ge) == 0:
        return 0, 0
    a = int(ge[0])
    geh = np.nonzero(t >= hi)[0]
    b = int(geh[0]) if len(geh) else ub - ua - 1
    return a, b - a + 1


def _range(ix, q, table=None, base=None):
    q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
    uf = torch.full((len(q),), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    uc = torch.full((len(q),), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.lists_range_units(_dev32(ix.base if base is None else base), _dev32(ix.table if table is None else table), _dev32(q[:, 0]),
                          _dev32(q[:, 1]), _dev32(q[:, 2]), ufirst=uf, ucount=uc, err=err)
    return uf.cpu().numpy().view(np.uint32), uc.cpu().numpy().view(np.uint32), int(err.item())


def _edge_queries(ix):
    q = []
    for j, v in enumerate(ix.lists):
        n = len(v)
        if n == 0:
            q += [(j, 0, 0xFFFFFFFF), (j, 0, 0)]
            continue
        # the first value, a block's last value, the next block's first value, the list's last value
        marks = {int(v[0]), int(v[-1])}
        for i in {0, ref.n_units(n) // 2, ref.n_units(n) - 2}:
            if 0 <= i and 256 * (i + 1) < n:
                marks |= {int(v[256 * (i + 1) - 1]), int(v[256 * (i + 1)])}
        pts = sorted({min(max(m + d, 0), 0xFFFFFFFF) for m in marks for d in (-1, 0, 1)} | {0xFFFFFFFF})
        q += [(j, lo, hi) for lo in pts for hi in pts]  # lo > hi and lo above the list's last value among them
    return q


def test_range_units_edges(ascending):
    for ix in ascending:
        q = _edge_queries(ix)
        assert any(lo > hi for _, lo, hi in q) and any(lo > int(ix.lists[j][-1]) for j, lo, _ in q if ix.lens[j])
        assert any(ix.lens[j] == 0 for j, _, _ in q) and any(0 < ix.lens[j] < 256 for j, _, _ in q)
        uf, uc, err = _range(ix, q)
        assert err == CLEAN
        want = np.array([_want_range(ix, *x) for x in q], dtype=np.uint32)
        assert np.array_equal(uf, want[:, 0]) and np.array_equal(uc, want[:, 1])
        # a superset of the units holding a value in range, by at most one unit at the top end
        for (j, lo, hi), a, c in zip(q, uf, uc):
            v = ix.lists[j].astype(np.int64)
            hit = np.nonzero((v >= lo) & (v <= hi))[0]
            if len(hit):
                assert a == hit[0] // 256 and hit[-1] // 256 <= a + c - 1 <= hit[-1] // 256 + 1


def test_range_units_bad_list_id(ascending):
    ix = ascending[1]
    j = ix.of_len(612)
    lo, hi = int(ix.lists[j][300]), int(ix.lists[j][400])
    q = [(j, lo, hi)] * 12
    q[5] = (ix.nlists, lo, hi)
    q[9] = (0xFFFFFFFF, lo, hi)
    uf, uc, err = _range(ix, q)
    assert err == 5
    for k in range(12):
        assert (uf[k], uc[k]) == ((0, 0) if k in (5, 9) else (1, 1)), k
    # a directory that runs past nunits is refused the same way
    base = ix.base.copy()
    base[j + 1] = ix.nunits + 1
    uf, uc, err = _range(ix, [(0, 0, 5), (j, lo, hi)], base=base)
    assert err == 1 and (uf[1], uc[1]) == (0, 0)


def test_range_units_wrapping_list_stays_inside():
    rng = np.random.default_rng(23)
    ix = Index([256 * 20 + 5, 300], True, rng, start0=np.array([(1 << 32) - 40000, 7], np.uint32))
    assert int(ix.lists[0][-1]) < int(ix.lists[0][0])  # wrapped
    pts = [0, 1, 1000, 1 << 31, (1 << 32) - 40000, (1 << 32) - 2, 0xFFFFFFFF] + [int(x) for x in ix.table[:21:4]]
    q = [(0, lo, hi) for lo in pts for hi in pts]
    uf, uc, err = _range(ix, q)
    assert err == CLEAN
    assert (uf.astype(np.int64) + uc.astype(np.int64) <= ix.units(0)).all()


# ---- 3. the units decode against slices ------------------------------------------------
def _run(ix, sels, cap=None, shift=0, table="own", start0="own", offs=None, base=None, select_too=False):
    """Decode selections [(list, ufirst, ucount)] of `ix` into cap values
    (default: what they hold) of a sentinel-filled buffer, d_out one value past
    a 16-byte boundary.  -> (values before d_out, the cap values, values after,
    out_ptr, err)"""
    sels = np.asarray(sels, dtype=np.int64).reshape(-1, 3)
    total = sum(len(ix.slice(j, uf, uc)) for j, uf, uc in sels if j < ix.nlists and uf + uc <= ix.units(j))
    cap = total if cap is None else cap
    big, s = _sentinel32(cap)
    out = big[s: s + cap]
    out_ptr = torch.full((len(sels) + 1,), SENT64, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = _dev32(ix.start0) if (ix.d1 and start0 is not None) else None
    tb = None
    if ix.d1:
        tb = _dev32(ix.table if isinstance(table, str) else table)
    tpf.decn256v32_lists_units(_dev8(ix.packed, shift), _dev64(ix.offs if offs is None else offs), _dev64(ix.ptr),
                               _dev32(ix.base if base is None else base), _dev32(sels[:, 0]), _dev32(sels[:, 1]), _dev32(sels[:, 2]),
                               d1=ix.d1, start0=st, unit_last=tb, out=out, out_ptr=out_ptr, err=err)
    got = big.cpu().numpy().view(np.uint32)
    return got[:s], got[s: s + cap], got[s + cap:], out_ptr.cpu().numpy(), int(err.item())


def _check(ix, sels, res):
    before, got, after, out_ptr, err = res
    assert err == CLEAN
    want = [ix.slice(j, uf, uc) for j, uf, uc in sels]
    want_ptr = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
    assert np.array_equal(out_ptr, want_ptr)
    for k, w in enumerate(want):
        assert np.array_equal(got[want_ptr[k]: want_ptr[k + 1]], w), (k, sels[k])
    assert (before == SENT).all() and (after == SENT).all() and (got[want_ptr[-1]:] == SENT).all()


def _untouched(res, out_ptr_too=True):
    before, got, after, out_ptr, _ = res
    assert (before == SENT).all() and (got == SENT).all() and (after == SENT).all()
    if out_ptr_too:
        assert (out_ptr == SENT64).all()


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("shift", [0, 5])
def test_named_ranges(matrix, small, shift, d1):
    ix, sm = matrix[(1, d1)], small[d1]
    j612 = sm.of_len(612)
    _check(sm, [(j612, 0, 1), (j612, 1, 1), (j612, 2, 1)], _run(sm, [(j612, 0, 1), (j612, 1, 1), (j612, 2, 1)], shift=shift))
    j17, j64, j5 = ix.of_len(256 * 17 + 3), ix.of_len(256 * 64 + 1), ix.of_len(5)
    for sels in ([(j17, 15, 3)],   # across a 16-unit run, into the tail
                 [(j64, 63, 2)],   # the last full block and a 1-value tail
                 [(j17, 16, 1)],   # the last full block alone of a list that has a tail: no tail is decoded
                 [(j17, 17, 1)],   # the tail alone
                 [(j5, 0, 1)],     # a tail-only list
                 [(j17, 3, 9), (j17, 5, 13), (j17, 3, 9), (j17, 17, 1), (j17, 0, 18)]):  # the same list, overlapping ranges
        _check(ix, sels, _run(ix, sels, shift=shift))


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_whole_lists_equal_the_selective_decode(matrix, seed, d1):
    ix = matrix[(seed, d1)]
    order = [int(j) for j in np.random.default_rng(29).permutation(ix.nlists)]
    sels = [(j, 0, ix.units(j)) for j in order]
    res = _run(ix, sels)
    _check(ix, sels, res)
    out, out_ptr = tpf.decn256v32_lists_select(_dev8(ix.packed), _dev64(ix.offs), _dev64(ix.ptr), _dev32(ix.base), _dev32(order), d1=d1,
                                               start0=_dev32(ix.start0))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), res[1]) and np.array_equal(out_ptr.cpu().numpy(), res[3])


@pytest.mark.parametrize("d1", [False, True])
def test_empty_ranges_anywhere(matrix, d1):
    ix = matrix[(2, d1)]
    a, b, z = ix.of_len(513), ix.of_len(256 * 16 + 1), ix.of_len(0)
    sels = [(a, 1, 0), (z, 0, 0), (a, 0, 2), (b, 16, 0), (b, 17, 0), (a, 3, 0), (b, 14, 3), (z, 0, 0), (a, 2, 1), (b, 0, 0), (b, 5, 0)]
    _check(ix, sels, _run(ix, sels))


@pytest.mark.parametrize("d1", [False, True])
def test_many_selections(matrix, d1):
    """150 selections of 0 to 3 units: the virtual runs of 16 units span many selections, the tails kernel many waves."""
    ix = matrix[(1, d1)]
    rng = np.random.default_rng(43)
    sels = []
    for _ in range(150):
        j = int(rng.integers(0, ix.nlists))
        uc = int(rng.integers(0, min(3, ix.units(j)) + 1))
        sels.append((j, int(rng.integers(0, ix.units(j) - uc + 1)), uc))
    assert sum(1 for j, uf, uc in sels if uc and uf + uc == ix.units(j) and ix.lens[j] % 256) >= 10
    _check(ix, sels, _run(ix, sels))


def test_nsel_zero(small):
    before, got, after, out_ptr, err = _run(small[True], [], cap=100)
    assert err == CLEAN and out_ptr.tolist() == [0]
    assert (before == SENT).all() and (got == SENT).all() and (after == SENT).all()


# ---- 4. blocks of every exception kind ---------------------------------------------------
def test_every_exception_kind():
    rng = np.random.default_rng(10)
    ix = Index([256 * 70 + 130, 5, 256 * 3, 256 * 33 + 1, 0, 200, 256 * 18 + 255], True, rng, ptr0=2, outliers=True)
    kinds = ref.block_kinds(ix.packed, ix.offs, ix.ptr - ix.ptr[0])
    assert kinds["vbyte"] >= 5 and kinds["bitmap"] >= 5 and kinds["plain"] >= 1, kinds
    got, err = _table(ix)
    assert err == CLEAN and np.array_equal(got, ix.table)
    sels = []
    for j in (0, 3, 6, 2, 5):
        for u in rng.permutation(ix.units(j))[:40]:
            sels.append((j, int(u), 1))
    sels = [sels[i] for i in rng.permutation(len(sels))]
    _check(ix, sels, _run(ix, sels))


# ---- 5. refusals ---------------------------------------------------------------------------
SEL8 = [(6, 2, 3), (0, 0, 2), (1, 0, 0), (2, 1, 2), (4, 0, 1), (5, 0, 0), (3, 0, 1), (0, 1, 1)]


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("what", ["nlists", "one_past", "wrap"])
def test_refused_selection(small, what, d1):
    ix = small[d1]
    sels = list(SEL8)
    if what == "nlists":
        sels[3], sels[6] = (ix.nlists, 0, 0), (0xFFFFFFFF, 0, 0)
    elif what == "one_past":
        sels[3], sels[6] = (2, 1, 3), (3, 1, 1)  # units 1..3 of a 3-unit list; unit 1 of a 1-unit list
    else:
        sels[3], sels[6] = (2, 0xFFFFFFFF, 2), (3, 2, 0)  # the sum wraps to 1 in 32 bits
    res = _run(ix, sels, cap=5000)
    assert res[4] == ix.nunits + 3
    _untouched(res)


@pytest.mark.parametrize("d1", [False, True])
def test_capacity_one_short(small, d1):
    ix = small[d1]
    want_ptr = np.concatenate([[0], np.cumsum([len(ix.slice(*s)) for s in SEL8])]).astype(np.int64)
    res = _run(ix, SEL8, cap=int(want_ptr[-1]) - 1)
    assert res[4] == ix.nunits + len(SEL8)
    _untouched(res, out_ptr_too=False)
    assert np.array_equal(res[3], want_ptr)
    _check(ix, SEL8, _run(ix, SEL8, cap=int(want_ptr[-1])))


@pytest.mark.parametrize("d1", [False, True])
def test_corrupted_block_is_reported_only_when_selected(small, d1):
    ix = small[d1]
    u = int(ix.base[6]) + 9  # unit 9 of the 17-unit list: its end offset, the start of unit 10, moves by one
    offs = ix.offs.copy()
    offs[u + 1] += 1
    sels = [(6, 3, 4), (2, 0, 3), (6, 9, 1), (6, 12, 2), (0, 0, 2)]
    assert _run(ix, sels, offs=offs)[4] == u
    sels[2] = (6, 11, 1)  # neither unit 9 nor unit 10 is selected now
    _check(ix, sels, _run(ix, sels, offs=offs))
    # the tail of the 612-value list, selected through its range
    u = int(ix.base[2]) + 2
    offs = ix.offs.copy()
    offs[u + 1] += 1
    assert _run(ix, [(6, 3, 4), (2, 1, 2)], offs=offs)[4] == u
    _check(ix, [(6, 3, 4), (2, 1, 1)], _run(ix, [(6, 3, 4), (2, 1, 1)], offs=offs))


# ---- 6. a wrong table is harmless -------------------------------------------------------------
def test_wrong_table_is_harmless(matrix):
    ix = matrix[(1, True)]
    j17, j5, j513 = ix.of_len(256 * 17 + 3), ix.of_len(5), ix.of_len(513)
    sels = [(j17, 0, 18), (j5, 0, 1), (j513, 1, 2), (j17, 16, 2), (j513, 0, 1)]
    before, got, after, out_ptr, err = _run(ix, sels, table=np.full(ix.nunits, 0xFFFFFFFF, np.uint32))
    assert err == CLEAN
    want = [ix.slice(*s) for s in sels]
    want_ptr = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
    assert np.array_equal(out_ptr, want_ptr)  # the layout does not depend on the table
    assert (before == SENT).all() and (after == SENT).all() and (got[want_ptr[-1]:] == SENT).all()
    # units that start from start0 are exact; the others carry the wrong start: value - true start + 0xFFFFFFFF
    for k, (j, uf, uc) in enumerate(sels):
        g = got[want_ptr[k]: want_ptr[k + 1]]
        for i in range(uc):
            lo, hi = 256 * i, min(256 * (i + 1), len(want[k]))
            if uf + i == 0:
                assert np.array_equal(g[lo:hi], want[k][lo:hi]), (k, i)
            else:
                prev = ix.lists[j][256 * (uf + i) - 1]
                assert np.array_equal(g[lo:hi], want[k][lo:hi] - prev + np.uint32(0xFFFFFFFF)), (k, i)


# ---- 7. composition: range search into the units decode, on the device ------------------------
def test_range_search_feeds_the_decode(ascending):
    ix = ascending[0]
    rng = np.random.default_rng(47)
    table = torch.empty(ix.nunits, dtype=torch.int32, device=DEV)
    packed, offs, ptr, base, st = _dev8(ix.packed), _dev64(ix.offs), _dev64(ix.ptr), _dev32(ix.base), _dev32(ix.start0)
    tpf.lists_unit_last(packed, offs, ptr, start0=st, out=table)
    q = []
    for _ in range(100):
        j = int(rng.integers(0, ix.nlists))
        if ix.lens[j] == 0:
            q.append((j, 5, 1 << 30))
            continue
        c = int(ix.lists[j][int(rng.integers(0, ix.lens[j]))]) + int(rng.integers(-3, 4))
        w = int(rng.choice([0, 1, 3000, 1 << 21]))
        q.append((j, max(c - w, 0), min(c + w, 0xFFFFFFFF)))
    q = np.asarray(q, dtype=np.int64)
    qlist = _dev32(q[:, 0])
    err = torch.zeros(2, dtype=torch.int64, device=DEV)
    uf, uc = tpf.lists_range_units(base, table, qlist, _dev32(q[:, 1]), _dev32(q[:, 2]), err=err[0:1])
    cap = 256 * 600  # a window of 2^22 holds about 512 values of gaps below 2^14: at most 6 units per query
    out = torch.full((cap,), SENT - (1 << 32), dtype=torch.int32, device=DEV)
    out, out_ptr = tpf.decn256v32_lists_units(packed, offs, ptr, base, qlist, uf, uc, d1=True, start0=st, unit_last=table, out=out,
                                              err=err[1:2])
    assert err.tolist() == [CLEAN, CLEAN]
    got, out_ptr = out.cpu().numpy().view(np.uint32), out_ptr.cpu().numpy()
    uf, uc = uf.cpu().numpy().view(np.uint32), uc.cpu().numpy().view(np.uint32)
    assert out_ptr[-1] <= cap and sum(uc) > 0
    for k, (j, lo, hi) in enumerate(q):
        g = got[out_ptr[k]: out_ptr[k + 1]]
        # every output value belongs to the named units ...
        assert np.array_equal(g, ix.slice(j, int(uf[k]), int(uc[k]))), k
        # ... and every list value in [lo, hi] appears in the output
        v = ix.lists[j].astype(np.int64)
        assert np.isin(ix.lists[j][(v >= lo) & (v <= hi)], g).all(), k


# ---- 8. index independence -----------------------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_index_independence(small, d1):
    ix = small[d1]
    rng = np.random.default_rng(53)
    more_len = [int(n) for n in rng.integers(0, 300, size=1000)]
    more_s0 = rng.integers(0, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32)
    more = [ref.d1_values(n, int(s), rng) if d1 else ref.plain_values(n, rng) for n, s in zip(more_len, more_s0)]
    grown = Index(None, d1, rng, ptr0=11, start0=np.concatenate([ix.start0, more_s0]), lists=ix.lists + more)
    a, b = _run(ix, SEL8), _run(grown, SEL8)
    _check(ix, SEL8, a)
    assert b[4] == CLEAN and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
