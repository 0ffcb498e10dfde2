"""Every encoder route on the tie families of tests/p4_ties.py: blocks that sit
on the decision boundaries of p4Bits32 / p4Bits64 -- equal costs at two widths,
psz == vsz, the plain block against the best patch, the raw escape of vbEnc and
the steps of the vbyte estimator -- where the device's closed form
(plan_block256, plan_block_g) must keep the reference's serial tie order.
Every comparison is bytes and offsets against the oracle's stream of the family
(tests/test_p4_ties_cpu.py holds that to the cost model and to the reference);
a mismatch names the classes of the units it is in.  Every encode is decoded by
the matching device decoder and compared with the input values."""
import ctypes
import functools

import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
import lists_remove_ref as rr
import p4_ties as pt
import v32_inputs
import v64_inputs
from lists_index import CLEAN, DEV

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
FILL8 = 0xA5


def to_dev(arr, W):
    if W == 32:
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(DEV)


def _wrong_sizes(offs, exp_off):
    """the units whose size differs (every offset after the first of them differs too)"""
    offs, exp_off = np.asarray(offs).astype(np.int64), np.asarray(exp_off).astype(np.int64)
    if len(offs) != len(exp_off):
        return [0]
    return np.nonzero(np.diff(offs) != np.diff(exp_off))[0]


def _same(c, packed, offs, what, exp=None):
    """offsets and bytes equal the oracle's; a failure names the classes of the first units that differ"""
    exp_packed, exp_off = (c.packed, c.off) if exp is None else exp
    offs = np.asarray(offs).astype(np.uint64)
    if not np.array_equal(offs, exp_off):
        raise AssertionError((what, "offsets", c.names(_wrong_sizes(offs, exp_off))))
    packed = np.asarray(packed)
    assert len(packed) == len(exp_packed), what
    bad = np.nonzero(packed != exp_packed)[0]
    assert len(bad) == 0, (what, "bytes", c.names(c.units_of_bytes(bad)))


def _decoded(c, what):
    """the device decoder of the family's format returns the values from the oracle's stream"""
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = tpf.dec_batch(c.fmt, torch.from_numpy(c.packed).to(DEV), torch.from_numpy(c.off.astype(np.int64)).to(DEV), c.nu, c.n,
                        starts=None if c.starts is None else to_dev(c.starts, c.W), err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN, (what, int(err.item()))
    got = out.cpu().numpy().view(c.vals.dtype).reshape(c.nu, -1)[:, :c.n]
    bad = np.nonzero((got != c.vals).any(axis=1))[0]
    assert len(bad) == 0, (what, "decode", c.names(bad))


# ---- 256v32 at n = 256: the hot path, all routes ---------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
def test_256v32_batch_entry(d1):
    """tpf.enc256v32 -- plan_block256 -- plain, as one chained delta-1 list from start0 and with per-block starts;
    the buffer past the stream keeps its fill byte"""
    c = pt.tie_case("256v32", 256, d1)
    vals = to_dev(c.units, 32)
    cap = int(tpf.lib().tpf_p4enc256v32_bound(c.nu))
    kws = [dict(d1=True, start0=c.start0), dict(d1=True, starts=to_dev(c.starts, 32))] if d1 else [dict()]
    for kw in kws:
        out = torch.full((cap,), FILL8, dtype=torch.uint8, device=DEV)
        _, offs = tpf.enc256v32(vals, out=out, **kw)
        got, total = out.cpu().numpy(), int(offs[-1].item())
        what = "enc256v32 " + ",".join(kw)
        _same(c, got[:total], offs.cpu().numpy(), what)
        assert (got[total:] == FILL8).all(), what
    _decoded(c, "256v32")


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("mode", [3, 4, 5])
def test_256v32_forced_routes(mode, d1):
    """tpfm_enc256v32: 3 = the two-pass encoder, 4 = the slot encoder with the fused planner, 5 = without"""
    c = pt.tie_case("256v32", 256, d1)
    cap = int(tpf.lib().tpf_p4enc256v32_bound(c.nu))
    out = torch.full((cap,), FILL8, dtype=torch.uint8, device=DEV)
    offs = tpf.enc256v32_path(mode, to_dev(c.units, 32), out, d1=d1, start0=c.start0 if d1 else 0)
    got, total = out.cpu().numpy(), int(offs[-1].item())
    _same(c, got[:total], offs.cpu().numpy(), f"route {mode} d1={d1}")
    assert (got[total:total + 4096] == FILL8).all()


# ---- every other case, through tpf.enc_batch -------------------------------------------------------
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("fmt,n", [x for x in pt.CASES if x != ("256v32", 256)])
def test_enc_batch(fmt, n, d1):
    """plan_block_g of every format at the smallest shapes each instance runs at; a short interleaved unit has non-zero
    slots past n, which a plain-mode block without delta-1 carries (oracle_lib.encode's pad) and nothing else reads"""
    c = pt.tie_case(fmt, n, d1)
    mod = v32_inputs if c.W == 32 else v64_inputs
    units, exp = c.units, None
    if fmt in mod.WIDTH and n < mod.WIDTH[fmt]:
        units = mod.padded(c.vals, fmt, fill=0xDEADBEEF if c.W == 32 else 0xDEADBEEFDEADBEEF)
        if not d1:
            exp = mod.oracle_stream(fmt, units, n)
            assert np.array_equal(exp[1], c.off) and not np.array_equal(exp[0], c.packed)  # tie blocks carry the padding
    kws = [dict(d1=True, start0=c.start0), dict(d1=True, starts=to_dev(c.starts, c.W))] if d1 else [dict()]
    for kw in kws:
        packed, offs = tpf.enc_batch(fmt, to_dev(units.ravel(), c.W), c.nu, n, **kw)
        _same(c, packed.cpu().numpy(), offs.cpu().numpy(), f"{fmt} n={n} " + ",".join(kw), exp)
    _decoded(c, f"{fmt} n={n} d1={d1}")


# ---- the lists encoder -----------------------------------------------------------------------------
class TieLists:
    """One index of the 32-bit families: a list is up to two full blocks of the (256v32, 256) family and a tail of the
    (32, 127), (32, 33) or (32, 9) family, or full blocks alone; every unit of the four families is in one list.
    gaps[j], label[j] (the units of list j as (family n, unit)), start0."""

    def __init__(self):
        rng = np.random.default_rng(9300)
        full = pt.tie_case("256v32", 256, False)
        tails = [(n, i) for n in (127, 33, 9) for i in range(pt.tie_case("32", n, False).nu)]
        tails = [tails[i] for i in rng.permutation(len(tails))]
        self.gaps, self.label, at = [], [], 0
        for k, (n, i) in enumerate(tails):
            take = min((0, 1, 2)[k % 3], full.nu - at)
            lab = [(256, at + x) for x in range(take)] + [(n, i)]
            at += take
            self.label.append(lab)
        while at < full.nu:  # the rest of the full blocks: lists without a tail
            take = min(5, full.nu - at)
            self.label.append([(256, at + x) for x in range(take)])
            at += take
        fam = {256: full, **{n: pt.tie_case("32", n, False) for n in (127, 33, 9)}}
        self.fam = fam
        self.gaps = [np.concatenate([fam[n].gaps[i] for n, i in lab]) for lab in self.label]
        self.nlists = len(self.gaps)
        self.start0 = rng.integers(0, 1 << 32, size=self.nlists, dtype=np.uint64).astype(np.uint32)
        self.unit_label = [x for lab in self.label for x in lab]

    def lists(self, d1, gaps=None):
        gaps = self.gaps if gaps is None else gaps
        if not d1:
            return gaps
        return [((np.cumsum(g.astype(np.uint64) + np.uint64(1)) + np.uint64(s)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                for g, s in zip(gaps, self.start0)]

    def names(self, units):
        return [(n, i, sorted(self.fam[n].classes[i])) for n, i in (self.unit_label[int(u)] for u in list(units)[:5])]


@functools.lru_cache(maxsize=None)
def _tie_lists():
    return TieLists()


@pytest.mark.parametrize("d1", [False, True])
def test_lists_encoder(d1):
    """tpf_p4nenc256v32_lists: full blocks through plan_block256, tails through plan_block_g; then decn256v32_lists"""
    tl = _tie_lists()
    lists = tl.lists(d1)
    packed, offs, ptr, vals = ref.compose(lists, d1, tl.start0)
    nunits = len(offs) - 1
    assert nunits == len(tl.unit_label)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_ptr = li.dev64(torch, ptr)
    d_st = li.dev32(torch, tl.start0) if d1 else None
    cap = tpf.lists_enc_bound(len(vals), tl.nlists)
    out = torch.full((cap,), FILL8, dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(nunits + 1, dtype=torch.int64, device=DEV)
    tpf.encn256v32_lists(li.dev32(torch, vals), d_ptr, d1=d1, start0=d_st, nunits=nunits, out=out, offsets=d_offs, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    got, goff = out.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    if not np.array_equal(goff, offs):
        raise AssertionError(("offsets", tl.names(_wrong_sizes(goff, offs))))
    bad = np.nonzero(got[:len(packed)] != packed)[0]
    assert len(bad) == 0, ("bytes", tl.names(np.unique(np.searchsorted(offs, bad.astype(np.uint64), side="right") - 1)))
    assert (got[len(packed):] == FILL8).all()
    dec = tpf.decn256v32_lists(out[:len(packed) + 64], d_offs, d_ptr, d1=d1, start0=d_st, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), vals)


# ---- append and remove re-encoding a tail ----------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Index:
    """the oracle's composition of lists, with the directory and the skip table of its definition"""

    def __init__(self, lists, d1, start0):
        self.packed, self.offs, self.ptr, self.vals = ref.compose(lists, d1, start0)
        self.base = np.asarray(ref.units_loop(self.ptr)[1], dtype=np.uint32)
        self.nunits = len(self.offs) - 1
        self.table = rr.table(lists)

    def inputs(self, d1, start0):
        return (li.dev8(torch, self.packed), li.dev64(torch, self.offs), li.dev64(torch, self.ptr), li.dev32(torch, self.base),
                li.dev32(torch, start0) if d1 else None, li.dev32(torch, np.concatenate([self.table, [0]])) if d1 else None)


def _tail_lists(d1):
    """the (32, 127) family as lists of one tail unit each: (case, the lists, start0)"""
    c = pt.tie_case("32", 127, False)
    start0 = np.random.default_rng(9400).integers(0, 1 << 32, size=c.nu, dtype=np.uint64).astype(np.uint32)
    gaps = list(c.gaps)
    if not d1:
        return c, gaps, start0
    return c, [((np.cumsum(g.astype(np.uint64) + np.uint64(1)) + np.uint64(s)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
               for g, s in zip(gaps, start0)], start0


def _outputs(out_cap, units_cap, nlists):
    return dict(out=torch.full((out_cap,), FILL8, dtype=torch.uint8, device=DEV), off=torch.zeros(units_cap + 1, dtype=torch.int64, device=DEV),
                lptr=torch.zeros(nlists + 1, dtype=torch.int64, device=DEV), lunit=torch.zeros(nlists + 1, dtype=torch.int32, device=DEV),
                ulast=torch.zeros(max(units_cap, 1), dtype=torch.int32, device=DEV))


def _same_index(c, new, g, d1, start0, what):
    """bytes, offsets and directory are the oracle's composition of the full units -- the tie blocks -- and the stream
    decodes to them"""
    off = g["off"].cpu().numpy().astype(np.uint64)[:new.nunits + 1]
    if not np.array_equal(off, new.offs):
        raise AssertionError((what, "offsets", c.names(_wrong_sizes(off, new.offs))))
    got = g["out"].cpu().numpy()
    bad = np.nonzero(got[:len(new.packed)] != new.packed)[0]
    assert len(bad) == 0, (what, "bytes", c.names(np.unique(np.searchsorted(new.offs, bad.astype(np.uint64), side="right") - 1)))
    assert np.array_equal(g["lptr"].cpu().numpy().astype(np.uint64), new.ptr), what
    assert np.array_equal(g["lunit"].cpu().numpy().view(np.uint32), new.base), what
    if d1:
        assert np.array_equal(g["ulast"].cpu().numpy().view(np.uint32)[:new.nunits], new.table), what
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    dec = tpf.decn256v32_lists(g["out"][:len(new.packed) + 64], g["off"][:new.nunits + 1], g["lptr"], d1=d1,
                               start0=li.dev32(torch, start0) if d1 else None, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), new.vals), what


@pytest.mark.parametrize("d1", [False, True])
def test_append_reencodes_tie_tails(d1):
    """every list of the old index holds a tie unit of the (32, 127) family without its last value; the append adds it,
    so the re-encoded tails are the tie blocks"""
    c, lists, start0 = _tail_lists(d1)
    old = _Index([v[:-1] for v in lists], d1, start0)
    new = _Index(lists, d1, start0)
    add = np.concatenate([np.array([v[-1] for v in lists], dtype=np.uint32), np.full(7, 0xDEADBEEF, np.uint32)])
    aptr = np.arange(c.nu + 1, dtype=np.uint64)
    L = tpf.lib()
    out_cap = int(L.tpf_lists_append_bound(len(old.packed), c.nu, len(add)))
    units_cap = int(L.tpf_lists_append_units_bound(old.nunits, c.nu, len(add)))
    g = _outputs(out_cap, units_cap, c.nu)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_in, d_off, d_ptr, d_base, d_st, d_tab = old.inputs(d1, start0)
    d_add, d_aptr = li.dev32(torch, add), li.dev64(torch, aptr)
    ws = torch.empty(max(int(L.tpf_lists_append_workspace_size(old.nunits, c.nu, len(add))), 1), dtype=torch.uint8, device=DEV)
    rc = L.tpf_lists_append(_p(d_in), len(old.packed), _p(d_off), old.nunits, _p(d_ptr), _p(d_base), c.nu, int(d1), _p(d_st),
                            _p(d_tab), _p(d_add), len(add), _p(d_aptr), c.nu, _p(g["out"]), out_cap, _p(g["off"]), units_cap,
                            _p(g["lptr"]), _p(g["lunit"]), _p(g["ulast"]), _p(ws), ws.numel(), _p(err),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tpf_last_error()
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    _same_index(c, new, g, d1, start0, "append")


@pytest.mark.parametrize("d1", [False, True])
def test_remove_reencodes_tie_tails(d1):
    """every list of the old index holds a tie unit of the (32, 127) family with one extra value at a seeded position;
    the remove deletes it"""
    c, lists, start0 = _tail_lists(d1)
    rng = np.random.default_rng(9500)
    at = rng.integers(0, 128, size=c.nu)
    at[:3] = (0, 127, 64)
    extra = rng.integers(0, 1 << 32, size=c.nu, dtype=np.uint64).astype(np.uint32)
    olds = [np.insert(v, int(p), x) for v, p, x in zip(lists, at, extra)]
    rc_ = rr.Case(olds, {j: np.array([int(p)], dtype=np.uint32) for j, p in enumerate(at)}, d1, start0, ptr0=0, pos0=0)
    new = _Index(lists, d1, start0)
    assert np.array_equal(rc_.xpacked, new.packed) and np.array_equal(rc_.xoffs, new.offs)
    L = tpf.lib()
    stage = rc_.targeted
    out_cap = int(L.tpf_lists_remove_bound(len(rc_.packed), rc_.nq, stage))
    g = _outputs(out_cap, rc_.nunits, c.nu)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    d_in, d_off, d_ptr, d_base = li.dev8(torch, rc_.packed), li.dev64(torch, rc_.offs), li.dev64(torch, rc_.ptr), li.dev32(torch, rc_.base)
    d_st = li.dev32(torch, start0) if d1 else None
    d_tab = li.dev32(torch, np.concatenate([rc_.table, [0]])) if d1 else None
    d_pos, d_pptr, d_ql = li.dev32(torch, rc_.pos), li.dev64(torch, rc_.pptr), li.dev32(torch, np.concatenate([rc_.qlist, [0]]))
    ws = torch.empty(max(int(L.tpf_lists_remove_workspace_size(rc_.nunits, c.nu, rc_.nq, len(rc_.pos), stage)), 1), dtype=torch.uint8,
                     device=DEV)
    rc = L.tpf_lists_remove(_p(d_in), len(rc_.packed), _p(d_off), rc_.nunits, _p(d_ptr), _p(d_base), c.nu, int(d1), _p(d_st), _p(d_tab),
                            _p(d_pos), len(rc_.pos), _p(d_pptr), _p(d_ql), rc_.nq, stage, _p(g["out"]), out_cap, _p(g["off"]), rc_.nunits,
                            _p(g["lptr"]), _p(g["lunit"]), _p(g["ulast"]), _p(ws), ws.numel(), _p(err),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tpf_last_error()
    torch.cuda.synchronize()
    assert int(err.item()) == CLEAN
    _same_index(c, new, g, d1, start0, "remove")


# ---- the per-block mirrors -------------------------------------------------------------------------
def _sample(c, limit=120):
    """at most `limit` units that hold every non-exempt class of the case: the first unit of each class, then the
    units in order"""
    first = {}
    for i, cl in enumerate(c.classes):
        for k in cl:
            first.setdefault(k, i)
    need = pt.required_classes(c.fmt, c.n)
    assert set(need) <= set(first), set(need) - set(first)
    picked = list(dict.fromkeys([first[k] for k in need] + list(range(c.nu))))[:limit]
    assert {first[k] for k in need} <= set(picked)
    return picked


@pytest.fixture(params=[0, 1, 2], ids=["server", "launch", "server-hostmail"])
def perblock_mode(request):
    L = tpf.lib()
    L.tpf_perblock_mode.restype = ctypes.c_int
    L.tpf_perblock_mode.argtypes = [ctypes.c_int]
    prev = L.tpf_perblock_mode(request.param)
    yield request.param
    L.tpf_perblock_mode(prev)


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("fmt,n", [("256v32", 256), ("128v32", 128), ("32", 127), ("128v64", 128), ("256v64", 256), ("64", 127)])
def test_per_block_mirrors(fmt, n, d1, perblock_mode):
    """tpf_p4Enc* / tpf_p4D1Enc* of all six families in every per-block design: bytes, end pointer and decode"""
    L = tpf.lib()
    c = pt.tie_case(fmt, n, d1)
    vt = ctypes.c_uint32 if c.W == 32 else ctypes.c_uint64
    enc_f = getattr(L, f"tpf_p4{'D1' if d1 else ''}Enc{fmt}")
    dec_f = getattr(L, f"tpf_p4{'D1' if d1 else ''}Dec{fmt}")
    for f in (enc_f, dec_f):
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p] + ([vt] if d1 else [])
        f.restype = ctypes.c_void_p
    for i in _sample(c):
        exp = c.packed[int(c.off[i]): int(c.off[i + 1])]
        st = [int(c.starts[i])] if d1 else []
        src = np.zeros(256 + 64, dtype=c.vals.dtype)
        src[:n] = c.vals[i]
        out = np.zeros(len(exp) + 4096, dtype=np.uint8)
        end = enc_f(src.ctypes.data, n, out.ctypes.data, *st)
        assert end is not None, L.tpf_last_error()
        assert end - out.ctypes.data == len(exp), (fmt, n, c.names([i]))
        assert np.array_equal(out[: len(exp)], exp), (fmt, n, c.names([i]))
        enc = np.concatenate([exp, np.zeros(64, dtype=np.uint8)])
        dec = np.zeros(256 + 64, dtype=c.vals.dtype)
        end = dec_f(enc.ctypes.data, n, dec.ctypes.data, *st)
        assert end is not None, L.tpf_last_error()
        assert end - enc.ctypes.data == len(exp), (fmt, n, c.names([i]))
        assert np.array_equal(dec[:n], c.vals[i]), (fmt, n, c.names([i]))
