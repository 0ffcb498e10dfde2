"""CPU checks behind the scale tests of the lists kernels
(tests/test_gpu_lists_scale.py): the launch caps the binding restates equal
the ones in the sources, the many-lists construction of tests/lists_scale.py
equals the oracle's composition list by list, and its whole-request
statements of the definitions equal the per-query ones the small GPU tests
use."""
import os
import re

import numpy as np
import pytest

import lists_index as li
import lists_ref as ref
import lists_scale as sc

tpf = pytest.importorskip("turbopfor_amd")

CSRC = os.path.join(tpf.PKG_DIR, "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(name, text):
    m = re.findall(r"constexpr\s+(?:uint32_t|int)\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert len(m) == 1, name
    return int(m[0])


# ---- the caps ------------------------------------------------------------------------------------
def test_binding_caps_equal_the_sources(monkeypatch):
    assert tpf.LISTS_MIN_W == _const("kListsMinW", _src("p4_lists_dev.h"))
    assert tpf.LISTS_IX_RUN == _const("kIxRun", _src("p4_lists_intersect.hip"))
    assert tpf.LISTS_GA_RUN == _const("kGaRun", _src("p4_lists_gather.hip"))
    assert tpf.LISTS_RUN_DEFAULT == _const("kRunDefault", _src("p4_dec_run.h"))
    # flat_grid: workgroups of 256 threads, capped per CU
    host = _src("p4_lists_host.h")
    body = host[host.index("inline uint32_t flat_grid("):]
    body = body[: body.index("}") + 1]
    assert "(items + 255u) / 256u" in body
    assert [int(x) for x in re.findall(r"grid_cap\(s,\s*(\d+)\)", body)] == [tpf.LISTS_FLAT_WG_PER_CU]
    assert "grid_cap" not in host.replace(body, "")  # the one place the flat cap is set
    # the item decodes: kListsMinW workgroups per CU, 4 waves of kIxRun / kGaRun items each
    for name, run in (("p4_lists_intersect.hip", "kIxRun"), ("p4_lists_gather.hip", "kGaRun")):
        text = _src(name)
        assert len(re.findall(r"grid_cap\(s,\s*dev::kListsMinW\)", text)) == 1, name
        assert len(re.findall(r"static_cast<uint64_t>\(gridDim\.x\) \* 4u \* kRun;", text)) == 1, name
        assert len(re.findall(r"k_(?:ix|ga)_dec<(?:D1, )?dev::" + run + ",", text)) == 1, name
    # the CU count is the attribute torch reports as multi_processor_count
    assert "hipDeviceAttributeMultiprocessorCount" in _src("capi.cpp")
    monkeypatch.setattr(tpf, "_lists_cus", lambda device: 256)
    assert tpf.lists_flat_cap("cuda:0") == 524288
    assert tpf.lists_item_cap("cuda:0") == 28672 == tpf.lists_item_cap("cuda:0", tpf.LISTS_GA_RUN)


# ---- the construction ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    rng = np.random.default_rng(5)
    kinds = sc.Kinds(rng)
    kind_of = kinds.choose(rng, 2000, big=0.02)
    return kinds, kind_of, sc.ScaleIndex(kinds, kind_of, ptr0=37)


def test_kinds_hold_the_lengths_the_issue_names(built):
    kinds, kind_of, ix = built
    assert 24 <= len(kinds.lens) <= 48
    assert set(sc.BIG_LENS) <= set(kinds.lens.tolist()) and {0, 1, 2, 3} <= set(kinds.lens.tolist())
    assert set(kind_of.tolist()) == set(range(len(kinds.lens)))  # every kind occurs in the index
    assert (ix.lens <= 3).mean() > 0.9


def test_construction_equals_the_composition(built):
    kinds, kind_of, ix = built
    lists = [kinds.values[k] for k in kind_of]
    want = li.Index(None, np.random.default_rng(0), ptr0=37, start0=kinds.start0[kind_of], lists=lists)
    assert want.ascends()
    packed, offs = ix.stream(True)
    assert np.array_equal(packed, want.packed) and packed.dtype == np.uint8
    assert np.array_equal(offs, want.offs) and offs.dtype == np.uint64
    assert np.array_equal(ix.ptr, want.ptr) and ix.ptr.dtype == np.uint64 and ix.ptr[0] == 37
    assert np.array_equal(ix.base, want.base) and ix.base.dtype == np.uint32
    assert np.array_equal(ix.start0, want.start0) and ix.start0.dtype == np.uint32
    assert np.array_equal(ix.vals, want.vals) and ix.vals.dtype == np.uint32
    assert np.array_equal(ix.table, want.table) and ix.table.dtype == np.uint32
    assert (ix.nlists, ix.nunits, ix.lens.tolist()) == (want.nlists, want.nunits, want.lens)
    # the plain form of the same values: same pointers and directory, its own bytes and offsets
    ppacked, poffs, pptr, pvals = ref.compose(lists, False, None, ptr0=37)
    packed, offs = ix.stream(False)
    assert np.array_equal(packed, ppacked) and np.array_equal(offs, poffs)
    assert np.array_equal(ix.ptr, pptr) and np.array_equal(ix.vals, pvals)
    assert not np.array_equal(ppacked, want.packed)


# ---- the whole-request statements against the per-query ones ------------------------------------------
@pytest.fixture(scope="module")
def small_ix():
    rng = np.random.default_rng(17)
    ix = li.Index([ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))], rng, ptr0=37, start_bits=31)
    assert ix.ascends()
    return ix


def _probe(ix, rng, nq):
    qlist = rng.integers(0, ix.nlists, size=nq)
    segs = []
    for j in qlist:
        v = ix.lists[j]
        m = int(rng.integers(0, 6))
        take = v[rng.integers(0, len(v), size=m)] if len(v) else np.zeros(0, np.uint32)
        near = (take.astype(np.int64) + rng.integers(-2, 3, size=len(take))).clip(0, 0xFFFFFFFF).astype(np.uint32)
        segs.append(np.sort(np.concatenate([take[: m // 2], near[m // 2:], rng.integers(0, 1 << 32, size=1, dtype=np.uint64).astype(np.uint32)])))
    return qlist, segs


def test_want_hits_equals_the_per_query_statement(small_ix):
    ix = small_ix
    rng = np.random.default_rng(3)
    qlist, segs = _probe(ix, rng, 300)
    ptr0 = 3
    probe = np.concatenate([np.full(ptr0, ix.vals[0], np.uint32)] + segs + [np.full(5, ix.vals[0], np.uint32)])
    pp = ptr0 + np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    want = li.want_hits(ix, list(zip(qlist.tolist(), segs)), ptr0)
    got = sc.want_hits(ix, qlist, pp, probe)
    assert len(want[0]) > 200
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # the unit a probe value lands in, against a search over the list's own slice of the table
    ql = np.repeat(qlist, np.diff(pp))
    units = sc.probe_units(ix, ql, probe[pp[0]: pp[-1]])
    for j, v, u in zip(ql[:400], probe[pp[0]:], units):
        ua, ub = int(ix.base[j]), int(ix.base[j + 1])
        ge = np.nonzero(ix.table[ua:ub] >= v)[0]
        assert u == (ua + int(ge[0]) if len(ge) else -1)
    heads = sc.item_heads(ql, units)
    assert 0 < len(heads) < len(ql) and units[heads].min() >= 0


def test_want_range_equals_the_per_query_statement(small_ix):
    import test_gpu_lists_units as units_tests  # its _want_range is the statement of the definition

    ix = small_ix
    rng = np.random.default_rng(4)
    q = []
    for _ in range(600):
        j = int(rng.integers(0, ix.nlists))
        n = ix.lens[j]
        c = int(ix.lists[j][int(rng.integers(0, n))]) if n else int(rng.integers(0, 1 << 32))
        lo = c + int(rng.integers(-3, 4)) - int(rng.choice([0, 1, 3000, 1 << 21]))
        hi = c + int(rng.integers(-3, 4)) + int(rng.choice([-5, 0, 1, 3000, 1 << 21]))
        q.append((j, min(max(lo, 0), 0xFFFFFFFF), min(max(hi, 0), 0xFFFFFFFF)))
    q += [(j, 0, 0xFFFFFFFF) for j in range(ix.nlists)] + [(j, 0xFFFFFFFF, 0xFFFFFFFF) for j in range(ix.nlists)]
    q = np.asarray(q, dtype=np.int64)
    want = np.array([units_tests._want_range(ix, *x) for x in q.tolist()], dtype=np.uint32)
    uf, uc = sc.want_range(ix, q[:, 0], q[:, 1], q[:, 2])
    assert np.array_equal(uf, want[:, 0]) and np.array_equal(uc, want[:, 1])
    assert (uc == 0).sum() > 20 and (uc > 1).sum() > 20


def test_want_select_units_and_gather_equal_slices(small_ix):
    ix = small_ix
    rng = np.random.default_rng(6)
    sel = rng.integers(0, ix.nlists, size=60)
    vals, out_ptr = sc.want_select(ix, sel)
    assert np.array_equal(vals, np.concatenate([ix.lists[j] for j in sel]))
    assert np.array_equal(out_ptr, np.concatenate([[0], np.cumsum([ix.lens[j] for j in sel])]))
    uc = np.array([int(rng.integers(0, ix.units(j) + 1)) for j in sel])
    uf = np.array([int(rng.integers(0, ix.units(j) - c + 1)) for j, c in zip(sel, uc)])
    vals, out_ptr = sc.want_units(ix, sel, uf, uc)
    parts = [ix.lists[j][256 * f: min(256 * (f + c), ix.lens[j])] for j, f, c in zip(sel, uf, uc)]
    assert np.array_equal(vals, np.concatenate(parts)) and np.array_equal(np.diff(out_ptr), [len(p) for p in parts])
    assert any(c and f + c == ix.units(j) and ix.lens[j] % 256 for j, f, c in zip(sel, uf, uc))  # a range that reaches a tail
    tails = sc.tail_units(ix)
    assert tails.sum() == sum(1 for n in ix.lens if n % 256) and tails[int(ix.base[ix.of_len(5)])]
    ql = [j for j in sel if ix.lens[j]]
    pos = [rng.integers(0, ix.lens[j], size=4) for j in ql]
    pp = 2 + 4 * np.arange(len(ql) + 1)
    flat = np.concatenate([[0, 0]] + pos + [[0]])
    assert np.array_equal(sc.want_gather(ix.ptr, ix.vals, ql, pp, flat), np.concatenate([ix.lists[j][p] for j, p in zip(ql, pos)]))
