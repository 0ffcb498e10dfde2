"""The tie families of tests/p4_ties.py without a device: the plain-Python cost
model against the oracle's p4Bits32 / p4Bits64 and against the mode of the
oracle's bytes, the census of the decision boundaries per case, the wrong
variants of the decision that the families tell from the right one, the
shortfall of the older inputs that made the families necessary, and the
oracle's bytes against the reference library where it is built."""
import collections
import ctypes

import numpy as np
import pytest

import datagen
import h64_inputs
import oracle_lib as orc
import p4_modes
import p4_ties as pt
import ref_lib
import v32_inputs
import v64_inputs

FULL_WIDTH = pt.FULL_WIDTH32 + [("128v64", 128), ("256v64", 256), ("64", 256), ("64", 127)]


def _p4bits(values, W):
    """(b, bx) of the oracle's p4Bits32 / p4Bits64."""
    L = orc.lib()
    v = np.ascontiguousarray(values, dtype=np.uint32 if W == 32 else np.uint64)
    bx = ctypes.c_uint(0)
    f, tp = (L.orc_p4bits32, orc.u32p) if W == 32 else (L.orc_p4bits64, orc.u64p)
    b = f(orc.ptr(v, tp), len(v), ctypes.byref(bx))
    return int(b), int(bx.value)


def _older_units(fmt, n):
    """The gaps of the mixed-mode units the suite already has at (fmt, n), with the oracle's stream of them."""
    if fmt == "64":
        gaps = h64_inputs.h64_values(np.random.default_rng([64100, n]), 300, n)
        packed, off = orc.enc64_batch(gaps)
        return gaps, packed, off
    c = (v32_inputs.v32_case if pt.WBITS[fmt] == 32 else v64_inputs.v64_case)(fmt, n, False, nu=300)
    return c.gaps, c.packed, c.off


def _check_stream(fmt, n, gaps, packed, off, what):
    """pt.choose equals the oracle's p4Bits on every block, and the header and mode of the oracle's bytes"""
    W, bn = pt.WBITS[fmt], pt.block_n(fmt, n)
    for i in range(len(gaps)):
        p = int(off[i])
        for k in range(n // bn):
            vals = gaps[i, k * bn: (k + 1) * bn]
            b, bx, raw = pt.choose(vals, W)
            assert (b, bx) == _p4bits(vals, W), (what, i, k)
            hdr, pbx, p = pt.parsed_header(packed, p, bn, W, pt.BASE_N[fmt])
            assert hdr == pt.header_of(b, bx, raw, W), (what, i, k, hdr, (b, bx, raw))
            assert pbx is None or pbx == bx, (what, i, k)
        assert p == int(off[i + 1]), (what, i)


@pytest.mark.parametrize("fmt,n", pt.CASES)
def test_restatement_equals_the_oracle(fmt, n):
    """cost_table's (b, bx) is orc_p4bits32 / orc_p4bits64's and its raw / compressed choice is the one in the oracle's
    bytes, on every block of the family and of the older mixed-mode units at the same (fmt, n); a unit's recorded
    histogram, flex count and classes are those of its values."""
    c = pt.tie_case(fmt, n, False)
    W, bn = c.W, pt.block_n(fmt, n)
    assert 0 < c.nu <= pt.MAX_UNITS
    _check_stream(fmt, n, c.gaps, c.packed, c.off, "family")
    seen = collections.defaultdict(set)
    for i, hist, high, vals, hdr, _ in c.blocks():
        assert np.bincount(pt.np_widths(vals), minlength=W + 1).tolist() == hist
        t = pt.cost_table(hist, bn, W)
        assert hdr == pt.header_of(t.b, t.bx, pt.is_raw(t, high), W), (i, hdr)
        if t.kind == "vb":
            assert sum(pt.vb_len(int(v) >> t.b0, W) for v in vals if int(v).bit_length() > t.b0) == pt.vb_bytes(t, high)
        seen[i] |= pt.classes(t, high)
    assert all(seen[i] == c.classes[i] for i in range(c.nu))
    _check_stream(fmt, n, *_older_units(fmt, n), "older units")


@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("fmt,n", pt.CASES)
def test_census(fmt, n, d1):
    """every class that is not exempt at (W, block n) in at least QUOTA units; with d1 the same gaps as one chained
    list that wraps the range, so the same classes"""
    c = pt.tie_case(fmt, n, d1)
    need = pt.required_classes(fmt, n)
    if (fmt, n) in pt.FULL_WIDTH32:
        assert need == pt.all_classes(32)
    if c.W == 64:
        assert need == pt.all_classes(64)
    short = {k: c.counts[k] for k in need if c.counts[k] < pt.QUOTA}
    assert not short, (fmt, n, short)
    if d1:
        assert c.classes == pt.tie_case(fmt, n, False).classes
        x = np.concatenate([[c.start0], c.vals.ravel()]).astype(object)
        assert any(int(x[k + 1]) < int(x[k]) for k in range(len(x) - 1))  # the list wraps
    # shuffled: a run of 16 units mixes classes
    runs = [frozenset().union(*c.classes[k: k + 16]) for k in range(0, c.nu - 15, 16)]
    assert min(len(r) for r in runs) >= 4, sorted(len(r) for r in runs)[:3]


def _kills(c, rule):
    """the units on which the mutant `rule` decides otherwise than the reference"""
    bn, out = pt.block_n(c.fmt, c.n), set()
    for i in range(c.nu):
        for hist, high in zip(c.hists[i], c.highs[i]):
            if pt.decision(hist, bn, c.W, high, rule) != pt.decision(hist, bn, c.W, high):
                out.add(i)
    return out


@pytest.mark.parametrize("fmt,n", pt.CASES)
def test_mutants_are_told_apart(fmt, n):
    """every wrong variant of the decision changes (b, bx, raw) on at least QUOTA units of a full-width case and on
    at least one of every case where its class is not exempt"""
    c = pt.tie_case(fmt, n, False)
    ex = pt.exempt(fmt, n)
    for rule in pt.MUTANTS:
        k = len(_kills(c, rule))
        if (fmt, n) in FULL_WIDTH:
            assert k >= pt.QUOTA, (fmt, n, rule, k)
        elif not all(cl in ex for cl in pt.MUTANT_CLASS[rule]):
            assert k >= 1, (fmt, n, rule, k)


def test_older_inputs_fall_short():
    """Why the families exist: on the hot-path case of test_v32_vs_oracle and on datagen.c2_blocks (widths 1..32, 0 and
    10 % exceptions) no block has two widths at the minimum cost, so the mutants of the tie order pass there."""
    older = {"v32_case": v32_inputs.v32_case("256v32", 256, False).gaps,
             "c2_blocks": np.concatenate([datagen.c2_blocks(60, bw, exc, seed=exc + 3) for bw in range(1, 33) for exc in (0, 10)])}
    for name, blocks in older.items():
        counts, kills = collections.Counter(), collections.Counter()
        for vals in blocks:
            if len(set(vals.tolist())) == 1:
                continue
            hist = np.bincount(pt.np_widths(vals), minlength=33).tolist()
            counts.update(pt.classes(pt.cost_table(hist, 256, 32)))  # high = 0: the raw-escape classes are not counted
            ref = pt.decision(hist, 256, 32, 0)
            kills.update(m for m in ("lowest_b", "kind_over_order") if pt.decision(hist, 256, 32, 0, m) != ref)
        print(name, len(blocks), dict(counts), dict(kills))
        for cl in ("multi_b_bitmap", "multi_b_vb", "multi_b_mixed_hi_bitmap", "multi_b_mixed_hi_vb"):
            assert counts[cl] < pt.QUOTA, (name, cl, counts[cl])
        assert kills["lowest_b"] < pt.QUOTA and kills["kind_over_order"] == 0, (name, dict(kills))


def test_exemptions_hold():
    """The arithmetic of p4_ties.EXEMPT: only the 32-bit cases of 9 values have any; the raw escape needs 11
    exceptions; and a seeded directed search of vbyte winners at n = 9 finds no two exceptions on either side of an
    estimator step (the module records the full enumeration)."""
    assert set(pt.EXEMPT) == {(32, 9)}
    assert min(xn for xn in range(1, 64) if 4 * xn - 32 >= xn) == 11  # sumlen >= xn and sumlen + 32 >= 4 xn
    assert not pt.vbyte_can_win(32, 9, (19, 20)) and not pt.vbyte_can_win(32, 9, (25, 26))
    rng = np.random.default_rng(99)
    vb = 0
    for _ in range(4000):
        b, o = int(rng.integers(0, 25)), int(rng.choice(pt.EST[:2]))
        if b + o + 1 > 32:
            continue
        cnt = [0] * 33
        cnt[b + o] += 1
        cnt[b + o + 1] += 1
        for w in rng.integers(0, 33, size=int(rng.integers(0, 7))):
            cnt[int(w)] += 1
        cnt[b] += 9 - sum(cnt)
        t = pt.cost_table(cnt, 9, 32)
        vb += t.kind == "vb"
        assert not pt.classes(t) & {"est_7", "est_15", "est_19", "est_25"}, cnt
    assert vb >= 100


@pytest.mark.skipif(not ref_lib.available(), reason="reference library not built")
@pytest.mark.parametrize("d1", [False, True])
@pytest.mark.parametrize("fmt,n", pt.CASES)
def test_oracle_equals_the_reference(fmt, n, d1):
    """The oracle's bytes of every unit of the family are the reference's scalar build's.  In a unit shorter than an
    interleaved layout the reference packs base slots past n from its uninitialised stack (tests/test_oracle_golden.py
    has the rule: a delta-1 plain block, and a 64-bit bitmap or vbyte block with b >= 1); there the base payload is
    left out and every other byte -- header, bx / xn, bitmap, patch bits, vbyte stream, positions -- is compared."""
    L = ref_lib.lib()
    name = "tpref_s_p4" + ("d1" if d1 else "") + "enc" + fmt
    if not hasattr(L, name):
        pytest.skip("the reference build lacks " + name)
    f = getattr(L, name)
    c = pt.tie_case(fmt, n, d1)
    tp = ref_lib.u32p if c.W == 32 else ref_lib.u64p
    short = pt.BASE_N[fmt] is not None and n < c.units.shape[1]
    for i in range(c.nu):
        src = np.zeros(256 + 64, dtype=c.units.dtype)
        src[: c.units.shape[1]] = c.units[i]
        out = np.zeros(n * 10 + 4096, dtype=np.uint8)
        end = f(src.ctypes.data_as(tp), n, out.ctypes.data_as(ref_lib.u8p), *([int(c.starts[i])] if d1 else []))
        got = out[: end - out.ctypes.data].copy()
        want = c.packed[int(c.off[i]): int(c.off[i + 1])].copy()
        if short and len(got) == len(want) and not np.array_equal(got, want):
            lo, hi = _unpinned_base(c, want, d1)
            got[lo:hi] = 0
            want[lo:hi] = 0
        assert np.array_equal(got, want), (fmt, n, d1, c.names([i]))


def _unpinned_base(c, enc, d1):
    """the base payload [lo, hi) of a short unit's block where the reference's rule leaves it unpinned, else (0, 0)"""
    if c.W == 32:
        mode, _, end = p4_modes.parse32(enc, 0, c.n, pt.BASE_N[c.fmt])
        return (1, end) if d1 and mode in ("plain", "plain32") else (0, 0)
    blk = p4_modes.parse64(enc, 0, c.n, 128)
    hit = (blk.mode in ("bitmap", "vb_raw", "vb_comp") and blk.b >= 1) or (d1 and blk.mode in ("plain", "plain63"))
    return blk.base if hit else (0, 0)
