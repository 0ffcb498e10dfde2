"""The census and the reference of the tail families (tests/lists_tails.py),
without a device: every tail unit of every stream form holds the mode it was
chosen for at its count, the oracle's composition of every list is the
reference's chained stream byte for byte (where oracle/_ref was built), and a
decode with a count or a start off by one gives other values than the ones the
GPU tests expect."""
import numpy as np
import pytest

import lists_tails as lt
import oracle_lib as orc
import ref_lib
from lists_index import SENT

FORMS = [("wide", False), ("wide", True), ("ascending", True)]


def test_unreached_names_only_the_smallest_compressed_vbyte_counts():
    assert all(f in lt.FAMILIES and m == "vb_comp" and 26 <= c <= 29 for f, c, m in lt.UNREACHED), lt.UNREACHED
    assert len(set(lt.UNREACHED)) == len(lt.UNREACHED)
    assert lt.R >= 3 and all(lt.floor(f, c, m) == 1 for f, c, m in lt.UNREACHED)
    for name in lt.FAMILIES:
        for cnt in lt.COUNTS:
            need = lt.required_modes(name, cnt)
            drop = set(lt.vi.required_modes(cnt)) - set(need)
            assert drop <= ({"const32", "plain32"} if name == "ascending" else set()), (name, cnt, drop)


@pytest.mark.parametrize("name,d1", FORMS)
def test_census(name, d1):
    fam = lt.family(name)
    s = fam.form(d1)
    assert s.nunits == len(s.offs) - 1 == int(s.base[-1]) and int(s.offs[-1]) == len(s.packed)
    seen = lt.census(fam, s.packed, s.offs, s.base)
    least = lt.check_floor(fam, seen)
    print(f"{name} d1={d1}: {fam.nlists} lists, {int(fam.lens.sum())} values, {s.nunits} units, "
          f"{len(seen)} (count, mode) groups, the smallest holds {least}")
    # the shape of the index: empty lists at the start, in the middle and at the end, the rest shuffled
    empty = np.nonzero(fam.lens == 0)[0]
    assert empty[0] == 0 and empty[-1] == fam.nlists - 1 and any(fam.nlists // 3 < j < 2 * fam.nlists // 3 for j in empty)
    assert set(fam.lens[fam.front] - fam.cnt[fam.front]) == {256} and (fam.lens[~fam.front] == fam.cnt[~fam.front]).all()
    wave = fam.cnt[64:128]
    assert len(set(wave.tolist())) > 32 and len({fam.mode[j] for j in range(64, 128)}) >= 5  # a run of 64 items mixes counts and modes


def test_ascending_ascends_and_wide_wraps():
    asc, wide = lt.family("ascending"), lt.family("wide")
    assert asc.index().ascends()
    assert int(asc.start0.max()) < 1 << 31 and max(int(g.max()) for g in asc.gaps if len(g)) < 1 << lt.CAP_BITS
    assert (1 << 31) + 511 * (1 << lt.CAP_BITS) < 1 << 32
    wraps = [j for j, (v, s) in enumerate(zip(wide.index().lists, wide.start0))
             if len(v) and (np.diff(np.concatenate([[s], v]).astype(np.int64)) < 0).any()]
    assert len(wraps) > 1000
    assert any(wide.front[j] for j in wraps) and any(not wide.front[j] for j in wraps)


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name,d1", FORMS)
def test_oracle_composition_is_the_reference_stream(name, d1):
    """Every list of the family, tail-only or behind a full block: the
    oracle's bytes are what a reference caller writes with p4(D1)Enc256v32 and
    p4(D1)Enc32 -- the horizontal tail at every count 1..255 and every mode.
    Every byte is compared: no tail's last base byte depends on anything but
    its values."""
    fam = lt.family(name)
    s = fam.form(d1)
    lists = fam.values(d1)
    compared = 0
    for j in range(fam.nlists):
        got = s.packed[int(s.offs[s.base[j]]): int(s.offs[s.base[j + 1]])]
        want = ref_lib.encn256v32_stream(lists[j], d1=d1, start0=int(fam.start0[j]) if d1 else 0)
        assert bytes(got) == want, (name, d1, j, int(fam.cnt[j]), fam.mode[j], bool(fam.front[j]))
        compared += 1
    print(f"{name} d1={d1}: {compared} lists compared with the reference")
    assert compared == fam.nlists


@pytest.mark.parametrize("name,d1", FORMS)
def test_a_wrong_count_or_start_changes_the_values(name, d1):
    """What a kernel with a count or a start off by one would write into cnt
    sentinel-guarded slots differs from the expected values at every tail, so
    the GPU comparisons would see it."""
    fam = lt.family(name)
    s = fam.form(d1)
    lists = fam.values(d1)
    for j, u in fam.tail_unit(s.base):
        cnt = int(fam.cnt[j])
        enc = bytes(s.packed[int(s.offs[u]): int(s.offs[u + 1])]) + bytes(16)
        start = fam.tail_start(j) if d1 else 0
        want = np.concatenate([lists[j][len(lists[j]) - cnt:], [SENT]]).astype(np.uint32)
        got, end = orc.decode("32", enc, cnt, d1=d1, start=start)
        assert np.array_equal(got, want[:cnt]) and end == len(enc) - 16, (name, j, cnt)
        for n in (cnt - 1, cnt + 1):
            if n == 0:
                continue
            wrong = want.copy()
            wrong[:cnt] = SENT
            wrong[:n] = orc.decode("32", enc, n, d1=d1, start=start)[0]
            assert not np.array_equal(wrong, want), (name, j, cnt, n, fam.mode[j])
        if d1:
            for st in (start - 1, start + 1):
                assert (orc.decode("32", enc, cnt, d1=True, start=st & 0xFFFFFFFF)[0] != want[:cnt]).all(), (name, j, cnt)
