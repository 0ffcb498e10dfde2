"""The inputs of tests/test_gpu_host_streams.py (tests/host_inputs.py),
checked on the oracle alone: the GPU tests must not pass for lack of a
discriminating case -- a chained list whose wrong start at a cut encodes to
the same bytes, padding slots that no block carries, a pair of nothing but
constant units."""
import numpy as np
import pytest

import host_inputs as hi
import oracle_lib

CASES = [(f, n, m) for f, n in hi.PAIRS for m in hi.MODES]
IDS = [f"{hi.FMT_NAME[f]}-n{n}-{m}" for f, n, m in CASES]


def _unit(c, i):
    return bytes(c.packed[int(c.off[i]): int(c.off[i + 1])])


def test_matrix_is_the_one_the_issue_sets():
    assert hi.PAIRS == [(0, 1), (0, 127), (0, 256), (1, 1), (1, 100), (1, 128), (2, 1), (2, 200), (2, 256),
                        (3, 1), (3, 127), (3, 256), (4, 1), (4, 100), (4, 128), (5, 256)]
    assert hi.NBLOCKS == (1, 5, 6, 15, 16, 36) and hi.MAX_NB == 36 and hi.CHUNK_UNITS == 5 and hi.ONE_UNIT_NB == 7
    assert hi.cuts(36) == [5, 10, 12, 15, 17, 18, 20, 22, 23, 24, 25, 28, 29, 30, 33, 34, 35]
    assert hi.cuts(2) == [1] and hi.cuts(6) == [2, 3, 4, 5] and hi.cuts(1) == []
    assert set(hi.ALL_CUTS) >= {1, 2, 3, 4, 5, 6, 8, 10, 15, 18, 35}


@pytest.mark.parametrize("fmt,n,mode", CASES, ids=IDS)
def test_expected_stream_decodes_to_the_input(fmt, n, mode):
    c = hi.case(fmt, n, mode)
    assert c.units.shape == (hi.MAX_NB, c.stride) and c.units.dtype == c.dtype
    assert c.chunk_bytes == 5 * c.stride * c.es
    for i in range(hi.MAX_NB):
        enc = _unit(c, i)
        got, used = oracle_lib.decode(c.name, enc, n, d1=bool(c.d1), start=int(c.true_starts[i]) if c.d1 else 0)
        assert used == len(enc), (c.id, i)
        np.testing.assert_array_equal(got, c.units[i, :n], err_msg=f"{c.id} unit {i}")
    if mode == "chain":
        # one list: every unit starts where the one before it ends, and it wraps the range
        assert c.h_starts is None and int(c.true_starts[0]) == c.start0
        np.testing.assert_array_equal(c.true_starts[1:], c.units[:-1, n - 1])
        flat = np.concatenate([[c.start0], c.units[:, :n].ravel()]).astype(c.dtype)
        assert (flat[1:] < flat[:-1]).any(), c.id
        assert c.start0 >= (1 << (8 * c.es)) - 4096
    if mode == "starts":
        # a start per unit that is NOT the previous unit's last value: a call that chained would differ
        assert c.h_starts is not None
        assert (c.h_starts[1:] != c.units[:-1, n - 1]).all(), c.id
        assert int(c.h_starts[0]) + 1 >= 1 << (8 * c.es)


@pytest.mark.parametrize("fmt,n", [(f, n) for f, n in hi.PAIRS if n < hi.width(f, n)],
                         ids=lambda v: str(v))
def test_a_wrong_start_at_a_cut_changes_the_unit_after_it(fmt, n):
    """Chained short units: at every cut the GPU tests use, the unit after the
    cut composed with slot stride-1 of the previous unit, or with the value at
    (c - 1) * n + n - 1 as if the stride were n, differs from the expectation.
    (At c = 1 the second address IS the previous unit's value n - 1: a stride
    of n cannot be told from the true one there, at any other cut it can.)"""
    c = hi.case(fmt, n, "chain")
    flat = c.units.ravel()
    for d1mode in ("chain", "starts"):
        cc = hi.case(fmt, n, d1mode)
        assert (cc.units[:, n:] != cc.units[:, n - 1:n]).all(), cc.id  # the padding differs from value n - 1 in every unit
    for cut in hi.ALL_CUTS:
        exp = _unit(c, cut)
        true = int(c.true_starts[cut])
        assert bytes(hi.oracle_unit(fmt, c.units[cut], n, true)) == exp
        wrong = [int(c.units[cut - 1, c.stride - 1])]
        if cut > 1:
            wrong.append(int(flat[(cut - 1) * n + n - 1]))
        for w in wrong:
            assert w != true, (c.id, cut)
            assert bytes(hi.oracle_unit(fmt, c.units[cut], n, w)) != exp, (c.id, cut, w)
        # ... and so does the call's own start0 carried past the cut
        assert bytes(hi.oracle_unit(fmt, c.units[cut], n, c.start0)) != exp, (c.id, cut)


@pytest.mark.parametrize("fmt,n", [(f, n) for f, n in hi.PAIRS if n < hi.width(f, n)],
                         ids=lambda v: str(v))
def test_plain_short_units_carry_their_padding(fmt, n):
    """At least a quarter of the units are plain-mode blocks whose bytes
    change when the slots n .. stride-1 are zeroed, so an upload of n values
    per unit (or of a zeroed stride) shows.  n = 1 is the exception the format
    makes: a one-value block is all zero or constant (v32_inputs.required_modes,
    v64_inputs.required_modes), never plain, and no block carries padding;
    there the padding must change nothing."""
    c = hi.case(fmt, n, "plain")
    assert (c.units[:, n:] != 0).all()
    z = c.units.copy()
    z[:, n:] = 0
    p0, o0 = hi.oracle_units(fmt, z, n)
    changed = sum(bytes(p0[int(o0[i]): int(o0[i + 1])]) != _unit(c, i) for i in range(hi.MAX_NB))
    if n == 1:
        assert changed == 0
    else:
        assert changed >= hi.MAX_NB // 4, (c.id, changed)
        # in every chunk and shard the GPU tests cut, so that each upload is held to it
        first_chunks = [any(bytes(p0[int(o0[i]): int(o0[i + 1])]) != _unit(c, i) for i in range(a, min(a + 5, hi.MAX_NB)))
                        for a in range(0, hi.MAX_NB, 5)]
        assert all(first_chunks), (c.id, first_chunks)


@pytest.mark.parametrize("fmt,n", hi.PAIRS, ids=lambda v: str(v))
def test_every_pair_has_a_unit_that_is_not_trivial(fmt, n):
    """n > 1: a unit that is neither constant nor all zero, in every mode's
    gaps.  A one-value unit is always constant; there: a non-zero one, and
    units that differ from each other."""
    for mode in hi.MODES:
        g = hi.case(fmt, n, mode).gaps
        if n > 1:
            assert ((g != g[:, :1]).any(axis=1)).any(), (fmt, n, mode)
        else:
            assert (g != 0).any() and len(np.unique(g)) > 1, (fmt, n, mode)


def test_prefixes_and_sub_streams_are_slices():
    c = hi.case(1, 100, "chain")
    p, o = c.stream(11, first=5)
    assert int(o[0]) == 0 and len(o) == 12 and len(p) == int(o[-1])
    assert bytes(p[: int(o[1])]) == _unit(c, 5) and c.start0_arg(5) == int(c.units[4, 99])
    p, o = c.stream(6)
    assert bytes(p) == b"".join(_unit(c, i) for i in range(6))


@pytest.mark.parametrize("fmt,n", hi.CORRUPT_PAIRS, ids=lambda v: str(v))
def test_corrupt_offset_cases_keep_offsets_rising(fmt, n):
    c = hi.corrupt_case(fmt, n)
    assert hi.CORRUPT_AT == (3, 8, 18, 35)
    for b in hi.CORRUPT_AT:
        off = c.off.copy()
        off[b] += 1
        assert (np.diff(off.astype(np.int64)) >= 2).all() or (np.diff(off.astype(np.int64))[[b - 1, b]] >= 2).all()
        assert (np.diff(off.astype(np.int64)) >= 0).all()
