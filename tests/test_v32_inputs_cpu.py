"""The census conditions of tests/test_gpu_formats32.py, established on the
oracle's bytes alone: which modes and which vbEnc32 marker lengths the seeded
inputs of v32_inputs reach at every n, so that the GPU tests cannot pass by
never reaching a path.  No device."""
import itertools

import numpy as np
import pytest

import oracle_lib
import p4_modes
import v32_inputs


def _decodes(case, packed, off):
    for i in range(case.nu):
        st = int(case.starts[i]) if case.d1 else 0
        got, used = oracle_lib.decode(case.fmt, packed[int(off[i]): int(off[i + 1])].tobytes(), case.n, d1=case.d1, start=st)
        assert used == int(off[i + 1]) - int(off[i]), i
        np.testing.assert_array_equal(got, case.vals[i], err_msg=f"unit {i}")


@pytest.mark.parametrize("fmt,n", v32_inputs.V32_CASES)
@pytest.mark.parametrize("d1", [False, True])
def test_v32_census(fmt, n, d1):
    """1029 units of v32_values reach every mode the encoder can produce at
    n (v32_inputs.required_modes) in at least 10 units, the decode-only bx = 0
    rewrite of the plain blocks included, and from n = 64 every marker length;
    the oracle decodes its own stream and the rewritten one to the inputs."""
    c = v32_inputs.v32_case(fmt, n, d1)
    need = v32_inputs.required_modes(n)
    for m in need:
        assert c.modes[m] >= 10, (m, dict(c.modes))
    if "vb_comp" in need and n >= 64:
        assert all(c.lens[k] >= 10 for k in range(1, 6)), sorted(c.lens.items())
    _decodes(c, c.packed, c.off)
    bp, bo, k = v32_inputs.as_bx0(c.packed, c.off, n, c.base_n)
    if "plain" in need:
        assert k >= 10
        assert p4_modes.census32(bp, bo, n, c.base_n)[0]["bx0"] == k
        _decodes(c, bp, bo)
    if d1:
        assert (np.diff(c.vals.ravel().astype(np.int64)) < 0).any()  # the chained list wraps 2^32


@pytest.mark.parametrize("fmt,n", v32_inputs.VBYTE_CASES)
@pytest.mark.parametrize("d1", [False, True])
def test_vbyte32_census(fmt, n, d1):
    """400 units of vbyte32_gaps: at least half compressed vbyte, every
    marker length 1..5 at least 10 times."""
    c = v32_inputs.vbyte_case(fmt, n, d1)
    assert 2 * c.modes["vb_comp"] >= c.nu, dict(c.modes)
    for k in range(1, 6):
        assert c.lens[k] >= 10, sorted(c.lens.items())
    _decodes(c, c.packed, c.off)


def _mode(v):
    return p4_modes.parse32(oracle_lib.encode("32", v), 0, len(v))[0]


def test_no_vbyte_at_tiny_n():
    """p4Bits32 reads only the bit widths: over every multiset of n widths
    0..32 (n = 2, 3; v32_inputs.VB_MIN_N has the counts up to n = 9) no block
    is vbyte."""
    for n in (2, 3):
        for ws in itertools.combinations_with_replacement(range(33), n):
            v = np.array([(1 << (w - 1)) if w else 0 for w in ws], dtype=np.uint32)
            if len(set(ws)) == 1 and ws[0] > 1:
                v[0] ^= 1  # same width, not constant
            assert _mode(v) in ("zero", "const", "const32", "plain", "plain32", "bitmap"), ws


def test_smallest_n_with_compressed_vbyte():
    """A directed search: a base of width b, xn >= 11 exceptions whose excess
    has exactly d bits (one-byte markers) and one outlier ow bits over the
    base.  Compressed vbyte first appears at n = VB_COMP_MIN_N."""
    rng = np.random.default_rng(26)
    first = None
    for n in range(11, v32_inputs.VB_COMP_MIN_N + 1):
        for xn, d, b, ow in itertools.product(range(11, min(n, 15)), (5, 6, 7, 8), (0, 3), range(9, 30)):
            v = v32_inputs._below(rng, (n,), b)
            pos = rng.choice(n, size=xn + 1, replace=False)
            v[pos[:xn]] |= (rng.integers(1 << (d - 1), min(1 << d, 156), size=xn, dtype=np.uint64) << np.uint64(b)).astype(np.uint32)
            v[pos[xn]] = v32_inputs._of_width(rng, b + max(ow, d + 1))
            if _mode(v) == "vb_comp":
                first = n
                break
        if first:
            break
    assert first == v32_inputs.VB_COMP_MIN_N


@pytest.mark.parametrize("fmt,n", v32_inputs.PAD_CASES)
def test_padding_contract_of_the_oracle(fmt, n):
    """What test_v32_padding_contract holds the device to: without delta-1 a
    plain-mode block carries the low b bits of the caller's slots past n and
    no other mode reads them; with delta-1 they are ignored."""
    c = v32_inputs.v32_case(fmt, n, False, nu=200)
    dirty = v32_inputs.padded(c.vals, fmt, fill=0xDEADBEEF)
    pk, off = v32_inputs.oracle_stream(fmt, dirty, n)
    np.testing.assert_array_equal(off, c.off)
    differ = 0
    for i in range(c.nu):
        a, b = c.packed[int(off[i]): int(off[i + 1])], pk[int(off[i]): int(off[i + 1])]
        mode = p4_modes.parse32(pk, int(off[i]), n, c.base_n)[0]
        if not np.array_equal(a, b):
            differ += 1
            assert mode in ("plain", "plain32"), (i, mode)
    assert differ >= 10
    d = v32_inputs.v32_case(fmt, n, True, nu=200)
    pk1, off1 = v32_inputs.oracle_stream(fmt, v32_inputs.padded(d.vals, fmt, fill=0xDEADBEEF), n, d.starts)
    np.testing.assert_array_equal(off1, d.off)
    np.testing.assert_array_equal(pk1, d.packed)
