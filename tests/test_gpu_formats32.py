"""GPU parity of the 32-bit interleaved formats on the generic kernels
(k_enc_gr / k_dec_gr on Fmt::V128, Fmt::V256 with n != 256: decode_block_g,
plan_block_g, emit_block_g, vbyte_value<false>, vblen32) at every n below the
layout width, and of every 32-bit route -- the 256v32 hot path included -- on
compressed vbEnc32 streams with every marker length.  Expected bytes and
offsets are the oracle's, decoded values are the numpy inputs, the decoders
are fed the oracle's stream.  tests/test_v32_inputs_cpu.py holds the same
census conditions without a device."""
import numpy as np
import pytest

import v32_inputs

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def to_dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).to(DEV)


def _encode_exact(fmt, n, units, exp_packed, exp_off, what, **kw):
    packed, offs = tpf.enc_batch(fmt, to_dev(units.ravel()), len(units), n, **kw)
    np.testing.assert_array_equal(offs.cpu().numpy().astype(np.uint64), exp_off, err_msg=f"{what}: offsets")
    np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed, err_msg=f"{what}: bytes")


def _decode_exact(fmt, n, packed, off, vals, starts, what):
    nu = len(vals)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = tpf.dec_batch(fmt, torch.from_numpy(packed).to(DEV), torch.from_numpy(off.astype(np.int64)).to(DEV), nu, n,
                        starts=None if starts is None else to_dev(starts), err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1, f"{what}: length check failed at unit {int(err.item())}"
    got = out.cpu().numpy().view(np.uint32).reshape(nu, -1)
    np.testing.assert_array_equal(got[:, :n], vals, err_msg=what)


def _roundtrip(c, what):
    """Encode exact (D1: one chained list and per-unit starts), decode exact."""
    if c.d1:
        _encode_exact(c.fmt, c.n, c.units, c.packed, c.off, what + " chained", d1=True, start0=v32_inputs.CHAIN_START0)
        _encode_exact(c.fmt, c.n, c.units, c.packed, c.off, what + " starts", d1=True, starts=to_dev(c.starts))
    else:
        _encode_exact(c.fmt, c.n, c.units, c.packed, c.off, what)
    _decode_exact(c.fmt, c.n, c.packed, c.off, c.vals, c.starts, what)


@pytest.mark.parametrize("fmt,n", v32_inputs.V32_CASES)
@pytest.mark.parametrize("d1", [False, True])
def test_v32_vs_oracle(fmt, n, d1):
    """128v32 at n = 1..128 and 256v32 at n = 1..255 (the reference takes any
    n: p4enc128v32_scalar.cpp, p4dec128v32_scalar.cpp and the 256v32 pair):
    1029 units = 16 full 64-unit workgroups (four waves of 16-unit runs) plus
    a ragged run of 5, passed at the full stride, every mode the encoder can
    produce at n in at least 10 units (census32 of the oracle's bytes).
    Bytes and offsets exact; delta-1 as one chained list from 0xFFFFF000 (it
    wraps 2^32; a unit starts from the previous unit's value n - 1) and by
    per-unit starts.  Values and d_err clean from the oracle's stream, and
    from the stream with every plain block rewritten to the decode-only
    0x80 | b, bx = 0 header."""
    c = v32_inputs.v32_case(fmt, n, d1)
    assert c.nu == 1029
    need = v32_inputs.required_modes(n)
    for m in need:
        assert c.modes[m] >= 10, (m, dict(c.modes))
    what = f"{fmt} n={n} d1={d1}"
    _roundtrip(c, what)
    bp, bo, k = v32_inputs.as_bx0(c.packed, c.off, n, c.base_n)
    if "plain" in need:
        assert k >= 10
        _decode_exact(fmt, n, bp, bo, c.vals, c.starts, what + " bx0")


@pytest.mark.parametrize("fmt,n", v32_inputs.PAD_CASES)
def test_v32_padding_contract(fmt, n):
    """The slots past n of every unit hold 0xDEADBEEF, then random words.
    Without delta-1 the bytes are the oracle's for the same padded unit: a
    plain-mode block carries the slots' low b bits, as the reference's does,
    and no other mode reads them.  With delta-1 the slots are ignored -- the
    bytes are the oracle's for zero padding -- and the next unit of a chained
    list starts from value n - 1.  The first n decoded values are exact."""
    rng = np.random.default_rng([77, n])
    u = v32_inputs.WIDTH[fmt]
    plain = v32_inputs.v32_case(fmt, n, False)
    d1 = v32_inputs.v32_case(fmt, n, True)
    carried = 0
    for name, fill in (("0xDEADBEEF", 0xDEADBEEF), ("random", rng.integers(0, 1 << 32, size=(plain.nu, u - n), dtype=np.uint64))):
        what = f"{fmt} n={n} padding {name}"
        dirty = v32_inputs.padded(plain.vals, fmt, fill=fill)
        exp_packed, exp_off = v32_inputs.oracle_stream(fmt, dirty, n)
        np.testing.assert_array_equal(exp_off, plain.off)  # the padding never changes a length
        carried += int(not np.array_equal(exp_packed, plain.packed))
        _encode_exact(fmt, n, dirty, exp_packed, exp_off, what)
        _decode_exact(fmt, n, exp_packed, exp_off, plain.vals, None, what)
        dirty = v32_inputs.padded(d1.vals, fmt, fill=fill)
        _encode_exact(fmt, n, dirty, d1.packed, d1.off, what + " d1 chained", d1=True, start0=v32_inputs.CHAIN_START0)
        _encode_exact(fmt, n, dirty, d1.packed, d1.off, what + " d1 starts", d1=True, starts=to_dev(d1.starts))
    assert carried == 2  # the plain-mode blocks did carry the padding
    _decode_exact(fmt, n, d1.packed, d1.off, d1.vals, d1.starts, f"{fmt} n={n} d1")


@pytest.mark.parametrize("fmt,n", v32_inputs.VBYTE_CASES)
def test_vbyte32_compressed_every_marker_form(fmt, n):
    """The COMPRESSED 32-bit vbyte stream (vbEnc32 / vbDec32,
    p4_scalar_internal.cpp:47-89, :163-237) on every 32-bit route: the
    generic kernels' vbyte_value<false> (the 0xFC and 0xFD.. branches),
    vbyte_len<false>, vblen32 and emit_block_g's long forms, and at (256v32,
    256) the hot encoder and decoder.  400 units, at least half of them
    compressed vbyte and every marker length 1..5 at least 10 times (counted
    in the oracle's bytes); bytes, offsets and values exact, plain and D1."""
    for d1 in (False, True):
        c = v32_inputs.vbyte_case(fmt, n, d1)
        assert c.nu == 400 and 2 * c.modes["vb_comp"] >= c.nu, dict(c.modes)
        for k in range(1, 6):
            assert c.lens[k] >= 10, sorted(c.lens.items())
        _roundtrip(c, f"{fmt} n={n} d1={d1}")
    if (fmt, n) != ("256v32", 256):
        return
    # the same gaps as one chained list through tpf_p4d1dec256v32_chained: the
    # sums pass and the decode pass both parse the stream
    packed = torch.from_numpy(c.packed).to(DEV)
    offs = torch.from_numpy(c.off.astype(np.int64)).to(DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = tpf.dec256v32_chained(packed, offs, c.nu, start0=v32_inputs.CHAIN_START0, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(c.nu, 256), c.vals)
    chain = tpf.D1Chain(packed, offs, c.nu)
    total = chain.sums(err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    want = int((c.gaps.astype(np.uint64) + np.uint64(1)).sum()) & 0xFFFFFFFF
    assert int(total.item()) & 0xFFFFFFFF == want
    out = chain.decode(v32_inputs.CHAIN_START0, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(c.nu, 256), c.vals)
