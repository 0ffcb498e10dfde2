"""GPU parity of the interleaved 64-bit family (p4{,D1}{Enc,Dec}128v64 and the
256v64 pair built from it) on every route: the generic kernels (k_enc_gr /
k_dec_gr on Fmt::V128X64: decode_block_g, plan_block_g, emit_block_g and
pack_elem's pair-swapped and horizontal base layouts) at every n below 128,
the run-pipelined kernels of p4_enc256v64.hip / p4_dec256v64.hip at n = 128
and for 256v64, and the per-block API.  Expected bytes and offsets are the
oracle's, decoded values are the numpy inputs, the decoders are fed the
oracle's stream.  tests/test_v64_inputs_cpu.py holds the same census
conditions without a device; tests/test_gpu_chained64.py takes the same units
through the chained decode."""
import ctypes

import numpy as np
import pytest

import v64_inputs

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def to_dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(DEV)


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
    got = out.cpu().numpy().view(np.uint64).reshape(nu, -1)
    np.testing.assert_array_equal(got[:, :n], vals, err_msg=what)


@pytest.mark.parametrize("fmt,n", v64_inputs.V64_CASES)
@pytest.mark.parametrize("d1", [False, True])
def test_v64_vs_oracle(fmt, n, d1):
    """128v64 at n = 1..128 (the reference takes any n: p4enc128v64_scalar.cpp,
    p4d1dec128v64_scalar.cpp; n = 127 runs on the generic kernels and n = 128
    on the run-pipelined ones) and 256v64 at 256: 1029 units = 16 full 64-unit
    workgroups plus a ragged run of 5, passed at the full stride, every class
    the encoder can produce at n -- each mode on the pair-swapped vertical base
    layout (b <= 32) and on the horizontal one (b > 32), width 63 / 64, and
    bitmap patches of bx <= 32 and bx > 32 -- in at least 10 units (counted in
    the oracle's bytes).  Bytes and offsets exact; delta-1 as one chained list
    from 2^64 - 4096 (it wraps 2^64; a short unit starts from the previous
    unit's value n - 1) and by per-unit starts.  Values and d_err clean from
    the oracle's stream, and from the stream with every plain block rewritten
    to the decode-only 0x80 | b, bx = 0 header."""
    c = v64_inputs.v64_case(fmt, n, d1)
    assert c.nu == 1029
    v64_inputs.check_census(c)
    what = f"{fmt} n={n} d1={d1}"
    if d1:
        _encode_exact(fmt, n, c.units, c.packed, c.off, what + " chained", d1=True, start0=v64_inputs.CHAIN_START0)
        _encode_exact(fmt, n, c.units, c.packed, c.off, what + " starts", d1=True, starts=to_dev(c.starts))
    else:
        _encode_exact(fmt, n, c.units, c.packed, c.off, what)
    _decode_exact(fmt, n, c.packed, c.off, c.vals, c.starts, what)
    bp, bo, kv, kh = v64_inputs.as_bx0(fmt, c.packed, c.off, n)
    if n > 1:
        assert kv >= 10 and kh >= 10, (kv, kh)
        _decode_exact(fmt, n, bp, bo, c.vals, c.starts, what + " bx0")


@pytest.mark.parametrize("fmt,n", v64_inputs.PAD_CASES)
def test_v64_padding_contract(fmt, n):
    """The slots past n of every unit hold 0xDEADBEEFDEADBEEF, then random
    words.  Without delta-1 the bytes are the oracle's for the same padded
    unit: a plain-mode block carries the slots' low b bits on either base
    layout (at width 64 the whole words), as the reference's
    bitpack128v64Scalar does, and no other mode reads them.  With delta-1 the
    slots are ignored -- the bytes are the oracle's for zero padding -- and
    the next unit of a chained list starts from value n - 1.  No length
    changes; the first n decoded values are exact."""
    rng = np.random.default_rng([78, n])
    plain = v64_inputs.v64_case(fmt, n, False)
    d1 = v64_inputs.v64_case(fmt, n, True)
    blocks = v64_inputs.blocks_of(fmt, plain.packed, plain.off, n)
    for name, fill in (("0xDEADBEEFDEADBEEF", 0xDEADBEEFDEADBEEF),
                       ("random", rng.integers(0, 1 << 64, size=(plain.nu, 128 - n), dtype=np.uint64))):
        what = f"{fmt} n={n} padding {name}"
        dirty = v64_inputs.padded(plain.vals, fmt, fill=fill)
        exp_packed, exp_off = v64_inputs.oracle_stream(fmt, dirty, n)
        np.testing.assert_array_equal(exp_off, plain.off)  # the padding never changes a length
        carried = {"plain_v": 0, "plain_h": 0, "plain63": 0}
        for i, _, blk in blocks:
            if not np.array_equal(exp_packed[int(exp_off[i]): blk.end], plain.packed[int(exp_off[i]): blk.end]):
                assert blk.split in carried, (i, blk.split)  # no other mode reads the padding
                carried[blk.split] += 1
        assert min(carried.values()) >= 1, carried  # plain blocks of each layout did carry the padding
        _encode_exact(fmt, n, dirty, exp_packed, exp_off, what)
        _decode_exact(fmt, n, exp_packed, exp_off, plain.vals, None, what)
        dirty = v64_inputs.padded(d1.vals, fmt, fill=fill)
        _encode_exact(fmt, n, dirty, d1.packed, d1.off, what + " d1 chained", d1=True, start0=v64_inputs.CHAIN_START0)
        _encode_exact(fmt, n, dirty, d1.packed, d1.off, what + " d1 starts", d1=True, starts=to_dev(d1.starts))
    _decode_exact(fmt, n, d1.packed, d1.off, d1.vals, d1.starts, f"{fmt} n={n} d1")


def _pick_units(c, count=64):
    """`count` units of a case with every required class of each of its
    128v64 blocks present: the first unit of each class, then the units in
    order."""
    first = {}
    for i, bn, blk in v64_inputs.blocks_of(c.fmt, c.packed, c.off, c.n):
        if blk.split in v64_inputs.required_modes(bn):
            first.setdefault((bn, blk.split), i)
    want = {(bn, m) for bn in v64_inputs.block_ns(c.fmt, c.n) for m in v64_inputs.required_modes(bn)}
    assert set(first) == want, want - set(first)
    picked = list(dict.fromkeys(list(first.values()) + list(range(c.nu))))[:count]
    assert len(picked) == count and set(first.values()) <= set(picked)
    return picked


@pytest.mark.parametrize("fmt,n", v64_inputs.PER_BLOCK_CASES)
@pytest.mark.parametrize("d1", [False, True])
def test_per_block_api_every_mode(fmt, n, d1):
    """tpf_p4{,D1}{Enc,Dec}128v64 at n = 7, 65, 127 and ...256v64 at n = 129,
    255 (split into 128v64 blocks like the reference), one call per unit on 64
    units of the cases above with every class of the format present: bytes,
    end pointers and values."""
    L = tpf.lib()
    c = v64_inputs.v64_case(fmt, n, d1)
    vt = ctypes.c_uint64
    enc_f = getattr(L, f"tpf_p4{'D1' if d1 else ''}Enc{fmt}")
    dec_f = getattr(L, f"tpf_p4{'D1' if d1 else ''}Dec{fmt}")
    for f in (enc_f, dec_f):
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p] + ([vt] if d1 else [])
        f.restype = ctypes.c_void_p
    for i in _pick_units(c):
        exp = c.packed[int(c.off[i]): int(c.off[i + 1])]
        st = [int(c.starts[i])] if d1 else []
        src = np.zeros(256 + 64, dtype=np.uint64)
        src[:n] = c.vals[i]
        out = np.zeros(len(exp) + 4096, dtype=np.uint8)
        end = enc_f(src.ctypes.data, n, out.ctypes.data, *st)
        assert end is not None, L.tpf_last_error()
        assert end - out.ctypes.data == len(exp), (fmt, n, i)
        np.testing.assert_array_equal(out[: len(exp)], exp, err_msg=f"{fmt} n={n} unit {i}")
        enc = np.concatenate([exp, np.zeros(64, dtype=np.uint8)])
        dec = np.zeros(256 + 64, dtype=np.uint64)
        end = dec_f(enc.ctypes.data, n, dec.ctypes.data, *st)
        assert end is not None, L.tpf_last_error()
        assert end - enc.ctypes.data == len(exp), (fmt, n, i)
        np.testing.assert_array_equal(dec[:n], c.vals[i], err_msg=f"{fmt} n={n} unit {i}")
