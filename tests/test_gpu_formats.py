"""GPU parity for every format of include/turbopfor.h through the batched
C-ABI (tpf_enc_batch / tpf_dec_batch): byte-exact encoder output and
bit-exact decoding against the golden fixtures generated from the
reference's src/scalar codec, plus oracle cross-checks at larger sizes."""
import collections

import numpy as np
import pytest

import datagen
import golden_io
import h64_inputs
import oracle_lib
import p4_modes

torch = pytest.importorskip("torch")
tpf = pytest.importorskip("turbopfor_amd")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U64 = (1 << 64) - 1

FAMILIES = [("g32.bin", "32"), ("g128v32.bin", "128v32"), ("g256v32.bin", "256v32"),
            ("g128v64.bin", "128v64"), ("g256v64.bin", "256v64"), ("g64.bin", "64"),
            ("g32vb.bin", "32"), ("g128v32s.bin", "128v32"), ("g256v32s.bin", "256v32"),
            ("g128v64s.bin", "128v64"), ("g256v64s.bin", "256v64")]


def to_dev(arr, wide):
    a = np.ascontiguousarray(arr, dtype=np.uint64 if wide else np.uint32)
    return torch.from_numpy(a.view(np.int64 if wide else np.int32)).to(DEV)


def groups(fname, fmt):
    """Golden records by (n, d1).  Batches hold whole 256v64 units; shorter
    256v64 vectors go through the per-block API (test_gpu_dropin.py)."""
    g = collections.defaultdict(list)
    for r in golden_io.load(fname):
        if fmt == "256v64" and r.n != 256:
            continue
        g[(r.n, r.d1)].append(r)
    return g


@pytest.mark.parametrize("fname,fmt", FAMILIES)
def test_golden_encode(fname, fmt):
    wide = fmt in ("64", "128v64", "256v64")
    for (n, d1), recs in groups(fname, fmt).items():
        recs = [r for r in recs if not r.decode_only]
        if not recs:
            continue
        u = tpf.unit_values(fmt, n)
        vals = np.zeros((len(recs), u), dtype=np.uint64 if wide else np.uint32)
        for i, r in enumerate(recs):
            vals[i, :n] = r.values
        starts = to_dev(np.array([r.start for r in recs], dtype=np.uint64), wide) if d1 else None  # (a list of ints past 2^63 would go float64)
        packed, offs = tpf.enc_batch(fmt, to_dev(vals.ravel(), wide), len(recs), n, d1=d1, starts=starts)
        pk = packed.cpu().numpy().tobytes()
        of = offs.cpu().numpy()
        for i, r in enumerate(recs):
            mine = pk[of[i]:of[i + 1]]
            if r.padding_unpinned:  # padding bits: the zero convention (oracle), length as the reference
                assert len(mine) == len(r.enc), f"{fmt} n={n} d1={d1} record {i}"
                assert mine == oracle_lib.encode(fmt, r.values, d1=d1, start=r.start), f"{fmt} n={n} record {i}"
            else:
                assert mine == r.enc, f"{fmt} n={n} d1={d1} record {i}"


@pytest.mark.parametrize("fname,fmt", FAMILIES)
def test_golden_decode(fname, fmt):
    wide = fmt in ("64", "128v64", "256v64")
    for (n, d1), recs in groups(fname, fmt).items():
        u = tpf.unit_values(fmt, n)
        offs = np.zeros(len(recs) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(r.enc) for r in recs])
        packed = torch.from_numpy(np.frombuffer(b"".join(x.enc for x in recs), dtype=np.uint8).copy()).to(DEV)
        starts = to_dev(np.array([r.start for r in recs], dtype=np.uint64), wide) if d1 else None  # (a list of ints past 2^63 would go float64)
        err = torch.zeros(1, dtype=torch.int64, device=DEV)
        out = tpf.dec_batch(fmt, packed, torch.from_numpy(offs).to(DEV), len(recs), n, starts=starts, err=err)
        torch.cuda.synchronize()
        assert int(err.item()) == -1, f"{fmt} n={n}: length check failed at {int(err.item())}"
        got = out.cpu().numpy().view(np.uint64 if wide else np.uint32).reshape(len(recs), u)
        for i, r in enumerate(recs):
            np.testing.assert_array_equal(got[i, :n], r.values, err_msg=f"{fmt} n={n} d1={d1} record {i}")


@pytest.mark.parametrize("bw", [4, 16, 31, 33, 40, 63, 64])
@pytest.mark.parametrize("exc", [0, 5, 25])
def test_256v64_roundtrip_vs_oracle(bw, exc):
    blocks = datagen.c4_blocks64(64, bw, exc, seed=bw * 7 + exc)
    exp_packed, exp_off = oracle_lib.enc256v64_batch(blocks)
    packed, offs = tpf.enc_batch("256v64", to_dev(blocks.ravel(), True), len(blocks), 256)
    np.testing.assert_array_equal(offs.cpu().numpy().astype(np.uint64), exp_off)
    np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed)
    out = tpf.dec_batch("256v64", packed, offs, len(blocks), 256)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64).reshape(-1, 256), blocks)


def test_256v64_d1_chained_vs_oracle():
    rng = np.random.default_rng(3)
    g = rng.integers(1, 1 << 20, size=(300 * 256,), dtype=np.uint64)
    vals = np.cumsum(g).astype(np.uint64).reshape(300, 256)
    starts = np.zeros(300, dtype=np.uint64)
    starts[1:] = vals[:-1, -1]
    exp_packed, exp_off = oracle_lib.enc256v64_batch(vals, starts=starts)
    packed, offs = tpf.enc_batch("256v64", to_dev(vals.ravel(), True), 300, 256, d1=True, start0=0)
    np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed)
    out = tpf.dec_batch("256v64", packed, offs, 300, 256, starts=to_dev(starts, True))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64).reshape(-1, 256), vals)


@pytest.mark.parametrize("n", [1, 7, 64, 127, 200, 256])
def test_p4enc32_vs_oracle(n):
    """C1-style horizontal blocks (p4Enc32/p4Dec32), incl. n=127 bw=8."""
    rng = np.random.default_rng(n)
    nb = 400
    bw = rng.integers(1, 33, size=(nb, 1))
    vals = (rng.integers(0, 1 << 62, size=(nb, n), dtype=np.uint64) & ((np.uint64(1) << bw.astype(np.uint64)) - np.uint64(1)))
    exc = rng.random((nb, n)) < 0.1
    vals = np.where(exc, rng.integers(0, 1 << 32, size=(nb, n), dtype=np.uint64), vals).astype(np.uint32)
    exp_packed, exp_off = oracle_lib.enc32_batch(vals)
    packed, offs = tpf.enc_batch("32", to_dev(vals.ravel(), False), nb, n)
    np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed)
    out = tpf.dec_batch("32", packed, offs, nb, n)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(nb, n), vals)


@pytest.mark.parametrize("n", [127, 256])
def test_p4dec32_corrupt_offsets_reported(n):
    """The run-pipelined generic decoder reports the first block whose parsed
    length disagrees with the offsets (d_err), like the 256v32 kernel."""
    rng = np.random.default_rng(7 + n)
    nb = 300
    vals = rng.integers(0, 1 << 11, size=(nb, n), dtype=np.uint64).astype(np.uint32)
    exp_packed, exp_off = oracle_lib.enc32_batch(vals)
    packed = torch.from_numpy(exp_packed).to(DEV)
    bad = exp_off.astype(np.int64).copy()
    bad[200] += 1  # block 199 looks one byte longer, block 200 one shorter
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.dec_batch("32", packed, torch.from_numpy(bad).to(DEV), nb, n, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 199
    out = tpf.dec_batch("32", packed, torch.from_numpy(exp_off.astype(np.int64)).to(DEV), nb, n, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1  # UINT64_MAX: every block consistent
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(nb, n), vals)


def _h32_values(rng, nb, n):
    """Blocks that exercise every p4Dec32 mode the windowed decoder parses:
    constant, plain, bitmap and vbyte exceptions (raw and compressed), at base
    widths 0..32 -- runs of small blocks share one staged window, 1 KB blocks
    split runs into windows of two."""
    bw = rng.integers(0, 33, size=(nb, 1)).astype(np.uint64)
    vals = rng.integers(0, 1 << 62, size=(nb, n), dtype=np.uint64) & ((np.uint64(1) << bw) - np.uint64(1))
    rate = rng.choice([0.0, 0.02, 0.1, 0.3], size=(nb, 1))
    exc = rng.random((nb, n)) < rate
    big = rng.integers(0, 1 << 32, size=(nb, n), dtype=np.uint64) >> rng.integers(0, 24, size=(nb, 1)).astype(np.uint64)
    vals = np.where(exc, big, vals).astype(np.uint32)
    const = rng.random(nb) < 0.1
    vals[const] = vals[const, :1]
    return vals


@pytest.mark.parametrize("n", [1, 33, 64, 65, 127, 128, 129, 255, 256])
@pytest.mark.parametrize("d1", [False, True])
def test_p4dec32_windows_vs_oracle(n, d1):
    """k_dec_h32w (p4Dec32 / p4D1Dec32 batches, n <= 256): mixed modes and
    widths over 64-block wave runs and their staging windows, ragged last run
    (nb % 64 != 0), bit-exact against the oracle's decode of the oracle's
    encoding (reference src/scalar/p4dec32.cpp:70-142, p4d1dec32.cpp)."""
    rng = np.random.default_rng(1000 * n + d1)
    nb = 3001
    vals = _h32_values(rng, nb, n)
    starts = rng.integers(0, 1 << 32, size=nb, dtype=np.uint64).astype(np.uint32) if d1 else None
    if d1:
        # p4D1Enc32 codes vals as strictly increasing deltas from the start
        vals = (np.cumsum(vals.astype(np.uint64) + 1, axis=1) + starts[:, None].astype(np.uint64) - 1).astype(np.uint32)
    packed, off = oracle_lib.enc32_batch(vals, starts=starts)
    exp = oracle_lib.dec32_batch(packed, off, nb, n, starts=starts)
    np.testing.assert_array_equal(exp, vals)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = tpf.dec_batch("32", torch.from_numpy(packed).to(DEV), torch.from_numpy(off.astype(np.int64)).to(DEV), nb, n,
                        starts=to_dev(starts, False) if d1 else None, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(nb, n), vals)


def test_p4dec32_windows_oversize_block_reported():
    """An offset pair that claims more bytes than a staging window (or runs
    past the stream) is reported through d_err, blocks before it stay exact."""
    rng = np.random.default_rng(5)
    nb, n = 200, 127
    vals = rng.integers(0, 1 << 9, size=(nb, n), dtype=np.uint64).astype(np.uint32)
    packed, off = oracle_lib.enc32_batch(vals)
    pad = np.zeros(len(packed) + 8192, dtype=np.uint8)
    pad[: len(packed)] = packed
    bad = off.astype(np.int64).copy()
    bad[71:] += 4000  # block 70 claims 4000 extra bytes
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = tpf.dec_batch("32", torch.from_numpy(pad).to(DEV), torch.from_numpy(bad).to(DEV), nb, n, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 70
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(nb, n)[:70], vals[:70])
    err.zero_()
    short = torch.from_numpy(packed[: int(off[150])].copy()).to(DEV)  # stream ends at block 150
    tpf.dec_batch("32", short, torch.from_numpy(off.astype(np.int64)).to(DEV), nb, n, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 150


def test_256v64_vbyte_every_marker_form():
    """128v64 vbyte exceptions in the RAW form: three large exceptions over a
    3-bit base make the encoder pick vbyte mode, and with three exceptions the
    compressed stream can never be 32 bytes shorter than the raw one
    (sumlen + 32 > 8 * xn), so every vbyte block carries the 0xFF marker and
    eight bytes per exception, of every magnitude from bit 3 to bit 63.  (The
    compressed forms are test_wide_vbyte_compressed_every_marker_form's.)
    Bytes against the oracle, values back from the batch decoder (plain and D1
    per-unit starts)."""
    rng = np.random.default_rng(11)
    nu = 512
    blocks = rng.integers(0, 8, size=(nu, 256), dtype=np.uint64)
    shifts = np.arange(3, 64)
    for i in range(nu):
        pos = rng.choice(256, size=3, replace=False)
        for k, p in enumerate(pos):
            s = int(shifts[(3 * i + k) % len(shifts)])
            blocks[i, p] = np.uint64((1 << s) | int(rng.integers(0, 1 << min(s, 62))))
    exp_packed, exp_off = oracle_lib.enc256v64_batch(blocks)
    packed, offs = tpf.enc_batch("256v64", to_dev(blocks.ravel(), True), nu, 256)
    np.testing.assert_array_equal(offs.cpu().numpy().astype(np.uint64), exp_off)
    np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed)
    heads = exp_packed[exp_off[:-1].astype(np.int64)]
    assert int(((heads & 0xC0) == 0x40).sum()) > nu // 2, "vbyte mode not chosen"
    modes, _ = p4_modes.census64(exp_packed, exp_off, 128, halves=2, base_n=128)
    assert modes["vb_raw"] > nu and modes["vb_comp"] == 0, modes  # the vbyte halves carry the 0xFF raw marker
    out = tpf.dec_batch("256v64", packed, offs, nu, 256)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64).reshape(-1, 256), blocks)
    # the same exceptions through D1 (gaps = the blocks' values)
    vals = np.cumsum(blocks.ravel() + np.uint64(1), dtype=np.uint64).reshape(nu, 256) - np.uint64(1)
    starts = np.zeros(nu, dtype=np.uint64)
    starts[1:] = vals[:-1, -1]
    exp_packed, exp_off = oracle_lib.enc256v64_batch(vals, starts=starts)
    packed, offs = tpf.enc_batch("256v64", to_dev(vals.ravel(), True), nu, 256, d1=True, start0=0)
    np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed)
    out = tpf.dec_batch("256v64", packed, offs, nu, 256, starts=to_dev(starts, True))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64).reshape(-1, 256), vals)


# ---- the horizontal 64-bit family: p4Enc64 / p4Dec64 / p4D1Enc64 / p4D1Dec64 ----
def _enc64_check(vals, n, starts=None, start0=0):
    """tpf_enc_batch fmt "64" against the oracle: bytes and offsets (D1: the
    chained list form and per-unit starts)."""
    nb = len(vals)
    exp_packed, exp_off = oracle_lib.enc64_batch(vals, starts=starts)
    dv = to_dev(vals.ravel(), True)
    variants = [dict()] if starts is None else [dict(d1=True, start0=start0), dict(d1=True, starts=to_dev(starts, True))]
    for kw in variants:
        packed, offs = tpf.enc_batch("64", dv, nb, n, **kw)
        np.testing.assert_array_equal(offs.cpu().numpy().astype(np.uint64), exp_off, err_msg=str(sorted(kw)))
        np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed, err_msg=str(sorted(kw)))
    return exp_packed, exp_off


def _dec64_check(packed, off, vals, n, starts=None):
    nb = len(vals)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = tpf.dec_batch("64", torch.from_numpy(packed).to(DEV), torch.from_numpy(off.astype(np.int64)).to(DEV), nb, n,
                        starts=None if starts is None else to_dev(starts, True), err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64).reshape(nb, n), vals)


def _p4enc64_body(n, d1, nb, seed):
    rng = np.random.default_rng(seed)
    gaps = h64_inputs.h64_values(rng, nb, n)
    start0 = int(rng.integers(0, 1 << 64, dtype=np.uint64)) if d1 else 0
    vals, starts = h64_inputs.d1_list(gaps, start0) if d1 else (gaps, None)
    exp_packed, exp_off = oracle_lib.enc64_batch(vals, starts=starts)
    np.testing.assert_array_equal(oracle_lib.dec64_batch(exp_packed, exp_off, nb, n, starts=starts), vals)
    # which modes the inputs reach, from the oracle's bytes (D1 codes the gaps themselves)
    modes, lens = p4_modes.census64(exp_packed, exp_off, n)
    _enc64_check(vals, n, starts, start0)
    _dec64_check(exp_packed, exp_off, vals, n, starts)
    # the decode-only header 0x80 | b with bx == 0 in place of every plain block
    bp, bo, k = h64_inputs.as_bx0(exp_packed, exp_off, n)
    if k:
        _dec64_check(bp, bo, vals, n, starts)
    return modes, lens, k


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256])
@pytest.mark.parametrize("d1", [False, True])
def test_p4enc64_vs_oracle(n, d1):
    """k_enc_gr / k_dec_gr on Fmt::H64 (reference src/scalar/p4enc64.cpp,
    p4dec64.cpp, p4d1enc64.cpp, p4d1dec64.cpp): 1029 blocks = 16 full
    64-block workgroups (four waves of kGRun = 16) plus a ragged run of 5, n
    across the bitmap-word and byte boundaries, every mode of the format in at
    least 10 blocks (counted in the oracle's bytes): bytes, offsets and values
    bit-exact, D1 as one chained list that wraps 2^64 and by per-unit starts."""
    modes, lens, bx0 = _p4enc64_body(n, d1, 1029, 64000 + 10 * n + d1)
    if n == 1:  # one value: all zero or constant
        need = ["zero", "const", "const63"]
    elif n == 2:  # vbyte never beats the bitmap patch of one exception
        need = ["zero", "const", "const63", "plain", "plain63", "bitmap"]
    else:
        need = ["zero", "const", "const63", "plain", "plain63", "bitmap", "vb_raw", "vb_comp"]
        assert bx0 >= 10
        assert all(lens[k] >= 1 for k in range(1, 10)), sorted(lens.items())
    for m in need:
        assert modes[m] >= 10, (m, dict(modes))


@pytest.mark.parametrize("nb", [1, 17])
@pytest.mark.parametrize("d1", [False, True])
def test_p4enc64_short_batches(nb, d1):
    """The same body at n = 256 with one block and with 17 (one full wave run
    and a run of one)."""
    _p4enc64_body(256, d1, nb, 64900 + 10 * nb + d1)


def test_p4enc64_slot_edge():
    """The largest p4Enc64 blocks -- n = 256 plain at width 64 and at width 63
    (stored as 64): 2,049 bytes each, against the 2,432-byte per-wave slot of
    the encoder's image and the decoder's staging -- interleaved with one-byte
    all-zero blocks, so that a run stages the extremes side by side."""
    rng = np.random.default_rng(6463)
    vals = np.zeros((800, 256), dtype=np.uint64)
    vals[0::4] = rng.integers(0, 1 << 64, size=(200, 256), dtype=np.uint64)
    vals[0::4, 0] |= np.uint64(1 << 63)
    vals[2::4] = rng.integers(0, 1 << 63, size=(200, 256), dtype=np.uint64)
    vals[2::4, 255] |= np.uint64(1 << 62)
    exp_packed, exp_off = _enc64_check(vals, 256)
    sizes = np.diff(exp_off.astype(np.int64))
    assert sizes.max() == 2049 and (sizes == 2049).sum() == 400 and (sizes == 1).sum() == 400
    assert set(exp_packed[exp_off[:-1:2].astype(np.int64)].tolist()) == {63}  # header 63 for both widths
    _dec64_check(exp_packed, exp_off, vals, 256)


def _wide_oracle(fmt, vals, starts=None):
    if fmt == "64":
        return oracle_lib.enc64_batch(vals, starts=starts)
    if fmt == "256v64":
        return oracle_lib.enc256v64_batch(vals, starts=starts)
    encs = [oracle_lib.encode(fmt, v, d1=starts is not None, start=0 if starts is None else int(starts[i]))
            for i, v in enumerate(vals)]
    off = np.concatenate([[0], np.cumsum([len(e) for e in encs])]).astype(np.uint64)
    return np.frombuffer(b"".join(encs), dtype=np.uint8).copy(), off


WIDE_VBYTE = [("64", 65), ("64", 256), ("128v64", 128), ("256v64", 256)]


@pytest.mark.parametrize("fmt,n", WIDE_VBYTE)
def test_wide_vbyte_compressed_every_marker_form(fmt, n):
    """The COMPRESSED 64-bit vbyte stream (vbEnc64 / vbDec64,
    p4_scalar_internal.cpp:447-526): the window parse of vbyte_exceptions_g,
    the long-form branch of vbyte_value, vblen64 and the compressed writer of
    emit_block_g, and the 128v64 / 256v64 kernels that share them.  At least
    half the blocks are compressed vbyte and every marker length 1..9 occurs at
    least 10 times (counted in the oracle's bytes); bytes, offsets and values
    exact, plain and D1."""
    nu = 400
    gaps = h64_inputs.wide_vbyte_gaps(fmt, n, nu)
    halves, bn, base_n = (2, 128, 128) if fmt == "256v64" else (1, n, None if fmt == "64" else 128)
    vals_d1, starts = h64_inputs.d1_list(gaps, 0)
    for vals, st in ((gaps, None), (vals_d1, starts)):
        exp_packed, exp_off = _wide_oracle(fmt, vals, st)
        modes, lens = p4_modes.census64(exp_packed, exp_off, bn, halves=halves, base_n=base_n)
        assert 2 * modes["vb_comp"] >= nu * halves, dict(modes)
        for k in range(1, 10):
            assert lens[k] >= 10, sorted(lens.items())
        dv = to_dev(vals.ravel(), True)
        for kw in ([dict()] if st is None else [dict(d1=True, start0=0), dict(d1=True, starts=to_dev(st, True))]):
            packed, offs = tpf.enc_batch(fmt, dv, nu, n, **kw)
            np.testing.assert_array_equal(offs.cpu().numpy().astype(np.uint64), exp_off)
            np.testing.assert_array_equal(packed.cpu().numpy(), exp_packed)
        err = torch.zeros(1, dtype=torch.int64, device=DEV)
        out = tpf.dec_batch(fmt, torch.from_numpy(exp_packed).to(DEV), torch.from_numpy(exp_off.astype(np.int64)).to(DEV), nu, n,
                            starts=None if st is None else to_dev(st, True), err=err)
        torch.cuda.synchronize()
        assert int(err.item()) == -1
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64).reshape(nu, -1), vals)


def test_p4dec64_corrupt_offsets_reported():
    """As test_p4dec32_corrupt_offsets_reported, for p4Dec64 at n = 256: the
    first block whose parsed length disagrees with the offsets is reported."""
    rng = np.random.default_rng(7 + 64)
    nb, n = 300, 256
    vals = rng.integers(0, 1 << 11, size=(nb, n), dtype=np.uint64)
    exp_packed, exp_off = oracle_lib.enc64_batch(vals)
    packed = torch.from_numpy(exp_packed).to(DEV)
    bad = exp_off.astype(np.int64).copy()
    bad[200] += 1  # block 199 looks one byte longer, block 200 one shorter
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    tpf.dec_batch("64", packed, torch.from_numpy(bad).to(DEV), nb, n, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 199
    out = tpf.dec_batch("64", packed, torch.from_numpy(exp_off.astype(np.int64)).to(DEV), nb, n, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == -1  # UINT64_MAX: every block consistent
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64).reshape(nb, n), vals)
